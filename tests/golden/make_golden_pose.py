"""Golden vectors for the camera-pose glue, recorded by RUNNING the reference's own functions (build container only, CPU only).

Run:  python tests/golden/make_golden_pose.py     (needs the reference tree; writes pose_heads.npz, pose_pick.npz, pose_cameras.npz and
                                                    pose_random_view.npz beside this file)

As tests/golden/make_golden_articulation.py: nothing of the reference is imported.  The two predictor files and Fauna.py are read with
``ast``; forward_pose, both sample_pose_hypothesis_from_quad_predictions, get_camera_extrinsics_from_pose, lookat_forward_to_rot_matrix
and get_random_view_mask are compiled on their own and called with a SimpleNamespace for ``self``: ``netPose`` returns the case's raw
tensor, ``self.render`` records its mvp, w2c and campos arguments and returns a dummy, and ``torch.randperm`` / ``torch.randint`` are
wrapped so that they return the case's permutations / degrees, which are recorded as inputs beside the results.  ``util.perspective`` is
the package's own.  Only inputs and results are written; no reference source travels.  The inputs are rebuilt from tests/pose_cases.py.
"""
import ast
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the package, for util.perspective
import pose_cases as C  # noqa: E402
from make_golden import REF  # noqa: E402

util = importlib.import_module("3danimals_amd.model.render.util")


class Torch:
    """``torch`` with randperm and randint answering from a queue; what they answered is kept."""

    def __init__(self):
        self.queue, self.drawn = [], []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _next(self, n):
        value = self.queue.pop(0)
        assert len(value) == n
        self.drawn.append(value.clone())
        return value.clone()

    def randperm(self, n, device=None):
        return self._next(n)

    def randint(self, high, size):
        return self._next(size[0])


def functions_of(rel_path, class_name, names, env):
    path = os.path.join(REF, *rel_path)
    tree = ast.parse(open(path).read(), path)
    body = tree.body if class_name is None else next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == class_name).body
    out = {}
    for fn in body:
        if isinstance(fn, ast.FunctionDef) and fn.name in names:
            fn.decorator_list = []  # (@staticmethod: called as a plain function here)
            scope = dict(env)
            exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), scope)
            out[fn.name] = scope[fn.name]
    assert set(out) == set(names), (rel_path, sorted(out))
    return out


def save(name, data):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), len(data), "arrays")


def main():
    T = Torch()
    env = dict(torch=T, nn=torch.nn, F=F, np=np, util=util)
    base_py, fauna_py = ("model", "predictors", "InstancePredictorBase.py"), ("model", "predictors", "InstancePredictorFauna.py")
    env.update(functions_of(base_py, None, ("lookat_forward_to_rot_matrix",), env))
    base = functions_of(base_py, "InstancePredictorBase", ("forward_pose", "sample_pose_hypothesis_from_quad_predictions",
                                                           "get_camera_extrinsics_from_pose"), env)
    fauna = functions_of(fauna_py, "InstancePredictorFauna", ("sample_pose_hypothesis_from_quad_predictions",), env)
    model = functions_of(("model", "models", "Fauna.py"), "FaunaModel", ("get_random_view_mask",), env)

    heads, pick, cameras = {}, {}, {}
    for name in list(C.FUSED_CASES):
        c = C.build_fused(name)
        me = SimpleNamespace(cfg_pose=SimpleNamespace(architecture="encoder_dino_patch_key", rot_rep="octlookat" if c["oct"] else "quadlookat",
                                                      lookat_zeroy=c["zeroy"], cam_pos_z_offset=C.Z_OFFSET, fov=C.FOV),
                             netPose=lambda _: c["raw"].clone(), max_trans_xyz_range=c["max_trans"], orthant_signs=c["signs"], num_pose_hypos=c["H"])
        poses_raw = base["forward_pose"](me, None, None)
        heads[name] = poses_raw.numpy()
        sample = (fauna if c["temp_clip_max"] == 10.0 else base)["sample_pose_hypothesis_from_quad_predictions"]
        assert c["temp_clip_max"] in (10.0, 100.0)
        T.queue = [c["rand_perm"], c["best_perm"]] if c["random_sample"] else []
        T.drawn = []
        pose_raw, pose, aux = sample(poses_raw, c["total_iter"], rot_temp_scalar=1.0, num_hypos=c["H"], naive_probs_iter=C.NAIVE_ITER,
                                     best_pose_start_iter=C.BEST_ITER, random_sample=c["random_sample"])
        assert not T.queue and len(T.drawn) == (2 if c["random_sample"] else 0)
        pick[name + "/pose_raw"], pick[name + "/pose"] = pose_raw.numpy(), pose.numpy()
        for k, v in aux.items():
            pick[f"{name}/{k}"] = v.numpy()
        for k, v in zip(("rand_perm", "best_perm"), T.drawn):
            pick[f"{name}/{k}"] = v.numpy()
        kw = {} if c["offset_extra"] is None else dict(offset_extra=c["offset_extra"])
        for k, v in zip(("mvp", "w2c", "campos"), base["get_camera_extrinsics_from_pose"](me, pose, **kw)):
            cameras[f"{name}/{k}"] = v.numpy()
        print(name, aux["rot_idx"].tolist()[:8], aux["rand_pose_flag"].tolist()[:8])
    for name in C.CAMERA_CASES:
        c = C.build_cameras(name)
        me = SimpleNamespace(cfg_pose=SimpleNamespace(cam_pos_z_offset=C.Z_OFFSET, fov=C.FOV))
        kw = {} if c["offset_extra"] is None else dict(offset_extra=c["offset_extra"])
        for k, v in zip(("mvp", "w2c", "campos"), base["get_camera_extrinsics_from_pose"](me, c["pose"], **kw)):
            cameras[f"alone_{name}/{k}"] = v.numpy()
    save("pose_heads.npz", heads)
    save("pose_pick.npz", pick)
    save("pose_cameras.npz", cameras)

    views = {}
    for name in C.RANDOM_VIEW_CASES:
        c = C.build_random_view(name)
        seen = {}

        def render(**kw):
            seen.update({k: kw[k].clone() for k in ("mvp", "w2c", "campos")})
            return [torch.zeros(len(c["degree"]), 4, 1, 1)]

        me = SimpleNamespace(accelerator=SimpleNamespace(device="cpu"), cfg_render=SimpleNamespace(cam_pos_z_offset=C.Z_OFFSET, fov=C.FOV), render=render)
        T.queue, T.drawn = [c["rand_degree"]], []
        out = model["get_random_view_mask"](me, c["w2c_pred"], [None] * len(c["degree"]), None, 1, bins=c["bins"])
        assert torch.equal(out["rand_degree"], c["rand_degree"]) and len(T.drawn) == 1
        views[name + "/rand_degree"] = T.drawn[0].numpy()
        for k, v in seen.items():
            views[f"{name}/{k}"] = v.numpy()
    save("pose_random_view.npz", views)


if __name__ == "__main__":
    main()
