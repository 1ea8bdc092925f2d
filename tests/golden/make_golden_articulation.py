"""Golden vectors for the articulation glue, recorded by RUNNING the reference's own functions (build container only, CPU only).

Run:  python tests/golden/make_golden_articulation.py     (needs the reference tree; writes articulation_limits.npz and
                                                            articulation_bones.npz beside this file)

The reference's predictor modules import its whole network and dataset stack, so nothing is imported: the two files are read with
``ast``, the function definitions named below are compiled on their own and called with a SimpleNamespace for ``self`` and stand-ins for
the few globals they touch (``estimate_bones`` / ``skinning`` return the case's bones, ``rearrange`` flattens the leading pair).  Only
their results are written; no reference source travels.  The inputs are rebuilt from tests/articulation_cases.py.
"""
import ast
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the package, for the cases module
import articulation_cases as C  # noqa: E402
from make_golden import REF  # noqa: E402

WANTED = {
    "InstancePredictorBase.py": ("InstancePredictorBase", ("get_bones", "get_bones_from_articulation", "apply_articulation_constraints")),
    "InstancePredictorFauna.py": ("InstancePredictorFauna", ("get_bones", "apply_articulation_constraints", "apply_fauna_articulation_regularizer")),
}


def functions_of(file_name, class_name, names, env):
    path = os.path.join(REF, "model", "predictors", file_name)
    tree = ast.parse(open(path).read(), path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == class_name)
    out = {}
    for fn in cls.body:
        if isinstance(fn, ast.FunctionDef) and fn.name in names:
            scope = dict(env)
            exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), scope)
            out[fn.name] = scope[fn.name]
    assert set(out) == set(names), (file_name, sorted(out))
    return out


def main():
    state = {}
    env = dict(torch=torch, F=F, np=np, print=lambda *a, **k: None, in_range=lambda *a: False,
               estimate_bones=lambda *a, **k: state["bones"],
               skinning=lambda verts, bones, *a, **k: (verts, {"posed_bones": state["bones"]}),
               rearrange=lambda t, pattern: t.reshape(-1, *t.shape[2:]))
    base = functions_of("InstancePredictorBase.py", *WANTED["InstancePredictorBase.py"], env)
    fauna = functions_of("InstancePredictorFauna.py", *WANTED["InstancePredictorFauna.py"], env)

    data = {}
    for name, (kind, cfg) in C.GOLDEN_LIMITS.items():
        x = C.golden_limits_x(name)
        arti = SimpleNamespace(**{k: cfg[k] for k in ("num_body_bones", "num_legs", "num_leg_bones", "output_multiplier", "max_arti_angle")},
                               static_root_bones=cfg.get("static_root_bones", False), constrain_legs=cfg.get("constrain_legs", False),
                               use_fauna_constraints=cfg.get("use_fauna_constraints", False), extra_constraints=cfg.get("extra_constraints", False))
        if kind == "base":
            out = base["apply_articulation_constraints"](SimpleNamespace(cfg_articulation=arti), x.clone())
        else:
            me = SimpleNamespace(cfg_articulation=arti, cfg_additional=SimpleNamespace(
                **{k: cfg[k] for k in ("iter_leg_rotation_start", "forbid_leg_rotate", "small_leg_angle", "reg_body_rotate_mult")}))
            a = x.clone()
            a *= arti.output_multiplier  # forward_articulation's own two statements in front of the constraints
            a = a.tanh()
            a = fauna["apply_articulation_constraints"](me, a, cfg["total_iter"])
            out = fauna["apply_fauna_articulation_regularizer"](me, a, cfg["total_iter"])
        assert out.dtype == torch.float32 and out.shape == x.shape
        data[name] = out.numpy()
        print(name, tuple(out.shape), float(out.abs().max()))
    path = os.path.join(HERE, "articulation_limits.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path))

    data = {}
    for name in C.GOLDEN_BONES:
        c = C.golden_bones_inputs(name)
        N = C.GOLDEN_N
        state["bones"] = c["bones"][:, None]  # [B|1, F = 1, K, 2, 3]
        me = SimpleNamespace(kinematic_tree_epoch=0, kinematic_tree=None, bone_aux=None, spatial_scale=C.SPATIAL_SCALE,
                             cfg_pose=SimpleNamespace(cam_pos_z_offset=C.Z_OFFSET), cfg_additional=SimpleNamespace(bone_y_threshold=None),
                             cfg_articulation=SimpleNamespace(num_body_bones=0, num_legs=0, num_leg_bones=0, body_bones_mode=None,
                                                              legs_to_body_joint_indices=None, bone_feature_mode=c["mode"],
                                                              skinning_temperature=1.0, refine_feature_mode=["dino_global", "dino_sample"]))
        verts = torch.zeros(N, 1, 4, 3)
        if c["pred"] == "refine":
            _, feat, pos = base["get_bones_from_articulation"](me, verts, c["feat"], c["patch"], c["mvp"], c["w2c"], state["bones"], torch.zeros(N, 1, C.GOLDEN_K, 3))
        else:
            _, feat, pos = (base if c["pred"] == "base" else fauna)["get_bones"](me, verts, c["feat"], c["patch"], c["mvp"], c["w2c"], N, 1, 0, 0)
        data[name + "_feat"], data[name + "_pos"] = feat.numpy(), pos.numpy()
        print(name, tuple(feat.shape), tuple(pos.shape))
    path = os.path.join(HERE, "articulation_bones.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
