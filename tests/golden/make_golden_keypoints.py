"""Golden vectors for the keypoint-transfer evaluation, recorded by IMPORTING the reference (build container only, CPU only).

Run:  python tests/golden/make_golden_keypoints.py     (needs the reference tree make_golden.py imports; writes tests/golden/keypoints.npz)

The reference's own transfer_keypoints, compute_pck, crop_keypoints_with_box, uncrop_keypoints_with_box and
Benchmark.compute_keypoints_error (evaluation/evaluate.py) run in float64 on the finite cases of tests/keypoints_cases.py: per
nearest-vertex case the chosen indices, for the pair case every intermediate of the loop of evaluate.py:557-587.  Only data is written;
no reference source travels.  The inputs are rebuilt from tests/keypoints_cases.py.  Every case is also checked against the float32
restatement of tests/keypoints_ref.py: a seed for which the two disagree (a float32 near-tie) must not become a fixture.
"""
import importlib
import os
import sys
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import keypoints_cases as C  # noqa: E402
import keypoints_ref as R  # noqa: E402
from make_golden import import_reference  # noqa: E402


def main():
    import_reference()
    for name in ("configargparse", "cv2", "requests", "tqdm", "matplotlib", "matplotlib.pyplot"):  # whichever are absent here
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = MagicMock()
    from evaluation import evaluate as ref

    data = {}
    for name in C.FINITE:
        case = C.make_case(name)
        idx = []
        for n in range(C.N):
            verts = case["uv"][n].astype(np.float64)  # (a copy: the reference overwrites its invisible rows)
            pred, aux = ref.transfer_keypoints(verts, case["vis"][n].astype(np.float64), case["uv"][n].astype(np.float64), case["kp"][n].astype(np.float64))
            assert np.array_equal(pred, case["uv"][n].astype(np.float64)[aux["vert_idx"]])
            idx.append(aux["vert_idx"])
        idx = np.stack(idx)
        assert np.array_equal(idx, R.nearest_visible_vertex(case["uv"], case["vis"], case["kp"])), f"{name}: float32 and float64 disagree, pick another seed"
        data[f"{name}_idx"] = idx.astype(np.int32)
        print(name, idx.shape, int(idx.max()))

    c = C.make_pck_case()
    uv64, kp64 = c["uv"].astype(np.float64), c["kp"].astype(np.float64)

    class Bench(ref.Benchmark):
        def load_keypoints(self, t):
            return ref.uncrop_keypoints_with_box(kp64[t], c["boxes"][t]), c["kp_visible"][t].astype(np.float64)

        def load_box(self, t):
            return c["boxes"][t]

    for pad, tag in ((0, ""), (C.PCK_PAD, "_pad")):
        bench = Bench(box_pad_frac=pad)
        vert_idx, preds, errs, viss = {}, [], [], []
        for s, t in c["pairs"]:
            pred, aux = ref.transfer_keypoints(uv64[s].copy(), c["vis"][s].astype(np.float64), uv64[t], kp64[s])
            assert vert_idx.setdefault(int(s), aux["vert_idx"]) is aux["vert_idx"] or np.array_equal(vert_idx[int(s)], aux["vert_idx"])
            pred_image = ref.uncrop_keypoints_with_box(pred, c["boxes"][t])
            err, target_visible, gt = bench.compute_keypoints_error(t, pred_image)
            preds.append(pred_image)
            errs.append(err)
            viss.append(c["kp_visible"][s].astype(np.float64) * target_visible)
        err, vis = np.stack(errs), np.stack(viss)
        data[f"pck{tag}_err"] = err
        data[f"pck{tag}_value"] = np.float64(ref.compute_pck(err, vis, 0.1))
        if not tag:
            data["pck_pred_image"] = np.stack(preds)
            data["pck_visible"] = vis
            data["pck_count"] = vis.sum(0)
            data["pck_correct"] = ((err < 0.1) * vis).sum(0)
            ours = R.nearest_visible_vertex(c["uv"], c["vis"], c["kp"])
            for s, got in vert_idx.items():
                assert np.array_equal(got, ours[s]), "pck case: float32 and float64 disagree"
            data["pck_vert_idx"] = ours.astype(np.int32)  # (rows of images that are never a source: the float32 rule's)
            data["pck_sources"] = np.array(sorted(vert_idx), np.int32)
            gt_image = np.stack([ref.uncrop_keypoints_with_box(kp64[n], c["boxes"][n]) for n in range(C.PCK_N)])
            data["pck_gt_image"] = gt_image
            data["pck_recrop"] = np.stack([ref.crop_keypoints_with_box(gt_image[n], c["boxes"][n]) for n in range(C.PCK_N)])
        print("pck", tag, float(data[f"pck{tag}_value"]), data["pck_count"], data["pck_correct"])
    path = os.path.join(HERE, "keypoints.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
