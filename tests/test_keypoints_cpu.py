"""Keypoint-transfer evaluation without a GPU: the entry points of include/a3d_eval.h, argument validation before any launch, the restatement (tests/keypoints_ref.py) against what was recorded of the
reference (tests/golden/keypoints.npz, tests/golden/make_golden_keypoints.py), and the CPU side of 3danimals_amd/evaluation.py."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check as A  # noqa: E402
import keypoints_cases as C  # noqa: E402
import keypoints_ref as R  # noqa: E402

ENTRIES = ("a3d_vertex_visibility_fwd", "a3d_nearest_visible_vertex_scratch_bytes", "a3d_nearest_visible_vertex_slab", "a3d_nearest_visible_vertex_fwd")
FAKE = 0x1000  # non-NULL, 16-byte aligned, never dereferenced


def _L():
    return importlib.import_module("3danimals_amd._lib")


def _E():
    return importlib.import_module("3danimals_amd.evaluation")


@pytest.fixture(scope="module")
def G():
    return golden("keypoints.npz")


def test_tenth_header_matches_the_tenth_table_and_the_other_surfaces_are_untouched():
    """What is this surface's own (tests/test_abi_cpu.py holds every surface's table and constants to its header)."""
    protos = A.prototypes("a3d_eval.h")
    assert set(protos) == set(ENTRIES)
    assert len(protos["a3d_vertex_visibility_fwd"][1]) == 10 and len(protos["a3d_nearest_visible_vertex_fwd"][1]) == 9
    text = open(os.path.join(A.INCLUDE, "a3d_eval.h")).read()
    assert "visualize_results.py:238-246" in text and "evaluate.py:461-472" in text  # the reference lines are cited
    overlay = importlib.import_module("3danimals_amd.overlay")
    assert not any("evaluation" in m for m in overlay.MODULES)
    pkg = importlib.import_module("3danimals_amd")
    assert "evaluation" in pkg.__all__ and pkg.evaluation is _E()


def test_entry_points_refuse_invalid_arguments_before_anything_is_launched():
    """None of the pointers below is ever dereferenced and nothing is launched (this runs without a GPU)."""
    lib = _L().lib()

    def refused(fn, good, **bad):
        assert getattr(lib, fn)(*dict(good, **bad).values(), None) == -1, bad
        msg = lib.a3d_last_error().decode()
        assert "invalid argument" in msg and fn in msg, (bad, msg)

    vis = dict(rast=FAKE, tri=FAKE, B=2, H=5, W=7, F=4, V=6, vis=FAKE, ok=FAKE)
    for key in ("B", "H", "W", "F", "V"):
        refused("a3d_vertex_visibility_fwd", vis, **{key: 0})
        refused("a3d_vertex_visibility_fwd", vis, **{key: -3})
    for key in ("rast", "tri", "vis", "ok"):
        refused("a3d_vertex_visibility_fwd", vis, **{key: None})
    refused("a3d_vertex_visibility_fwd", vis, rast=FAKE + 4)
    refused("a3d_vertex_visibility_fwd", vis, B=2048, H=1024, W=1024)  # B * H * W = 2^31
    refused("a3d_vertex_visibility_fwd", vis, B=1 << 16, V=1 << 15)  # B * V = 2^31

    nvv = dict(uv=FAKE, vis=FAKE, kp=FAKE, N=3, V=65, K=16, keys=FAKE, idx=FAKE)
    for key in ("N", "V", "K"):
        refused("a3d_nearest_visible_vertex_fwd", nvv, **{key: 0})
        refused("a3d_nearest_visible_vertex_fwd", nvv, **{key: -1})
    for key in ("uv", "vis", "kp", "keys", "idx"):
        refused("a3d_nearest_visible_vertex_fwd", nvv, **{key: None})
    refused("a3d_nearest_visible_vertex_fwd", nvv, uv=FAKE + 4)
    refused("a3d_nearest_visible_vertex_fwd", nvv, keys=FAKE + 4)
    refused("a3d_nearest_visible_vertex_fwd", nvv, N=1 << 16, V=1 << 15)
    refused("a3d_nearest_visible_vertex_fwd", nvv, N=1 << 16, K=1 << 15)
    refused("a3d_nearest_visible_vertex_fwd", nvv, N=1, V=(1 << 30) + 1)
    assert lib.a3d_nearest_visible_vertex_scratch_bytes(3, 17) == 3 * 17 * 8
    for sizes in ((0, 16), (3, 0), (-1, 16), (1 << 16, 1 << 15)):
        assert lib.a3d_nearest_visible_vertex_scratch_bytes(*sizes) == 0, sizes


def test_slab_sizes_fill_the_chip_for_one_image_and_for_thousands():
    L = _L()
    lib = L.lib()
    for v in C.VS:
        assert lib.a3d_nearest_visible_vertex_slab(C.N, v) == C.SLAB == L.NVV_THREADS  # what the cases of the GPU test are built around
    assert -(-5000 // C.SLAB) == 20
    for n, v, _, trips in C.TRIPS.values():  # the cases whose threads make more than one trip over their slab
        assert lib.a3d_nearest_visible_vertex_slab(n, v) == L.NVV_THREADS * trips and trips > 1
    assert max(t[3] for t in C.TRIPS.values()) == L.NVV_MAX_TRIPS
    for n, v in ((1, 6000), (1, 24000), (1, 300000), (256, 6000), (256, 24000), (2048, 24000), (4000, 300000)):
        slab = lib.a3d_nearest_visible_vertex_slab(n, v)
        groups = n * -(-v // slab)
        assert slab % L.NVV_THREADS == 0 and L.NVV_THREADS <= slab <= L.NVV_THREADS * L.NVV_MAX_TRIPS
        assert groups >= min(1024, -(-n * v // L.NVV_THREADS) // 2), (n, v, slab, groups)  # at least half the chip's 2048 slots, or all the work there is
    assert lib.a3d_nearest_visible_vertex_slab(0, 5) == 0 and lib.a3d_nearest_visible_vertex_slab(5, 0) == 0


@pytest.mark.parametrize("name", C.FINITE)
def test_restatement_equals_the_reference_on_every_finite_case(name, G):
    case = C.make_case(name)
    got = R.nearest_visible_vertex(case["uv"], case["vis"], case["kp"])
    assert np.array_equal(got, G[f"{name}_idx"])  # (for random_*: the float32 rule and the float64 reference agree for these seeds)
    ours = _E()._nearest_visible_vertex_torch(*(torch.from_numpy(case[k]) for k in ("uv", "vis", "kp")))
    assert ours.dtype == torch.int64 and np.array_equal(ours.numpy(), got)


def test_the_cases_are_what_they_say(G):
    for name in C.LATTICE:
        case = C.make_case(name)
        step = 1024 if name.startswith("lattice") else 8
        for key in ("uv", "kp"):
            assert np.array_equal(case[key] * step, np.rint(case[key] * step)) and np.abs(case[key]).max() <= 2
        assert tuple(case["uv"].shape) == (C.N, int(name.split("_")[1][1:]), 2) and case["kp"].shape[1] == int(name.split("_")[2][1:])
    # ties: the coarse cases have vertices at equal distance from a keypoint, and the recorded answer is the lowest index among them
    case, idx = C.make_case("coarse_V5000_K16"), G["coarse_V5000_K16_idx"]
    tied = 0
    for n in range(C.N):
        src = case["uv"][n].astype(np.float64)
        src[case["vis"][n] == 0] = np.inf
        d2 = ((src[None] - case["kp"][n][:, None].astype(np.float64)) ** 2).sum(-1)
        equal = d2 == d2.min(1, keepdims=True)
        tied += int((equal.sum(1) > 1).sum())
        assert np.array_equal(equal.argmax(1), idx[n])
    assert tied >= 20
    d = C.make_case("duplicates_across_slabs")
    idx = G["duplicates_across_slabs_idx"]
    j = np.arange(16)
    assert np.array_equal(idx[0], 10 + j) and np.array_equal(idx[1], 300 + 3 * j) and np.array_equal(idx[2], 10 + j + (1 + j) * C.SLAB)
    assert (idx[2] // C.SLAB != idx[0] // C.SLAB).all() and np.array_equal(d["uv"][0, idx[2]], d["uv"][0, idx[0]])
    assert (G["only_last_visible_idx"] == 4999).all()
    assert (G["none_visible_idx"][[0, 2]] == 0).all() and (G["none_visible_idx"][1] == 4000).all()
    inv = C.make_case("invisible_is_nearest")
    assert (G["invisible_is_nearest_idx"] != 7 + 300 * j).all() and (inv["vis"][0, G["invisible_is_nearest_idx"][0]] == 1).all()


def test_nan_and_inf_rules_of_the_restatement():
    c = C.make_case("nan_keypoint")
    got = R.nearest_visible_vertex(c["uv"], c["vis"], c["kp"])
    assert got[0, 3] == 0 and got[1, 5] == 0 and (got[2] == 0).all() and (got[0, :3] > 0).all() and c["vis"][0, 0] == 0
    c = C.make_case("nan_vertex")
    got = R.nearest_visible_vertex(c["uv"], c["vis"], c["kp"])
    assert (got[0] == 4321).all() and (got[1] != 100).all() and (got[2] == 255).all()
    c = C.make_case("inf_coordinates")
    got = R.nearest_visible_vertex(c["uv"], c["vis"], c["kp"])
    assert (got[0] != 17).all() and (got[0] != 18).all() and got[1, 2] == 0 and got[2, 4] == 2000  # (kp = inf: the invisible vertex 0 is inf - inf, a NaN)
    for name in C.SPECIAL_NONFINITE:
        c = C.make_case(name)
        ours = _E()._nearest_visible_vertex_torch(*(torch.from_numpy(c[k]) for k in ("uv", "vis", "kp")))
        assert np.array_equal(ours.numpy(), R.nearest_visible_vertex(c["uv"], c["vis"], c["kp"])), name


def test_visibility_restatement_on_a_hand_made_raster():
    tri = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [1, 3, 5]])
    rast = np.zeros((2, 3, 4, 4), np.float32)
    rast[0, 1, 1, 3] = 2
    rast[0, 2, 3, 3] = 2
    rast[0, 0, 0, 3] = 4
    rast[1, 2, 2, 3] = 1
    rast[..., 0] = 0.25  # (the other channels are not read)
    got = R.visibility(rast, tri, 8)
    assert got.dtype == np.float32 and np.array_equal(got, np.array([[0, 1, 1, 1, 1, 1, 0, 0], [1, 1, 1, 0, 0, 0, 0, 0]], np.float32))


def test_pair_stage_restatement_and_the_module_equal_the_reference(G):
    c = C.make_pck_case()
    assert c["pairs"].shape == (C.PCK_P, 2) and (c["pairs"][:, 0] == c["pairs"][:, 1]).any() and len(G["pck_sources"]) == C.PCK_N
    idx = R.nearest_visible_vertex(c["uv"], c["vis"], c["kp"])
    assert np.array_equal(idx, G["pck_vert_idx"])
    for pad, tag in ((0.0, ""), (C.PCK_PAD, "_pad")):
        ours = R.pair_stage(c["uv"], idx, c["kp"], c["kp_visible"], c["boxes"], c["pairs"], 0.1, pad)
        np.testing.assert_allclose(ours["err"], G[f"pck{tag}_err"], rtol=1e-12, atol=0)
        assert ours["pck"] == float(G[f"pck{tag}_value"])
        if not tag:
            np.testing.assert_allclose(ours["pred_image"], G["pck_pred_image"], rtol=1e-12, atol=0)
            assert np.array_equal(ours["visible"], G["pck_visible"]) and np.array_equal(ours["count"], G["pck_count"]) and np.array_equal(ours["correct"], G["pck_correct"])
        # the module on CPU tensors: the same float32 rule in torch, the pair stage in float64 torch
        t = {k: torch.from_numpy(v) for k, v in c.items()}
        pck, err, visible, vert_idx = _E().keypoint_transfer_pck(t["uv"], t["vis"], t["kp"], t["kp_visible"], t["boxes"], t["pairs"], box_pad_frac=pad)
        assert isinstance(pck, float) and err.dtype == visible.dtype == torch.float64 and err.shape == visible.shape == (C.PCK_P, C.PCK_K)
        assert vert_idx.dtype == torch.int64 and np.array_equal(vert_idx.numpy(), G["pck_vert_idx"])
        np.testing.assert_allclose(err.numpy(), G[f"pck{tag}_err"], rtol=1e-12, atol=0)
        assert np.array_equal(visible.numpy(), G["pck_visible"]) and pck == float(G[f"pck{tag}_value"])
        assert np.array_equal(visible.sum(0).numpy(), G["pck_count"])
        if not tag:  # (recorded for the default pad only)
            assert np.array_equal(((err < 0.1) * visible).sum(0).numpy(), G["pck_correct"])
    assert 0.3 < float(G["pck_value"]) < 0.9 and G["pck_count"].min() > 0


def test_crop_uncrop_and_compute_pck_are_the_reference_statements(G):
    E = _E()
    c = C.make_pck_case()
    boxes = torch.from_numpy(c["boxes"])
    gt = E.uncrop_keypoints_with_box(torch.from_numpy(c["kp"]), boxes)  # batched boxes
    assert gt.dtype == torch.float64 and gt.shape == (C.PCK_N, C.PCK_K, 2)
    np.testing.assert_allclose(gt.numpy(), G["pck_gt_image"], rtol=1e-12, atol=0)
    for n in range(C.PCK_N):  # one box, as a tuple of numbers
        one = E.uncrop_keypoints_with_box(torch.from_numpy(c["kp"][n]), tuple(c["boxes"][n]))
        np.testing.assert_allclose(one.numpy(), G["pck_gt_image"][n], rtol=1e-12, atol=0)
        np.testing.assert_allclose(R.uncrop(c["kp"][n], c["boxes"][n]), G["pck_gt_image"][n], rtol=1e-12, atol=0)
        np.testing.assert_allclose(R.crop(G["pck_gt_image"][n], c["boxes"][n]), G["pck_recrop"][n], rtol=1e-12, atol=1e-15)
    back = E.crop_keypoints_with_box(torch.from_numpy(G["pck_gt_image"]), boxes)
    np.testing.assert_allclose(back.numpy(), G["pck_recrop"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(back.numpy(), c["kp"], rtol=0, atol=1e-14)
    pck = E.compute_pck(torch.from_numpy(G["pck_err"]), torch.from_numpy(G["pck_visible"]), 0.1)
    assert pck.dim() == 0 and pck.dtype == torch.float64
    # (sixteen shares in [0, 1] summed in torch's order instead of numpy's: each of the 15 additions rounds by at most 2^-53 of a partial sum <= 16)
    assert abs(float(pck) - float(G["pck_value"])) <= 15 * 16 * 2.0 ** -53 / 16
    shares = E._pck_per_keypoint(torch.from_numpy(G["pck_err"]), torch.from_numpy(G["pck_visible"]), 0.1)
    assert np.array_equal(shares.numpy(), G["pck_correct"] / G["pck_count"]) and float(shares.numpy().mean()) == float(G["pck_value"])


def test_a_keypoint_that_is_never_visible_gives_a_nan_pck():
    E = _E()
    c = {k: torch.from_numpy(v) for k, v in C.make_pck_case().items()}
    c["kp_visible"][:, 5] = 0
    pck, err, visible, _ = E.keypoint_transfer_pck(c["uv"], c["vis"], c["kp"], c["kp_visible"], c["boxes"], c["pairs"])
    assert np.isnan(pck) and bool((visible[:, 5] == 0).all()) and bool(torch.isfinite(err).all())
    assert np.isnan(float(E.compute_pck(err, visible, 0.1))) and np.isnan(R.pck(err.numpy(), visible.numpy(), 0.1))


def test_transfer_keypoints_has_the_reference_shapes_and_does_not_touch_its_arguments(G):
    E = _E()
    c = C.make_case("lattice_V257_K16")
    uv, vis, kp = (torch.from_numpy(c[k]) for k in ("uv", "vis", "kp"))
    keep = uv.clone()
    pred, aux = E.transfer_keypoints(uv[0], vis[0], uv[1], kp[0])  # single
    assert torch.equal(uv, keep) and bool(torch.isfinite(uv).all())  # (the reference overwrites the invisible rows with inf)
    assert pred.shape == (16, 2) and pred.dtype == uv.dtype and set(aux) == {"vert_idx"} and aux["vert_idx"].shape == (16,)
    assert np.array_equal(aux["vert_idx"].numpy(), G["lattice_V257_K16_idx"][0]) and torch.equal(pred, uv[1][aux["vert_idx"]])
    pred_b, aux_b = E.transfer_keypoints(uv, vis, uv.flip(0), kp)  # batched
    assert pred_b.shape == (C.N, 16, 2) and np.array_equal(aux_b["vert_idx"].numpy(), G["lattice_V257_K16_idx"])
    assert torch.equal(pred_b[0], uv[2][aux_b["vert_idx"][0]])
    pred_np, _ = E.transfer_keypoints(c["uv"][0], c["vis"][0], c["uv"][1], c["kp"][0])  # numpy arrays, as the reference takes
    assert torch.equal(pred_np, pred)
    with pytest.raises(ValueError, match="transfer_keypoints"):
        E.transfer_keypoints(uv[0], vis[0, :-1], uv[1], kp[0])


def test_ops_raise_on_cpu_tensors_and_on_wrong_arguments():
    L = _L()
    ops = importlib.import_module("3danimals_amd.ops")
    rast, tri = torch.zeros(2, 5, 7, 4), torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(L.A3DError, match="vertex_visibility"):
        ops.vertex_visibility(rast, tri, 6)
    with pytest.raises(L.A3DError, match="no CPU fallback"):
        ops.nearest_visible_vertex(torch.zeros(3, 9, 2), torch.ones(3, 9), torch.zeros(3, 4, 2))
    with pytest.raises(L.A3DError, match="no CPU fallback"):
        _E().project_and_occlude(torch.zeros(2, 9, 3), tri, torch.eye(4)[None], (8, 8))
    for bad in (dict(rast=rast[0]), dict(rast=rast[..., :3]), dict(rast=rast.int()), dict(tri=tri.float()), dict(tri=tri[:, :2]), dict(num_vertices=0),
                dict(tri=tri[:0]), dict(rast=rast[:0])):
        with pytest.raises(ValueError, match="vertex_visibility"):
            ops.vertex_visibility(**dict(dict(rast=rast, tri=tri, num_vertices=6), **bad))
    good = dict(uv=torch.zeros(3, 9, 2), visibility=torch.ones(3, 9), keypoints=torch.zeros(3, 4, 2))
    for bad in (dict(uv=good["uv"][0]), dict(uv=torch.zeros(3, 9, 3)), dict(visibility=torch.ones(3, 8)), dict(keypoints=torch.zeros(2, 4, 2)),
                dict(keypoints=torch.zeros(3, 0, 2)), dict(visibility=torch.ones(3, 9, dtype=torch.int32)), dict(uv=torch.zeros(3, 9, 2, dtype=torch.int64))):
        with pytest.raises(ValueError, match="nearest_visible_vertex"):
            ops.nearest_visible_vertex(**dict(good, **bad))
