"""The distance transform on the GPU (csrc/edt.hip through ops.distance_transform, model.dataset.util.compute_distance_transform and
pipeline._distance_transforms) against the restatement of tests/edt_ref.py: everything is compared with torch.equal -- the squared
distances are integers, the distances one float64 root, one float64 divide and one rounding of them."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_cases as C  # noqa: E402
import edt_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = (1.0, 256.0, 300.0)
KINDS = [(name, False) for name in C.ALL_CASES] + [(name, True) for name in C.U8_CASES]


def _ops():
    return importlib.import_module("3danimals_amd.ops")


def _src(name, float_kind):
    case = C.as_float(name) if float_kind else C.make_case(name)
    return torch.from_numpy(case["src"]).cuda(), case["thresholds"]


@pytest.mark.parametrize("name,float_kind", KINDS, ids=[f"{n}-{'f32' if f else 'src'}" for n, f in KINDS])
def test_squared_distances_distances_and_indices_equal_the_reference(name, float_kind):
    ops = _ops()
    src, thresholds = _src(name, float_kind)
    zero = C.zeros(name, float_kind)
    want_d2, want_idx = C.expected(name, float_kind)
    d2, idx = ops.distance_transform(src, squared=True, return_indices=True, thresholds=thresholds)
    assert d2.dtype == idx.dtype == torch.int32 and d2.shape == idx.shape == zero.shape and not d2.requires_grad
    wrong = int((d2.cpu() != torch.from_numpy(want_d2)).sum())
    print(f"{name} float_kind={float_kind}: {wrong} of {want_d2.size} squared distances differ")
    assert torch.equal(d2.cpu(), torch.from_numpy(want_d2).int())
    assert torch.equal(ops.distance_transform(src, squared=True, thresholds=thresholds), d2)  # the instance without idx
    if want_idx is not None:
        assert torch.equal(idx.cpu(), torch.from_numpy(want_idx).int())
    else:
        images = zero.reshape(-1, *zero.shape[-2:])
        for img, a, b in zip(images, d2.cpu().numpy().astype(np.int64).reshape(images.shape), idx.cpu().numpy().astype(np.int64).reshape(images.shape)):
            assert R.idx_is_a_nearest_zero(img, a, b)
    for scale in SCALES:
        dist, idx2 = ops.distance_transform(src, scale=scale, return_indices=True, thresholds=thresholds)
        want = torch.from_numpy(R.dist_from_d2(want_d2, scale))
        assert dist.dtype == torch.float32 and not dist.requires_grad
        off = int((dist.cpu() != want).sum())
        print(f"  scale {scale}: {off} of {want.numel()} distances differ")
        assert torch.equal(dist.cpu(), want) and torch.equal(idx2, idx)
        assert torch.equal(ops.distance_transform(src, scale=scale, thresholds=thresholds), dist)


def test_an_image_without_a_zero_pixel_is_finite_and_leaves_its_neighbour_alone():
    ops = _ops()
    src, _ = _src("no_zero_first_33x70", False)
    d2, idx = ops.distance_transform(src, squared=True, return_indices=True)
    none = 33 * 33 + 70 * 70
    assert bool((d2[0] == none).all()) and bool((idx[0] == -1).all())
    dist = ops.distance_transform(src, scale=70.0)
    assert torch.equal(dist[0].cpu(), torch.full((33, 70), np.float32(np.sqrt(np.float64(none)) / 70.0))) and bool(torch.isfinite(dist).all())
    alone_d2, alone_idx = ops.distance_transform(src[1:], squared=True, return_indices=True)
    assert torch.equal(alone_d2[0], d2[1]) and torch.equal(alone_idx[0], idx[1]) and int(d2[1].max()) < none
    # a bool source is the uint8 source
    assert torch.equal(ops.distance_transform(src != 0, squared=True), d2)


def test_two_runs_give_the_same_bits():
    ops = _ops()
    for name, float_kind in (("fills_255x257", False), ("fractional_nan_65x63", False), ("fills_3x300", True)):
        src, thresholds = _src(name, float_kind)
        a = ops.distance_transform(src, scale=300.0, return_indices=True, thresholds=thresholds)
        b = ops.distance_transform(src, scale=300.0, return_indices=True, thresholds=thresholds)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", ("fractional_nan_65x63", "fractional_half_33x70"))
def test_float_kind_is_laid_out_as_two_uint8_calls(name):
    ops = _ops()
    src, (t_in, t_out) = _src(name, False)
    both = ops.distance_transform(src, squared=True, return_indices=True, thresholds=(t_in, t_out))
    inside = ops.distance_transform(src >= t_in, squared=True, return_indices=True)  # (a NaN compares False: a zero pixel of both)
    outside = ops.distance_transform((src <= t_out).to(torch.uint8) * 255, squared=True, return_indices=True)
    n, h, w = src.shape
    assert both[0].shape == (n, 2, h, w) and both[0].is_contiguous()
    for k in range(2):
        assert torch.equal(both[k][:, 0], inside[k]) and torch.equal(both[k][:, 1], outside[k])


def test_refusals_through_the_abi_leave_the_outputs_untouched():
    L = importlib.import_module("3danimals_amd._lib")
    lib = L.lib()
    M, H, W = 2, 5, 7
    src = torch.zeros(M, H, W, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(lib.a3d_edt_scratch_bytes(M, H, W), dtype=torch.uint8, device="cuda")
    dist = torch.full((M, H, W), -7.0, device="cuda")
    d2 = torch.full((M, H, W), -7, dtype=torch.int32, device="cuda")
    idx = torch.full((M, H, W), -7, dtype=torch.int32, device="cuda")
    good = dict(src=src.data_ptr(), kind=L.EDT_SRC_U8, t_in=1.0, t_out=0.0, M=M, H=H, W=W, scale=1.0, scratch=scratch.data_ptr(), dist=dist.data_ptr(),
                d2=d2.data_ptr(), idx=idx.data_ptr())
    for bad in (dict(M=0), dict(H=0), dict(W=0), dict(H=4097), dict(W=4097), dict(dist=None, d2=None, idx=None), dict(src=None), dict(scale=0.0),
                dict(scale=-2.0), dict(scratch=None), dict(kind=7)):
        assert lib.a3d_edt_fwd(*dict(good, **bad).values(), L.stream()) == -1, bad
        msg = lib.a3d_last_error().decode()
        assert "a3d_edt_fwd" in msg and "invalid argument" in msg, (bad, msg)
    torch.cuda.synchronize()
    assert bool((dist == -7.0).all()) and bool((d2 == -7).all()) and bool((idx == -7).all())
    assert lib.a3d_edt_fwd(*good.values(), L.stream()) == 0  # (the list the refused ones differ from by one argument is accepted)
    torch.cuda.synchronize()
    assert bool((dist == 0).all()) and bool((d2 == 0).all()) and torch.equal(idx[0].cpu(), torch.arange(H * W, dtype=torch.int32).reshape(H, W))
    with pytest.raises(L.A3DError, match="a3d_edt_fwd"):
        L.call("a3d_edt_fwd", *dict(good, scale=0.0).values(), L.stream())


def test_compute_distance_transform_has_the_reference_channel_order():
    util = importlib.import_module("3danimals_amd.model.dataset.util")
    disc = C.make_case("disc_64x64")["src"][0].astype(np.float32)  # a {0,1} silhouette
    other = (C.make_case("fills_64x64")["src"][C.FILLS.index("random_0.5")] != 0).astype(np.float32)
    mask = torch.from_numpy(np.stack([disc, other])[:, None]).cuda()
    mask = torch.cat([mask, torch.rand_like(mask)], dim=1)  # channel 0 is used; this view is not contiguous
    got = util.compute_distance_transform(mask[:, :2])
    assert got.shape == (2, 2, 64, 64) and got.dtype == torch.float32 and got.device == mask.device and not got.requires_grad
    for b, m in enumerate((disc, other)):
        inside = R.dist_from_d2(R.brute(m == 0)[0])  # cv2.distanceTransform(np.uint8(m)): zero pixels are the background
        outside = R.dist_from_d2(R.brute(m != 0)[0])  # ... of np.uint8(1 - m): zero pixels are the mask
        assert torch.equal(got[b, 0].cpu(), torch.from_numpy(inside)) and torch.equal(got[b, 1].cpu(), torch.from_numpy(outside))
    assert float(got[0, 0, 30, 33]) > 15.0 and float(got[0, 1, 30, 33]) == 0.0  # deep inside the disc


@pytest.mark.parametrize("shape", ((2, 256, 256), (2, 96, 80)))
def test_pipeline_distance_transforms_on_the_gpu_equal_the_scipy_path(shape):
    pipeline = importlib.import_module("3danimals_amd.pipeline")
    n, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    mask = np.stack([((yy - 0.45 * h) ** 2 + (xx - 0.55 * w) ** 2 <= (0.3 * min(h, w)) ** 2),
                     ((yy - 0.6 * h) ** 2 / 4 + (xx - 0.4 * w) ** 2 <= (0.2 * min(h, w)) ** 2)]).astype(np.float32)
    mask = torch.from_numpy(mask)
    assert 0 < float(mask[0].mean()) < 1 and 0 < float(mask[1].mean()) < 1  # both classes in every image
    want = pipeline._distance_transforms(mask)
    got = pipeline._distance_transforms(mask.cuda())
    assert got.is_cuda and got.shape == (n, 2, h, w) and got.dtype == torch.float32
    print(f"{shape}: {int((got.cpu() != want).sum())} of {want.numel()} values differ from the scipy path")
    assert torch.equal(got.cpu(), want)
    assert float(want[0, 1].max()) > 0 and float(want[0, 0, 0, 0]) > 0  # channel 0: outside, distance to the mask; channel 1: inside
