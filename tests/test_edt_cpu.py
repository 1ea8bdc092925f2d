"""The distance transform without a GPU: the entry points of include/a3d_edt.h, argument validation before any launch, the brute-force restatement (tests/edt_ref.py) against scipy on every case that has a
zero pixel, its tie rule, the float64 -> float32 root the distances rest on, and the CPU side of the Python layers."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check as A  # noqa: E402
import edt_cases as C  # noqa: E402
import edt_ref as R  # noqa: E402

ENTRIES = ("a3d_edt_scratch_bytes", "a3d_edt_fwd")
FAKE = 0x1000  # non-NULL, 16-byte aligned, never dereferenced


def _L():
    return importlib.import_module("3danimals_amd._lib")


def test_eighth_header_matches_the_eighth_table_and_the_other_surfaces_are_untouched():
    """What is this surface's own (tests/test_abi_cpu.py holds every surface's table and constants to its header)."""
    protos = A.prototypes("a3d_edt.h")
    assert set(protos) == set(ENTRIES)
    fwd = protos["a3d_edt_fwd"][1]
    assert len(fwd) == 13 and fwd[1] == "int" and fwd[2] == fwd[3] == "float" and fwd[7] == "double" and protos["a3d_edt_scratch_bytes"][0] == "size_t"
    assert "model/dataset/util.py:12-18" in open(os.path.join(A.INCLUDE, "a3d_edt.h")).read()  # the reference lines are cited
    overlay = importlib.import_module("3danimals_amd.overlay")
    assert not any("dataset" in m for m in overlay.MODULES)  # the mirror of compute_distance_transform is not part of the overlay


def test_entry_points_refuse_invalid_arguments_before_anything_is_launched():
    """None of the pointers below is ever dereferenced and nothing is launched (this runs without a GPU)."""
    L = _L()
    lib = L.lib()
    good = dict(src=FAKE, kind=L.EDT_SRC_U8, t_in=1.0, t_out=0.0, M=2, H=5, W=7, scale=1.0, scratch=FAKE, dist=FAKE, d2=FAKE, idx=FAKE)

    def refused(**bad):
        args = dict(good, **bad)
        assert lib.a3d_edt_fwd(*args.values(), None) == -1, bad
        msg = lib.a3d_last_error().decode()
        assert "invalid argument" in msg and "a3d_edt_fwd" in msg, (bad, msg)

    assert lib.a3d_edt_fwd(*dict(good, src=None).values(), None) == -1  # (the one valid list differs from these by one argument each)
    for key in ("M", "H", "W"):
        refused(**{key: 0})
        refused(**{key: -2})
    refused(H=4097)
    refused(W=4097)
    refused(M=128, H=4096, W=4096)  # M * H * W = 2^31
    refused(dist=None, d2=None, idx=None)
    refused(src=None)
    refused(scratch=None)
    refused(scratch=FAKE + 1)
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        refused(scale=scale)
    refused(kind=2)
    refused(kind=-1)
    refused(kind=L.EDT_SRC_F32, M=3)  # two channels per image
    refused(kind=L.EDT_SRC_F32, src=FAKE + 2)
    assert lib.a3d_edt_scratch_bytes(2, 5, 7) == 2 * 2 * 5 * 7 + 4 and lib.a3d_edt_scratch_bytes(127, 4096, 4096) == 127 << 25
    for sizes in ((0, 5, 7), (2, 0, 7), (2, 5, 0), (1, 4097, 1), (1, 1, 4097), (128, 4096, 4096), (-1, 5, 7)):
        assert lib.a3d_edt_scratch_bytes(*sizes) == 0, sizes


@pytest.mark.parametrize("name", C.ALL_CASES)
def test_brute_force_and_scipy_agree_on_every_image_that_has_a_zero_pixel(name):
    from scipy.ndimage import distance_transform_edt

    compared = 0
    for float_kind in (False, True) if name in C.U8_CASES else (False,):
        z = C.zeros(name, float_kind)
        d2, idx = C.expected(name, float_kind)
        assert d2.shape == z.shape and (idx is None) == (z.shape[-2] * z.shape[-1] > R.BRUTE_PIXELS)
        images = z.reshape(-1, *z.shape[-2:])
        for img, want, want_idx in zip(images, d2.reshape(images.shape), [None] * len(images) if idx is None else idx.reshape(images.shape)):
            if not img.any():
                assert (want == R.none_value(*img.shape)).all() and want.min() > (img.shape[0] - 1) ** 2 + (img.shape[1] - 1) ** 2
                continue
            edt = distance_transform_edt(~img)
            assert float(np.abs(edt ** 2 - np.rint(edt ** 2)).max()) <= 3e-14 * max(1.0, float(edt.max()) ** 2)
            assert np.array_equal(np.rint(edt ** 2).astype(np.int64), want)
            assert (want[img] == 0).all() and (want[~img] > 0).all()
            if want_idx is not None:
                assert R.idx_is_a_nearest_zero(img, want, want_idx)
            compared += 1
    assert compared >= 2


def test_the_cases_are_what_they_say():
    assert [tuple(int(v) for v in n[6:].split("x")) for n in C.U8_CASES if n.startswith("fills_")] == list(C.SHAPES)
    for h, w in C.SHAPES:
        z = C.zeros(f"fills_{h}x{w}")
        count = dict(zip(C.FILLS, z.reshape(len(C.FILLS), -1).sum(1).tolist()))
        assert count["no_zero"] == 0 and count["all_zero"] == h * w and count["centre"] == 1 and count["zero_row"] == w and count["zero_column"] == h
        assert all(count[f"corner_{a}{b}"] == 1 for a in "0h" for b in "0w") and count["checkerboard"] == (h * w + 1) // 2
        assert z[C.FILLS.index("corner_hw"), h - 1, w - 1] and z[C.FILLS.index("corner_0w"), 0, w - 1] and z[C.FILLS.index("corner_h0"), h - 1, 0]
    # the longest search: 255x257, the single zero pixel in a corner
    d2, _ = C.expected("fills_255x257")
    assert int(d2[C.FILLS.index("corner_00")].max()) == C.LONGEST_D2 == 130052 == int(d2[C.FILLS.index("corner_hw")].max())
    # the batch whose first image has no zero pixel
    z = C.zeros("no_zero_first_33x70")
    assert not z[0].any() and z[1].any() and (C.expected("no_zero_first_33x70")[1][0] == -1).all()
    # the float kind of a uint8 case: channel 0 is the case, channel 1 its complement
    zf = C.zeros("disc_64x64", True)
    assert np.array_equal(zf[:, 0], C.zeros("disc_64x64")) and np.array_equal(zf[:, 1], ~zf[:, 0])
    # soft masks: a NaN is a zero pixel of both channels, a fractional value is a zero pixel of both under (1, 0), the channels overlap
    src, z = C.make_case("fractional_nan_65x63")["src"], C.zeros("fractional_nan_65x63")
    assert np.isnan(src[2, 33, 30]) and z[2, 0, 33, 30] and z[2, 1, 33, 30] and z[2, 0, 2, 3] and z[2, 1, 2, 3] and src[2, 2, 3] == 0.5
    assert (z[:, 0] & z[:, 1]).sum() > 100  # not complements
    src, z = C.make_case("fractional_half_33x70")["src"], C.zeros("fractional_half_33x70")
    assert not z[0, 0, 0, 69] and z[0, 1, 0, 69] and z[0, 0, 32, 0] and not z[0, 1, 32, 0] and z[1, 0, 5, 5] and z[1, 1, 5, 5]
    assert src[np.isfinite(src)].min() < 0 and src[np.isfinite(src)].max() > 1


def test_the_tie_rule_on_the_two_discs():
    z = C.zeros("two_discs_65x63")
    d2, idx = C.expected("two_discs_65x63")
    # image 0: mirrored about the column x = 31 -- every pixel of that column is equally near both discs and takes the LEFT one
    assert np.array_equal(z[0], z[0][:, ::-1])
    qy, qx = idx[0][:, 31] // 63, idx[0][:, 31] % 63
    assert (qx < 31).all() and z[0][qy, 2 * 31 - qx].all() and ((np.arange(65) - qy) ** 2 + (31 - qx) ** 2 == d2[0][:, 31]).all()
    # image 1: mirrored about the row y = 32 -- the UPPER one
    assert np.array_equal(z[1], z[1][::-1])
    qy, qx = idx[1][32] // 63, idx[1][32] % 63
    assert (qy < 32).all() and z[1][2 * 32 - qy, qx].all() and ((32 - qy) ** 2 + (np.arange(63) - qx) ** 2 == d2[1][32]).all()
    # and the smallest flat index among ALL equally near zero pixels, everywhere
    for img, want_d2, want_idx in zip(z, d2, idx):
        qy, qx = np.nonzero(img)
        for py, px in ((0, 0), (30, 31), (32, 28), (64, 62), (32, 31), (17, 45)):
            near = np.nonzero((py - qy) ** 2 + (px - qx) ** 2 == want_d2[py, px])[0]
            assert near.size >= 1 and want_idx[py, px] == (qy[near] * 63 + qx[near]).min()


def test_float32_of_the_float64_root_is_the_correctly_rounded_float32_root_up_to_2_to_the_24():
    n = np.arange(0, (1 << 24) + 1, dtype=np.int64)
    assert np.array_equal(np.sqrt(n.astype(np.float64)).astype(np.float32), np.sqrt(n.astype(np.float32)))
    assert np.array_equal(R.dist_from_d2(n[:4097]), np.sqrt(n[:4097].astype(np.float32)))


@pytest.mark.parametrize("name", ("fills_7x5", "fills_33x70", "disc_64x64", "two_discs_65x63"))
def test_removing_one_zero_pixel_changes_the_reference(name):
    """So an implementation that drops a candidate cannot pass: every zero pixel is the strictly nearest one of some pixel (itself)."""
    z = C.zeros(name)
    d2, _ = C.expected(name)
    rng = np.random.default_rng(5)
    for img, want in zip(z, d2):
        ys, xs = np.nonzero(img)
        if ys.size < 2:
            continue
        for k in rng.choice(ys.size, size=min(3, ys.size), replace=False):
            fewer = img.copy()
            fewer[ys[k], xs[k]] = False
            got = R.brute(fewer)[0]
            assert got[ys[k], xs[k]] > 0 and (got >= want).all() and (got != want).any()


def test_ops_and_the_mirror_raise_on_cpu_tensors():
    L = _L()
    ops = importlib.import_module("3danimals_amd.ops")
    util = importlib.import_module("3danimals_amd.model.dataset.util")
    with pytest.raises(L.A3DError, match="distance_transform"):
        ops.distance_transform(torch.zeros(2, 5, 7, dtype=torch.uint8))
    with pytest.raises(L.A3DError, match="distance_transform"):
        ops.distance_transform(torch.zeros(2, 5, 7), thresholds=(1.0, 0.0), return_indices=True)
    with pytest.raises(L.A3DError, match="no CPU fallback"):
        util.compute_distance_transform(torch.zeros(2, 1, 5, 7))
    for bad in (dict(src=torch.zeros(5, 7, dtype=torch.uint8)), dict(src=torch.zeros(2, 5, 7)), dict(src=torch.zeros(2, 5, 7, dtype=torch.uint8), thresholds=(1, 0)),
                dict(src=torch.zeros(2, 5, 7, dtype=torch.float64), thresholds=(1, 0)), dict(src=torch.zeros(2, 5, 7, dtype=torch.uint8), scale=0.0),
                dict(src=torch.zeros(2, 5, 7, dtype=torch.uint8), scale=float("nan")), dict(src=torch.zeros(1, 4097, 1, dtype=torch.uint8)),
                dict(src=torch.zeros(0, 5, 7, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="distance_transform"):
            ops.distance_transform(**bad)
    with pytest.raises(ValueError, match="compute_distance_transform"):
        util.compute_distance_transform(torch.zeros(2, 5, 7))


def test_distance_transforms_of_a_cpu_mask_are_the_scipy_statements():
    from scipy.ndimage import distance_transform_edt

    pipeline = importlib.import_module("3danimals_amd.pipeline")
    mask = torch.from_numpy(np.stack([C.make_case("disc_64x64")["src"][0], (C.make_case("fills_64x64")["src"][C.FILLS.index("random_0.5")] != 0)]).astype(np.float32))
    got = pipeline._distance_transforms(mask)
    m = mask.numpy() > 0.5
    want = np.zeros((2, 2, 64, 64), np.float32)
    for b in range(2):
        want[b, 0] = distance_transform_edt(~m[b]) / 64
        want[b, 1] = distance_transform_edt(m[b]) / 64
    assert got.dtype == torch.float32 and got.device.type == "cpu" and torch.equal(got, torch.from_numpy(want))
    # and what the GPU path is held to (tests/test_edt_gpu.py): the same values from the squared distances of the restatement
    z = np.stack([~m, m], axis=1)  # channel 0 is the transform of ~m: its zero pixels are the mask
    for b in range(2):
        for c in range(2):
            assert np.array_equal(R.dist_from_d2(R.brute(~z[b, c])[0], 64.0), want[b, c])
