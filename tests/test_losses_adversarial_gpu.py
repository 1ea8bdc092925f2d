"""The loss kernels (csrc/losses.hip) on the GPU against the float64 restatement tests/losses_ref.py, on the cases of
losses_ref.CASES: ops.reconstruction_losses (``_ReconLosses.apply`` with dt1 = None for the cases without dt1) and ops.flow_loss --
the five per-frame columns, the eroded common mask, the per-pair flow loss and the gradients to the shaded image, the features and
the flow, for every case.  ops.flow_loss gets the reference's mask of the same case (the kernel's own is asserted equal to it).

Tolerance.  Errors are in units of 2^-24 x magnitude (losses_ref).  losses_ref.MEASURED holds what the float32 evaluation of the
restatement reaches per case and quantity (measured and asserted on the CPU by tests/test_losses_cpu.py); a kernel gets 4 x that
many units plus 4 ulp of the float64 value, and nothing else.  No element and no frame is left out.  The integer results -- the mask,
dropped pairs, gradients off the mask, on a sequence's last frame and where rgb equals its target -- are exact.
tests/test_losses_cpu.py::test_bounds_catch_a_wrong_piece shows the bounds bite.

Which case reaches which path of losses.hip:
  scalar feature branch (D % 4 != 0)               d1, d3, d5, hw_1x1_b3, hw_1x7_b3, hw_257x1_n1, hw_1x257_b3, hw_17x33_b3, no_dt1_sum
  wave-cooperative, D / 4 not a power of two       d12, d20 (3, 5), d260 (65 > 64), hw_3x85_n1 (3), hw_200x3_n1 (5), d12_offset1
  wave-cooperative, float4 form                    d4, d8, d16_contig, hw_16x16_n1, hw_130x130_n1, ...
  non-VEC because of the stride (17 channels)      d16_wide17, flow_b3_f4
  non-VEC because of a misaligned base pointer     d16_offset1, d12_offset1
  no features                                      d_none, hw_2x300_b3, rgb_ties, rgb_wide, flow_b1_f2, flow_b3_f2_stride3, flow_b3_f4_sum
  dt1 == nullptr                                   no_dt1, no_dt1_sum
  frames smaller than one work-group               hw_1x1_*, hw_1x7_*, hw_9x1_*, hw_3x85_* (255 pixels)
  H W = 255, 256, 257                              hw_3x85_*, hw_16x16_*, hw_257x1_* and hw_1x257_*
  W = 1 / H = 1                                    hw_1x1_*, hw_9x1_*, hw_257x1_* / hw_1x1_*, hw_1x7_*, hw_1x257_*
  W > 256 (a work-group inside one row)            hw_2x300_*, hw_4x300_n3 (with an interior)
  one work-group over many rows                    hw_200x3_* (86 rows)
  more than 64 work-groups (second trip, finish)   hw_130x130_* (67; _b3 for fl_finish_kernel)
  F = 2 / F > 2 with B > 1                         *_b3, flow_b3_f2_stride3 / flow_b3_f4, flow_b3_f4_sum
  empty mask (max(2 count, 1)) / one mask pixel    pairs 'empty' / 'one': hw_200x3_b3, flow_b3_f2_stride3, flow_b3_f4, flow_b3_f4_sum /
                                                   hw_16x16_b3, hw_17x33_b3, flow_b1_f4_stride3, flow_b3_f4, flow_b3_f4_sum; every H < 3 or W < 3
  |flow_gt| = 0.5 exactly / the next float         pairs 'half' / 'over0', 'over1': hw_3x85_b3, hw_130x130_b3, flow_b1_f2, flow_b3_f4, ...
  a large flow off the mask only                   pairs 'offmask': hw_16x16_b3, hw_130x130_b3, flow_b1_f4_stride3, flow_b3_f2_stride3, flow_b3_f4
  pix_stride 3                                     hw_1x7_b3, hw_3x85_b3, hw_257x1_b3, hw_200x3_b3, hw_17x33_b3, flow_*_stride3
  zero / negative / tiny alpha                     alpha 'special': hw_*_b3 (most), d1, d4, d20, d16_wide17, no_dt1, hw_17x33_n1
  soft mask_gt                                     mask_098, mask_0995, hw_9x1_n1, hw_1x257_n1
  a hole across a work-group boundary / a row end  mask_hole_group_edge, hw_4x300_n3, hw_200x3_n1, hw_130x130_n1 / mask_hole_row_end,
                                                   hw_3x85_n1, hw_16x16_n1
  rgb == image_gt bit for bit                      rgb_ties, hw_16x16_n1, hw_17x33_n1
  upstream loss.sum() (expanded) / columns 0..3    up 'sum': hw_1x7_n1, hw_2x300_b3, d3, d20, rgb_wide, flow_b3_f4_sum, ... / 'cols4':
                                                   hw_9x1_b3, hw_130x130_b3, d8
"""
import functools
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import losses_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("3danimals_amd.ops")


@functools.lru_cache(maxsize=None)
def case_and_reference(name):
    """(case, float64 reference): computed once per case, shared by the tests that need it, never modified."""
    c = S.build(name)
    return c, S.reference(c)


def within(got, ref, name, key, what=""):
    got = got.detach().cpu()
    val, mag = ref[key]
    assert got.shape == val.shape and got.dtype == torch.float32, (name, key, tuple(got.shape), tuple(val.shape))
    u = S.units(got, val, mag) if bool(torch.isfinite(got).all()) else float("inf")
    print(f"{name}{what}: {key} {u:.3f} units (float32 torch {S.figure(name, key)}, bound {S.allowed_units(name, key):.3f} + 4 ulp)")
    bad = S.bad_elements(got, val, mag, name, key)
    if bad.numel():
        i = tuple(bad[0].tolist())
        pytest.fail(f"{name}{what}: {key} outside the bound at {bad.shape[0]} elements, e.g. {i}: got {float(got[i])!r}, ref {float(val[i])!r}, "
                    f"magnitude {float(mag[i])!r} ({u:.2f} units)")


def run(c, ref, ops, dev):
    """Case ``c`` through ops.reconstruction_losses (or _ReconLosses.apply without dt1) and ops.flow_loss, in the layouts the case
    names: key -> tensor on the device; 'mask' is the kernel's own uint8 mask [N,H,W]."""
    N, H, W, D = c["N"], c["H"], c["W"], c["D"]
    d = lambda k: c[k].to(dev)
    shaded = d("shaded").requires_grad_(True)
    feat = None
    if D:
        if c["layout"] == "wide17":
            feat = torch.cat([d("feat"), torch.full((N, H, W, 1), 0.5, device=dev)], -1).requires_grad_(True)[..., :D]
        elif c["layout"] == "offset1":
            store = torch.cat([torch.zeros(1, device=dev), d("feat").reshape(-1)]).requires_grad_(True)
            feat = store[1:].view(N, H, W, D)
            assert feat.data_ptr() % 16 == 4 and feat.is_contiguous()
        else:
            feat = d("feat").requires_grad_(True)
    if c["dt1"]:
        loss, both = ops.reconstruction_losses(shaded.permute(0, 3, 1, 2), None if feat is None else feat.permute(0, 3, 1, 2), d("image_gt"),
                                               d("feat_gt") if D else None, d("mask_gt"), d("mask_dt"), d("valid"), return_mask=True)
    else:
        loss, both = ops._ReconLosses.apply(shaded, feat, d("image_gt"), d("feat_gt") if D else None, d("mask_gt"), d("mask_dt")[:, 0], None, d("valid"))
    res = dict(loss=loss, mask=both.view(N, H, W))
    up, w = c["up"], d("w_loss")
    total = loss.sum() if up == "sum" else ((loss[:, :4] * w[:, :4]).sum() if up == "cols4" else (loss * w).sum())
    leaves = [shaded] + ([feat] if D else [])
    if c["F"] > 1:
        if c["fstride"] == 3:
            flow = torch.cat([d("flow"), torch.ones(N, H, W, 1, device=dev)], -1).requires_grad_(True)[..., :2]
        else:
            flow = d("flow").requires_grad_(True)
        fl = ops.flow_loss(flow.permute(0, 3, 1, 2), d("flow_gt"), ref["mask"].to(dev).reshape(-1), c["B"], c["F"])
        total = total + (fl.sum() if up == "sum" else (fl * d("w_flow")).sum())
        leaves.append(flow)
        res["flow"] = fl
    g = torch.autograd.grad(total, leaves)
    res.update(g_rgb=g[0][..., :3], g_alpha=g[0][..., 3])
    if D:
        assert g[1].shape == (N, H, W, D)
        res["g_feat"] = g[1]  # (17-channel layout: a [..., :D] view, the alpha slot behind it is not written and not compared)
    if c["F"] > 1:
        res["g_flow"] = g[-1]
    return res


@pytest.mark.parametrize("name", list(S.CASES))
def test_losses_against_float64(name, ops, dev):
    """Every case: the integer results exactly, the float results within the bound (module docstring)."""
    c, ref = case_and_reference(name)
    got = run(c, ref, ops, dev)
    mask = ref["mask"]
    assert got["mask"].dtype == torch.uint8 and torch.equal(got["mask"].cpu(), mask), (name, int((got["mask"].cpu() != mask).sum()))
    for k in S.keys_of(c):
        within(got[k], ref, name, k)
    off = mask == 0
    g_rgb = got["g_rgb"].cpu()
    assert bool((g_rgb[off] == 0).all()), name
    ties = (c["shaded"][..., :3] == c["image_gt"].permute(0, 2, 3, 1))
    assert bool((g_rgb[ties] == 0).all()), name
    if c["D"]:
        assert bool((got["g_feat"].cpu()[off] == 0).all()), name
    if not c["dt1"]:
        assert bool((got["loss"][:, 4] == 0).all()), name
    if c["F"] > 1:
        B, Fr = c["B"], c["F"]
        g_flow = got["g_flow"].cpu()
        assert bool((g_flow[off] == 0).all()) and bool((g_flow.view(B, Fr, -1)[:, -1] == 0).all()), name
        dropped = ref["dropped"]
        assert bool((got["flow"].cpu()[dropped] == 0).all()) and bool((g_flow.view(B, Fr, -1)[:, :-1][dropped] == 0).all()), name


@pytest.mark.parametrize("name", ["d5", "d16_contig", "d12", "d16_wide17", "d16_offset1", "d_none", "no_dt1", "hw_130x130_b3", "flow_b3_f4",
                                  "flow_b1_f4_stride3"])
def test_two_runs_are_bit_identical(name, ops, dev):
    """Forward and backward twice, one case per kernel branch (scalar features, float4 form, D / 4 = 3, 17-channel stride, misaligned
    base, no features, no dt1, 67 work-groups through both finish kernels, flow with stride 2 and 3): every sum is reduced in a fixed
    order, so every output is bit-identical."""
    c, ref = case_and_reference(name)
    a, b = run(c, ref, ops, dev), run(c, ref, ops, dev)
    for k in ("mask",) + S.keys_of(c):
        assert torch.equal(a[k], b[k]), (name, k)
