"""The rasteriser forward (csrc/raster.hip: rs_box, the pooled candidates, the 8x8 tile test, rs_row_span, rs_order, rs_tri_kernel<4 / 2 / 1>,
the resolves) on the named cases of tests/raster_cases.py, against the BOX-FREE reference -- oracle/raster_ref.c's frag() at every pixel
of the frame for every triangle (raster_ref.rasterize(..., whole_frame=True)) --, bit for bit: triangle ids and (u, v, z/w), no
tolerance.  (The one per-image-clip case of 700 images compares with the boxed oracle; tests/test_raster_cases_cpu.py shows the two
oracles equal on every case, and the box-free one in agreement with the float64 statement of the definition, tests/raster_fwd_ref.py.)

Every case runs through ops.rasterize with a cleared key cache (the clear path), again (the keys re-armed by the first call's resolve),
and -- where the frame has the covered-pixel list's tile order -- through defer_resolve followed by ensure_resolved (the stand-alone
resolve).  A shared clip ([1,V,4], batch = B) must give B copies of the one reference image.  The peeled cases are peeled until the
empty layer: layer n at every pixel is the n-th fragment, in (z/w, id) order, of the box-free fragment list (a3d_ref_fragments), its
texel that of the box-free oracle's own peel.

Per case: covered pixels of the reference image (of image 0) / boxes above RS_BIG = 512 pixels / their 8x8 tiles (image 0):

    box_64                  48 x 48  F = 32   LPT = 4  covered    86  big boxes   0  tiles    0  peeled: 1 layers + the empty one
    box_65                  48 x 48  F = 32   LPT = 4  covered    87  big boxes   0  tiles    0  peeled: 1 layers + the empty one
    box_512_32x16           48 x 48  F = 32   LPT = 4  covered   546  big boxes   0  tiles    0  peeled: 2 layers + the empty one
    box_528_33x16           48 x 48  F = 32   LPT = 4  covered   562  big boxes   2  tiles   20  peeled: 2 layers + the empty one
    box_529_23x23           23 x 23  F = 32   LPT = 4  covered   529  big boxes   2  tiles   18  peeled: 2 layers + the empty one
    box_576_24x24           32 x 32  F = 32   LPT = 4  covered   589  big boxes   2  tiles   18  peeled: 2 layers + the empty one
    frame_256_full         256 x 256 F = 51   LPT = 4  covered 65536  big boxes  11  tiles 1376  peeled: 3 layers + the empty one
    faces_1                 32 x 32  F = 1    LPT = 4  covered   304  big boxes   1  tiles   16
    faces_15                32 x 32  F = 15   LPT = 4  covered    74  big boxes   0  tiles    0
    faces_16                32 x 32  F = 16   LPT = 4  covered    45  big boxes   0  tiles    0  B = 2 (shared clip)
    faces_17                32 x 32  F = 17   LPT = 4  covered    83  big boxes   0  tiles    0
    faces_63                32 x 32  F = 63   LPT = 4  covered   278  big boxes   0  tiles    0
    faces_64                32 x 32  F = 64   LPT = 4  covered   298  big boxes   0  tiles    0
    faces_65                32 x 32  F = 65   LPT = 4  covered   262  big boxes   0  tiles    0  B = 2 (shared clip)
    faces_257               32 x 32  F = 257  LPT = 4  covered   741  big boxes   0  tiles    0
    big_64_consecutive      24 x 24  F = 64   LPT = 4  covered   576  big boxes  64  tiles  576
    big_in_each_slice       32 x 32  F = 64   LPT = 4  covered   652  big boxes   4  tiles   36
    lpt_300000              16 x 16  F = 240  LPT = 4  covered   254  big boxes   0  tiles    0  B = 1250 (shared clip)
    lpt_300240              16 x 16  F = 240  LPT = 2  covered   254  big boxes   0  tiles    0  B = 1251 (shared clip)
    lpt_600000              16 x 16  F = 240  LPT = 2  covered   254  big boxes   0  tiles    0  B = 2500 (shared clip)
    lpt_600240              16 x 16  F = 240  LPT = 1  covered   254  big boxes   0  tiles    0  B = 2501 (shared clip)
    lpt1_256_big            24 x 24  F = 256  LPT = 1  covered   576  big boxes 256  tiles 2304  B = 2344 (shared clip)
    lpt2_per_image_clip     16 x 16  F = 450  LPT = 2  covered   256  big boxes   0  tiles    0  B = 700
    spiky_small             96 x 96  F = 720  LPT = 4  covered  7055  big boxes  87  tiles 3458  B = 2  peeled: 10 layers + the empty one
    slivers_far             64 x 64  F = 52   LPT = 4  covered  4096  big boxes  22  tiles 1136  peeled: 7 layers + the empty one
    signed_zero_pair        32 x 32  F = 8    LPT = 4  covered   666  big boxes   0  tiles    0  peeled: 2 layers + the empty one
    depth_order             64 x 64  F = 300  LPT = 4  covered  1535  big boxes   5  tiles   80
    bad_input               64 x 64  F = 34   LPT = 4  covered  2948  big boxes  22  tiles  692
    frame_1x40               1 x 40  F = 21   LPT = 4  covered    32  big boxes   0  tiles    0
    frame_33x1              33 x 1   F = 21   LPT = 4  covered    33  big boxes   0  tiles    0
    frame_8x32               8 x 32  F = 21   LPT = 4  covered   176  big boxes   0  tiles    0
    frame_5x3                5 x 3   F = 21   LPT = 4  covered    13  big boxes   0  tiles    0  B = 3 (shared clip)
    frame_50x70             50 x 70  F = 21   LPT = 4  covered  1995  big boxes   1  tiles   63
    frame_24x40             24 x 40  F = 21   LPT = 4  covered   569  big boxes   1  tiles   15

What showed on the MI355X (first run of this module, kernels as they were):

  * Item 5 (depth order at signed zero) SHOWED as read: signed_zero_pair came out with the higher id (the one at -0) where the reference has the lower
    one (333 pixels, the (+0, -0) pairs; in the (-0, +0) id order both sides agree), and layer 0 of its peel likewise.  rs_order now takes -0 as +0 before it
    builds the key, for the fragment and for the peel's ``prev`` key; the oracle's rule (equal depth: the lower id) stands.
  * Item 6 (rs_box with a denormal w) SHOWED: bad_input differed at 1166 of 4096 pixels -- the triangles with a vertex at x = y = 0,
    w in {1e-38, 1e-42} (0 * rcp(w) = 0 * inf = NaN, dropped by fminf / fmaxf) and at denormal x, y (+-inf where x / w is on screen)
    lost the pixels outside the hull of their other two vertices.  rs_box now takes the full frame when a projected coordinate is
    not finite.
  * Found beyond the issue's list: with that box in place 119 pixels still differed, all of triangle 18 (vertex (0.3 w, -0.2 w),
    w = 1e-42), culled by rs_row_span: 1 / A overflows for an edge coefficient A in the denormal range, the half-line's end became
    +-inf whatever the true quotient, and the relative ``tol`` of the tile test and of the span vanishes with the products.  The span
    now ignores an edge whose reciprocal is not finite, and both culls' tolerance has an absolute part (RS_TOL_ABS).  (A float32
    restatement of the two culls on the CPU loses the same 165 fragments before and none after.)
  * Items 1 - 4 and 7 did NOT show: the pixel box of both sides, the pooled reciprocal division, the tile test, the row spans, the
    multi-chunk loop, the 256-entry big-box list of rs_tri_kernel<1>, both lanes-per-triangle thresholds and every peel were
    bit-exact on the first run (41 of 44 tests passed as the kernels were; all 44 after the three changes).
  * bad_input's 'big boxes' above counts the oracle-flavour box; the kernel adds the eight triangles with a denormal w (full frame).
"""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("3danimals_amd.ops")


def _expect(name):
    c = RC.all_cases()[name]
    ref = RC.reference(name)[c["oracle"] if c["oracle"] == "boxed" else "whole"].numpy()
    return c, ref


def _same(out, ref, B, what):
    """out [B,H,W,4] (device) against ref [1|B,H,W,4]: ids first (the clearer message), then every float, then the sign of zero"""
    out = out.detach().cpu().numpy()
    assert out.shape[0] == B
    ref = np.broadcast_to(ref, out.shape)
    bad = out[..., 3] != ref[..., 3]
    if bad.any():  # (kernel id, reference id) -> pixels, the commonest first; -1 = empty
        pairs, n = np.unique(np.stack([out[..., 3][bad], ref[..., 3][bad]], 1).astype(np.int64) - 1, axis=0, return_counts=True)
        top = sorted(zip(n.tolist(), pairs.tolist()), reverse=True)[:12]
        raise AssertionError(f"{what}: ids differ at {int(bad.sum())} pixels, first (image, y, x) {[int(v[0]) for v in np.nonzero(bad)]}; "
                             f"pixels x (kernel, reference) id: {top}")
    assert np.array_equal(out, ref), what


@pytest.mark.parametrize("name", RC.NAMES)
def test_rasterize_case_bit_exact_vs_box_free_reference(name, dev, ops):
    c, ref = _expect(name)
    H, W, B = c["H"], c["W"], c["B"]
    clip_d, tri_d = c["clip"].to(dev), c["tri"].to(dev)
    ops._rast_keys.clear()
    first = ops.rasterize(clip_d, tri_d, (H, W), batch=B)   # keys cleared by the call
    second = ops.rasterize(clip_d, tri_d, (H, W), batch=B)  # keys re-armed by the first call's resolve
    assert len(ops._rast_keys) == 1
    _same(first, ref, B, (name, "clear path"))
    _same(second, ref, B, (name, "re-armed path"))
    assert np.array_equal(first.cpu().numpy(), second.cpu().numpy())
    if H % 8 == 0 and W % 8 == 0 and (H * W) % 256 == 0:
        third = ops.rasterize(clip_d, tri_d, (H, W), batch=B, defer_resolve=True)
        ops.ensure_resolved(third)
        _same(third, ref, B, (name, "defer_resolve + ensure_resolved"))
        fourth = ops.rasterize(clip_d, tri_d, (H, W), batch=B)  # ... and the keys the stand-alone resolve re-armed
        _same(fourth, ref, B, (name, "after the stand-alone resolve"))


@pytest.mark.parametrize("name", RC.PEEL_NAMES)
def test_depth_peeling_down_to_the_empty_layer(name, dev, ops):
    from oracle import raster_ref

    c = RC.all_cases()[name]
    H, W, B = c["H"], c["W"], c["clip"].shape[0]
    count, zw, ids = (t.numpy() for t in RC.peel_reference(name))
    clip_d, tri_d = c["clip"].to(dev), c["tri"].to(dev)
    depth = int(count.max())
    prev_d = prev_o = None
    ops._rast_keys.clear()
    for n in range(depth + 1):
        layer = ops.rasterize(clip_d, tri_d, (H, W), prev=prev_d)
        want = raster_ref.rasterize(c["clip"], c["tri"], (H, W), prev=prev_o, whole_frame=True)
        got = layer.cpu().numpy()
        assert np.array_equal(got[..., 3].astype(np.int64) - 1, np.where(count > n, ids[..., n], -1)), (name, n)  # the n-th fragment
        assert np.array_equal(got[..., 2], np.where(count > n, zw[..., n], 0.0)), (name, n)
        _same(layer, want.numpy(), B, (name, "layer", n))
        prev_d, prev_o = layer, want
    assert not bool((prev_d[..., 3] > 0).any())  # the last layer is empty
