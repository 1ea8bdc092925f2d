"""The image-space derivative kernels (csrc/deriv.hip: a3d_rast_db_fwd / _bwd, a3d_interp_da_fwd / _bwd) on the GPU, through
ops.rasterize_db / ops.interpolate_da and through the nvdiffrast stand-in, against the float64 restatement tests/deriv_ref.py: forward
and every gradient (g_clip, g_attr, g_rast_db) on the scenes of deriv_ref.SCENES, depth layer >= 1, a deferred-resolve raster, range
mode, an empty image, known answers, the textured-mesh chain into dr.texture, launch counts and peak memory.

Tolerance.  Errors are measured in units of 2^-24 x magnitude (deriv_ref: the expression evaluated with absolute values; per vertex the
sum over the pixels that feed it).  PARENT_UNITS holds, per quantity, what the torch fp32 path (ops._rasterize_db_torch /
ops._interpolate_da_torch and their autograd: the parent commit's implementation) reaches against the restatement over every element
of every scene of this file and both depth layers -- measured on the CPU by tests/test_deriv_cpu.py, which asserts it on every pixel.
The kernels get 4 x that (another summation order in the scatter: tile-staged against index_put) plus a floor of 4 ulp of the
float64 value; no pixel is excluded.  tests/test_deriv_cpu.py::test_bounds_catch_one_dropped_pixel shows the bounds bite.
"""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deriv_ref as R  # noqa: E402
import texture_ref as T  # noqa: E402

# measured maxima of the torch fp32 path over SCENES x depth layers {0, 1} and the range-mode, empty and chain scenes, every element
# (units of 2^-24 x magnitude; CPU, one thread; tests/test_deriv_cpu.py prints them per scene and asserts them): db 2.76629 (b3_odd_c3_subset),
# g_clip 0.1666 (b1_tall_c1, layer 1), da 2.67221, g_rast_db 2.51184 (b16_shared_c8_permuted), g_attr 1.85203 (the same, layer 1) -- the
# measured figures, written with three decimals (the third rounded up so that the CPU assertion on the measurement itself holds).
# (g_clip's magnitude sums |term| through 1 / s^3 per vertex and is far above what either implementation errs by: hence the small figure.)
# Kernel bound per element: 2^-24 (4 x PARENT_UNITS x magnitude + 4 |float64 value|).
PARENT_UNITS = dict(db=2.767, g_clip=0.167, da=2.673, g_attr=1.853, g_rast_db=2.512)

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("3danimals_amd.ops")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("3danimals_amd._lib")


@pytest.fixture(scope="module")
def dr():
    sys.path.insert(0, os.path.join(ROOT, "3danimals_amd", "shims"))
    return importlib.import_module("nvdiffrast.torch")


def _assert_within(got, ref, mag, key, what):
    got = got.detach().cpu()
    u = R.units(got, ref, mag) if bool(torch.isfinite(got).all()) else float("inf")
    print(f"{what}: {key} {u:.3f} units (torch fp32 path <= {PARENT_UNITS[key]}, bound {4 * PARENT_UNITS[key]} + 4 ulp)")
    bad = R.violations(got, ref, mag, PARENT_UNITS[key])
    if bad.numel():
        i = tuple(bad[0].tolist())
        pytest.fail(f"{what}: {key} outside the bound at {bad.shape[0]} elements, e.g. {i}: got {float(got[i])!r}, ref {float(ref[i])!r}, "
                    f"magnitude {float(mag[i])!r} ({u:.2f} units)")


def check_operators(ops, dev, clip, tri, attr, diff, rast_d, seed, what):
    """Both operators, forward and every gradient, on the raster ``rast_d`` (on the device) against the restatement."""
    rast = rast_d.detach().cpu()
    tri_d = tri.to(dev)
    g_db = R.upstream(rast.shape, seed)
    c = clip.to(dev).requires_grad_(True)
    db = ops.rasterize_db(c, tri_d, rast_d.detach())
    assert db.shape == rast.shape and db.dtype == torch.float32
    (g_clip,) = torch.autograd.grad(db, c, g_db.to(dev))
    ref = R.rasterize_db_full(clip, tri, rast, g_db)
    _assert_within(db, ref["db"], ref["mag"], "db", what)
    _assert_within(g_clip, ref["g_clip"], ref["g_clip_mag"], "g_clip", what)
    assert float(g_clip[..., 2].abs().max()) == 0.0
    db_in = ref["db"].float()
    a, d = attr.to(dev).requires_grad_(True), db_in.to(dev).requires_grad_(True)
    da = ops.interpolate_da(a, rast_d.detach(), tri_d, d, diff)
    S = len(R.select(diff, attr.shape[2]))
    assert da.shape == (*rast.shape[:3], 2 * S)
    g_da = R.upstream(da.shape, seed + 1)
    g_attr, g_rdb = torch.autograd.grad(da, [a, d], g_da.to(dev))
    ref = R.interpolate_da_full(attr, rast, tri, db_in, diff, g_da)
    _assert_within(da, ref["da"], ref["mag"], "da", what)
    _assert_within(g_attr, ref["g_attr"], ref["g_attr_mag"], "g_attr", what)
    _assert_within(g_rdb, ref["g_db"], ref["g_db_mag"], "g_rast_db", what)
    unselected = [ch for ch in range(attr.shape[2]) if ch not in R.select(diff, attr.shape[2])]
    assert float(g_attr[..., unselected].abs().max() if unselected else 0.0) == 0.0
    return db


@gpu
@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_operators_against_the_restatement(name, dev, ops):
    """Instanced and shared clip / attr, B in {1, 2, 3, 16}, non-square and odd frames (W = 5, 7), C in {1, 2, 3, 8, 13, 24}, diff_attrs
    'all', a subset, a permuted subset and a list with a repeated index, S = 24 > 16 selected attributes (a3d_interp_da_bwd's per-pixel
    kernel instead of the tile scatter); perspective w in [0.6, 1.6], mixed winding."""
    sc = R.scene(name)
    rast = ops.rasterize(sc["clip"].to(dev), sc["tri"].to(dev), (sc["H"], sc["W"]), batch=sc["B"])
    assert int((rast[..., 3] > 0).sum()) > 0.2 * rast[..., 3].numel()
    check_operators(ops, dev, sc["clip"], sc["tri"], sc["attr"], sc["diff_attrs"], rast, sc["seed"], name)


@gpu
def test_operators_on_the_chain_scene(dev, ops):
    """The scene of test_textured_mesh_chain_into_dr_texture, operator by operator and element by element."""
    sc = R.chain_scene()
    rast = ops.rasterize(sc["clip"].to(dev), sc["tri"].to(dev), (sc["H"], sc["W"]))
    check_operators(ops, dev, sc["clip"], sc["tri"], sc["attr"], sc["diff_attrs"], rast, sc["seed"], "chain scene")


@gpu
@pytest.mark.parametrize("name", ["b3_odd_c3_subset", "b16_shared_c8_permuted"])
def test_second_depth_layer_through_the_shim(name, dev, ops, dr):
    """Layer 1 of a DepthPeeler: the rast_db it returns is the kernels' for the surface behind the first one."""
    sc = R.scene(name)
    pos = sc["clip"].expand(sc["B"], -1, -1).contiguous().to(dev).requires_grad_(True)
    with dr.DepthPeeler(dr.RasterizeGLContext(), pos, sc["tri"].to(dev), [sc["H"], sc["W"]]) as peeler:
        rast0, _ = peeler.rasterize_next_layer()
        rast1, db1 = peeler.rasterize_next_layer()
    assert int((rast1[..., 3] > 0).sum()) > 50 and not torch.equal(rast0[..., 3], rast1[..., 3])
    db = check_operators(ops, dev, sc["clip"], sc["tri"], sc["attr"], sc["diff_attrs"], rast1, sc["seed"], name + " layer 1")
    assert torch.equal(db1.materialize(), db)


@gpu
def test_a_raster_whose_resolve_was_deferred(dev, ops):
    """rasterize(defer_resolve=True) leaves the texels to its consumer: rasterize_db resolves them first (ensure_resolved)."""
    sc = R.scene("b1_square_uv")
    clip, tri = sc["clip"].to(dev), sc["tri"].to(dev)
    plain = ops.rasterize(clip, tri, (sc["H"], sc["W"]))
    want = ops.rasterize_db(clip, tri, plain)
    lazy = ops.rasterize(clip, tri, (sc["H"], sc["W"]), defer_resolve=True)
    was_pending = ops._pending_resolve.peek(lazy) is not None
    got = ops.rasterize_db(clip, tri, lazy)
    assert ops._pending_resolve.peek(lazy) is None and torch.equal(lazy, plain) and torch.equal(got, want)
    assert was_pending or not ops.dispatch_order_ok(dev)
    check_operators(ops, dev, sc["clip"], sc["tri"], sc["attr"], sc["diff_attrs"], lazy, 5, "deferred resolve")


@gpu
def test_range_mode_through_the_shim(dev, ops, dr):
    """pos [V,4] and attr [V,C] shared, image b renders tri[first : first + count]: the same kernels with batch stride 0."""
    sc = R.range_scene()
    clip, tri, attr, ranges, H, W = (sc[k] for k in ("clip", "tri", "attr", "ranges", "H", "W"))
    pos = clip[0].to(dev).requires_grad_(True)
    a = attr[0].to(dev).requires_grad_(True)
    rast, db = dr.rasterize(dr.RasterizeGLContext(), pos, tri.to(dev), [H, W], ranges=ranges)
    out, da = dr.interpolate(a, rast, tri.to(dev), rast_db=db, diff_attrs=[2, 0])
    assert da.shape == (3, H, W, 4) and float(da[2].abs().max()) == 0.0 and float(db[2].abs().max()) == 0.0
    g_db, g_da = R.upstream(rast.shape, 23), R.upstream(da.shape, 24)
    r = rast.detach().cpu()
    ref = R.rasterize_db_full(clip, tri, r, g_db)
    (g_pos,) = torch.autograd.grad(db.materialize(), pos, g_db.to(dev), retain_graph=True)
    _assert_within(db.materialize(), ref["db"], ref["mag"], "db", "range mode")
    _assert_within(g_pos[None], ref["g_clip"], ref["g_clip_mag"], "g_clip", "range mode")
    db_leaf = db.materialize().detach().requires_grad_(True)
    _, da2 = dr.interpolate(a, rast, tri.to(dev), rast_db=db_leaf, diff_attrs=[2, 0])
    g_a, g_rdb = torch.autograd.grad(da2, [a, db_leaf], g_da.to(dev))
    ref = R.interpolate_da_full(attr, r, tri, db_leaf.detach().cpu(), [2, 0], g_da)
    _assert_within(da2, ref["da"], ref["mag"], "da", "range mode")
    _assert_within(g_a[None], ref["g_attr"], ref["g_attr_mag"], "g_attr", "range mode")
    _assert_within(g_rdb, ref["g_db"], ref["g_db_mag"], "g_rast_db", "range mode")


@gpu
def test_an_empty_image_gives_zeros_and_zero_gradients(dev, ops, dr):
    sc = R.empty_scene()  # everything off screen
    clip, tri = sc["clip"], sc["tri"]
    pos = clip.to(dev).requires_grad_(True)
    attr = sc["attr"].to(dev).requires_grad_(True)
    rast, db = dr.rasterize(dr.RasterizeGLContext(), pos, tri.to(dev), [19, 23])
    _, da = dr.interpolate(attr, rast, tri.to(dev), rast_db=db, diff_attrs="all")
    assert float(rast[..., 3].max()) == 0.0
    assert torch.equal(db.materialize(), torch.zeros(2, 19, 23, 4, device=dev)) and torch.equal(da, torch.zeros(2, 19, 23, 6, device=dev))
    g_pos, g_attr = torch.autograd.grad((da * 3.0).sum() + db.materialize().sum(), [pos, attr])
    assert float(g_pos.abs().max()) == 0.0 and float(g_attr.abs().max()) == 0.0
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("H,W", [(32, 64), (16, 4)])
def test_known_answer_orthographic_axis_aligned_triangle(H, W, dev, ops, dr):
    """w = 1, vertices (3,-1), (-1,3), (-1,-1): the edge matrix [p0 - p2, p1 - p2] is 4 I, so rast_db is the constant (1/4 * 2/W, 0, 0,
    1/4 * 2/H) and out_da of the attribute uv = xy the constant (2/W, 0, 0, 2/H).  Every coordinate is a power of two or a small odd
    multiple of one and every fp32 operation is exact: torch.equal."""
    pos = torch.tensor([[[3.0, -1.0, 0.0, 1.0], [-1.0, 3.0, 0.0, 1.0], [-1.0, -1.0, 0.0, 1.0]]], device=dev)
    tri = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    rast, db = dr.rasterize(dr.RasterizeGLContext(), pos, tri, [H, W])
    assert float(rast[..., 3].min()) == 1.0  # the triangle covers the frame
    want = torch.tensor([0.5 / W, 0.0, 0.0, 0.5 / H], device=dev).expand(1, H, W, 4)
    assert torch.equal(db.materialize(), want)
    uv, da = dr.interpolate(pos[..., :2].contiguous(), rast, tri, rast_db=db, diff_attrs="all")
    assert torch.equal(da, torch.tensor([2.0 / W, 0.0, 0.0, 2.0 / H], device=dev).expand(1, H, W, 4))
    # a general orthographic triangle: the inverse of its edge matrix scaled by 2/W and 2/H, constant over the triangle
    p = torch.tensor([[[-0.8, -0.7, 0.1, 1.0], [0.9, -0.4, 0.3, 1.0], [-0.1, 0.85, 0.2, 1.0]]], dtype=torch.float64)
    M = torch.stack([p[0, 0, :2] - p[0, 2, :2], p[0, 1, :2] - p[0, 2, :2]], -1)
    inv = torch.linalg.inv(M) * torch.tensor([2.0 / W, 2.0 / H], dtype=torch.float64)
    rast = ops.rasterize(p.float().to(dev), tri, (H, W))
    got = ops.rasterize_db(p.float().to(dev), tri, rast).cpu().double()
    cov = rast[..., 3].cpu() > 0
    assert int(cov.sum()) > 0
    np.testing.assert_allclose(got[cov].numpy(), inv.reshape(-1).expand(int(cov.sum()), 4).numpy(), rtol=2e-5, atol=1e-9)
    assert float(got[~cov].abs().max()) == 0.0


@gpu
def test_textured_mesh_chain_into_dr_texture(dev, ops, dr):
    """dr.rasterize -> dr.interpolate(uv, rast_db, 'all') -> dr.texture(tex, uv, uv_da) with gradients to tex, the uv attribute and pos,
    against the same chain in float64 (deriv_ref + texture_ref).  The chain's fp32 error is dominated by stages this change does not
    touch (the barycentrics of the raster buffer, the level of detail's log2, the texture scatter), so its bound is taken from the same
    chain with the torch statements in place of the kernels, run beside it: 4 x that chain's largest error per tensor plus 1e-6 of the
    tensor's largest magnitude.  That is a bound per tensor, not per element, and it is meant as one: this test is about the wiring --
    the gradient of the colour reaches tex, the uv attribute and pos through BOTH new backwards (pos only through rast_db's and the
    raster buffer's) -- while the precision of each operator, element by element, and the dropped pixel are the business of the
    operator tests above, which run on this scene too (test_operators_on_the_chain_scene)."""
    sc = R.chain_scene()
    B, H, W, clip, tri, uv_attr, tex = (sc[k] for k in ("B", "H", "W", "clip", "tri", "attr", "tex"))
    g_out = R.upstream((B, H, W, 3), sc["seed"])
    tri_d = tri.to(dev)

    def chain(kernels):
        pos, a, t = (x.to(dev).requires_grad_(True) for x in (clip, uv_attr, tex))
        rast, db = dr.rasterize(dr.RasterizeGLContext(), pos, tri_d, [H, W])
        if kernels:
            uv, uv_da = dr.interpolate(a, rast, tri_d, rast_db=db, diff_attrs="all")
        else:
            uv = ops.interpolate(a, rast, tri_d)
            uv_da = ops._interpolate_da_torch(a, rast, tri_d, ops._rasterize_db_torch(pos, tri_d, rast), "all")
        col = dr.texture(t, uv, uv_da, filter_mode="linear-mipmap-linear")
        return [col.detach().cpu()] + [g.cpu() for g in torch.autograd.grad(col, [t, a, pos], g_out.to(dev))], rast.detach().cpu()

    got, rast = chain(True)
    parent, rast_p = chain(False)
    assert torch.equal(rast, rast_p)
    pos, a, t = (x.double().requires_grad_(True) for x in (clip, uv_attr, tex))
    bary = R.barycentric_map(pos, tri, rast)
    uv = R.interpolate(a, rast, tri, bary)
    uv_da = R.interpolate_da(a, rast, tri, R.rasterize_db(pos, tri, rast), "all")
    col = T.texture(t, uv, uv_da, filter_mode="linear-mipmap-linear")
    ref = [col.detach()] + list(torch.autograd.grad(col, [t, a, pos], g_out.double()))
    for k, x, p, r in zip(("colour", "g_tex", "g_uv_attr", "g_pos"), got, parent, ref):
        e_k, e_p = float((x.double() - r).abs().max()), float((p.double() - r).abs().max())
        print(f"chain {k}: kernels {e_k:.3e}, torch statements {e_p:.3e}, max |ref| {float(r.abs().max()):.3e}")
        assert e_k <= 4 * e_p + 1e-6 * float(r.abs().max()), (k, e_k, e_p)


@gpu
def test_launch_counts_and_peak_memory(dev, ops, dr, L):
    """Materialising rast_db is one a3d_* call, interpolate(..., diff_attrs=) two (a3d_interp_fwd and a3d_interp_da_fwd), and none of
    the torch path's gather temporaries exists: the peak of the new path lies below the torch path's by at least one [B,H,W,3,4]
    float tensor on the same call."""
    B, H, W = 16, 128, 128
    clip, tri = R.soup(12, 51, B=B)
    pos, tri_d = clip.to(dev), tri.to(dev)
    attr = R.attributes(1, clip.shape[1], 2, 52).to(dev)
    rast, db = dr.rasterize(dr.RasterizeGLContext(), pos, tri_d, [H, W], grad_db=False)
    torch.cuda.synchronize()
    with L.KernelTimer() as t:
        dense = db.materialize()
    assert {k: c for k, (c, _) in t.summary().items()} == {"a3d_rast_db_fwd": 1}
    with L.KernelTimer() as t:
        dr.interpolate(attr, rast, tri_d, rast_db=db, diff_attrs="all")
    assert {k: c for k, (c, _) in t.summary().items()} == {"a3d_interp_fwd[C2]": 1, "a3d_interp_da_fwd[S2]": 1}

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        del out
        return torch.cuda.max_memory_allocated() - base

    one_gather = B * H * W * 3 * 4 * 4
    for new, old in ((lambda: ops.rasterize_db(pos, tri_d, rast), lambda: ops._rasterize_db_torch(pos, tri_d, rast)),
                     (lambda: ops.interpolate_da(attr, rast, tri_d, dense, "all"), lambda: ops._interpolate_da_torch(attr, rast, tri_d, dense, "all"))):
        p_new, p_old = peak(new), peak(old)
        print(f"peak bytes: kernels {p_new}, torch statements {p_old}, one [B,H,W,3,4] float tensor {one_gather}")
        assert p_new <= p_old - one_gather, (p_new, p_old, one_gather)


@gpu
def test_double_backward_falls_back_to_the_torch_statement(dev, ops):
    """A backward under create_graph=True differentiates the torch statement, for both operators: the second-order gradients equal those
    of the torch statements called directly.  Both sides run the same operations; only index_put's order of summation per vertex differs
    from run to run on the device, which for the at most 2^10 pixels that feed a vertex here is 2^10 x 2^-24 = 6e-5 of the summed terms:
    1e-4 of the largest value."""
    sc = R.scene("b1_square_uv")
    tri = sc["tri"].to(dev)
    rast = ops.rasterize(sc["clip"].to(dev), tri, (sc["H"], sc["W"]))
    assert int((rast[..., 3] > 0).sum()) <= 64 * 64

    def close(got, want, what):
        assert bool(torch.isfinite(got).all()) and float(want.abs().max()) > 0, what
        err, top = float((got - want).abs().max()), float(want.abs().max())
        print(f"double backward {what}: max error {err:.3e}, max |value| {top:.3e}")
        assert err <= 1e-4 * top, (what, err, top)

    def second_db(fn):
        clip = sc["clip"].to(dev).requires_grad_(True)
        (g,) = torch.autograd.grad(fn(clip, tri, rast).sum(), clip, create_graph=True)
        return torch.autograd.grad((g * g).sum(), clip)[0]

    close(second_db(ops.rasterize_db), second_db(ops._rasterize_db_torch), "rasterize_db -> clip")
    db = ops.rasterize_db(sc["clip"].to(dev), tri, rast).detach()
    w_a, w_d = R.upstream(sc["attr"].shape, 61).to(dev), R.upstream(db.shape, 62).to(dev)
    g_da = R.upstream((*db.shape[:3], 2 * sc["attr"].shape[2]), 63).to(dev)

    def second_da(fn):
        a, d = sc["attr"].to(dev).requires_grad_(True), db.clone().requires_grad_(True)
        g_a, g_d = torch.autograd.grad(fn(a, rast, tri, d, sc["diff_attrs"]), [a, d], g_da, create_graph=True)
        assert g_a.requires_grad and g_d.requires_grad
        return torch.autograd.grad((g_a * w_a).sum() + (g_d * w_d).sum(), [a, d])

    for got, want, what in zip(second_da(ops.interpolate_da), second_da(ops._interpolate_da_torch), ("attr", "rast_db")):
        close(got, want, "interpolate_da -> " + what)
