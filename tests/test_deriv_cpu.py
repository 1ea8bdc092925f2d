"""Image-space derivatives without a GPU: the entry points of include/a3d_deriv.h, argument validation
before any launch, the float64 restatement (tests/deriv_ref.py) against finite differences of the barycentrics, the torch fp32 path
against that restatement on every pixel of every scene of the GPU test (the measurement its bounds come from), and the sensitivity of
those bounds to one dropped pixel."""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check as A  # noqa: E402
import deriv_ref as R  # noqa: E402
from test_deriv_gpu import PARENT_UNITS  # noqa: E402

ENTRIES = ("a3d_rast_db_fwd", "a3d_rast_db_bwd", "a3d_interp_da_fwd", "a3d_interp_da_bwd")


def _L():
    return importlib.import_module("3danimals_amd._lib")


def _ops():
    return importlib.import_module("3danimals_amd.ops")


def test_third_header_matches_the_third_table_and_the_other_surfaces_are_untouched():
    """What is this surface's own (tests/test_abi_cpu.py holds every surface's table and constants to its header)."""
    protos = A.prototypes("a3d_deriv.h")
    assert set(protos) == set(ENTRIES)
    assert protos["a3d_rast_db_fwd"] != ("int", ["ptr"]) and len(protos["a3d_interp_da_bwd"][1]) == 17


def test_invalid_arguments_are_refused_before_anything_is_launched():
    """None of the pointers below is ever dereferenced and nothing is launched (this runs without a GPU)."""
    L = _L()
    lib = L.lib()
    p = 0x1000

    def refused(name, *args):
        assert getattr(lib, name)(*args) == -1, name
        msg = lib.a3d_last_error().decode()
        assert "invalid argument" in msg and name in msg, msg

    refused("a3d_rast_db_fwd", None, 1, p, p, 1, 3, 1, 8, 8, p, None)  # no clip
    refused("a3d_rast_db_fwd", p, 2, p, p, 3, 3, 1, 8, 8, p, None)  # clip batch neither 1 nor B
    refused("a3d_rast_db_fwd", p, 1, None, p, 1, 3, 1, 8, 8, p, None)  # triangles without a list
    refused("a3d_rast_db_bwd", p, p, 1, p, p, 1, 3, 1, 0, 8, p, None)  # H = 0
    refused("a3d_rast_db_bwd", p, p, 1, p, p, 1, 3, 1, 8, 8, None, None)  # no g_clip
    refused("a3d_interp_da_fwd", p, 1, 65, None, 65, p, p, p, 1, 3, 1, 8, 8, p, None)  # C > 64
    refused("a3d_interp_da_fwd", p, 1, 3, None, 2, p, p, p, 1, 3, 1, 8, 8, p, None)  # 'all' with S != C
    refused("a3d_interp_da_fwd", p, 1, 3, p, 0, p, p, p, 1, 3, 1, 8, 8, p, None)  # nothing selected
    refused("a3d_interp_da_fwd", p, 1, 3, p, 65, p, p, p, 1, 3, 1, 8, 8, p, None)  # S > A3D_DERIV_MAX_SELECTED
    refused("a3d_interp_da_bwd", p, p, 1, 3, None, 3, p, p, p, 1, 3, 1, 8, 8, None, None, None)  # no gradient wanted
    refused("a3d_interp_da_bwd", p, p, 2, 3, None, 3, p, p, p, 3, 3, 1, 8, 8, p, p, None)  # attr batch neither 1 nor B


def test_ops_keep_the_torch_statement_for_cpu_and_float64_tensors():
    """CPU tensors (any dtype) evaluate the torch statement; in float64 it agrees with the restatement up to its pixel centres, which it
    forms in float32 whatever the dtype of clip (6e-8 relative on f, a few times that on the derivatives: 1e-6 of the largest value)."""
    ops = _ops()
    sc = R.scene("b3_odd_c3_subset")
    rast = _raster(sc)
    db = ops.rasterize_db(sc["clip"].double(), sc["tri"], rast)
    assert db.dtype == torch.float64
    ref = R.rasterize_db_full(sc["clip"], sc["tri"], rast)
    assert float((db - ref["db"]).abs().max()) <= 1e-6 * float(ref["db"].abs().max())
    da = ops.interpolate_da(sc["attr"].double(), rast, sc["tri"], db, sc["diff_attrs"])
    want = R.interpolate_da(sc["attr"], rast, sc["tri"], db, sc["diff_attrs"])
    assert da.shape == want.shape and float((da - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(ops.rasterize_db(sc["clip"], sc["tri"], rast), ops._rasterize_db_torch(sc["clip"], sc["tri"], rast))
    with pytest.raises(IndexError):
        ops._selected([0, 3], 3)
    with pytest.raises(ValueError):
        ops._selected("some", 3)
    assert ops._selected("all", 3) is None and ops._selected([-1, 0, 0], 3) == (2, 0, 0)


def test_restatement_agrees_with_finite_differences_of_the_barycentrics():
    """rast_db of the restatement against central differences of (u, v) evaluated at f +- h (float64, h = 1e-6 in NDC; the second-order
    term is ~h^2 |u'''| ~ 1e-11 relative for these triangles), on a handful of triangles and pixels.  This pins the specification."""
    H, W, h = 21, 34, 1e-6
    for seed in range(6):
        clip, tri = R.soup(1, 50 + seed)
        P = clip[0].double()
        rast = torch.zeros(1, H, W, 4)
        rast[..., 3] = 1.0
        db = R.rasterize_db(clip, tri, rast)[0]
        for (py, px) in ((0, 0), (5, 30), (20, 33), (11, 17)):
            fx, fy = R.centres(W)[px], R.centres(H)[py]
            ux1, vx1 = R.barycentrics(P, fx + h, fy)
            ux0, vx0 = R.barycentrics(P, fx - h, fy)
            uy1, vy1 = R.barycentrics(P, fx, fy + h)
            uy0, vy0 = R.barycentrics(P, fx, fy - h)
            fd = torch.stack([(ux1 - ux0) / (2 * h) * 2 / W, (uy1 - uy0) / (2 * h) * 2 / H, (vx1 - vx0) / (2 * h) * 2 / W,
                              (vy1 - vy0) / (2 * h) * 2 / H])
            assert float((db[py, px] - fd).abs().max()) <= 1e-8 * float(fd.abs().max()) + 1e-12, (seed, py, px, db[py, px], fd)
    # ... and interpolate_da is the chain rule on the interpolated attribute: A(f) = u A0 + v A1 + (1 - u - v) A2
    clip, tri = R.soup(1, 77)
    attr = R.attributes(1, 3, 2, 5)
    rast = torch.zeros(1, H, W, 4)
    rast[..., 3] = 1.0
    da = R.interpolate_da(attr, rast, tri, R.rasterize_db(clip, tri, rast), "all")[0, 7, 9]
    A, P = attr[0].double(), clip[0].double()
    val = lambda fx, fy: (lambda u, v: u * A[0] + v * A[1] + (1 - u - v) * A[2])(*R.barycentrics(P, fx, fy))
    fx, fy = R.centres(W)[9], R.centres(H)[7]
    dX = (val(fx + h, fy) - val(fx - h, fy)) / (2 * h) * 2 / W
    dY = (val(fx, fy + h) - val(fx, fy - h)) / (2 * h) * 2 / H
    fd = torch.stack([dX, dY], -1).reshape(-1)
    assert float((da - fd).abs().max()) <= 1e-8 * float(fd.abs().max())


def _raster(sc, layer=0):
    from oracle import raster_ref

    clip = sc["clip"].expand(sc["B"], -1, -1).contiguous()
    rast = raster_ref.rasterize(clip, sc["tri"], (sc["H"], sc["W"]))
    for _ in range(layer):
        rast = raster_ref.rasterize(clip, sc["tri"], (sc["H"], sc["W"]), prev=rast)
    return rast


def parent_path_units(sc, rast, ops):
    """The torch fp32 path (ops._rasterize_db_torch / ops._interpolate_da_torch and their autograd) against the restatement on one scene:
    dict quantity -> error in units of 2^-24 x magnitude (deriv_ref.units: the maximum over every element; nothing is masked)."""
    clip, tri, attr, diff = sc["clip"], sc["tri"], sc["attr"], sc["diff_attrs"]
    g_db = R.upstream(rast.shape, sc["seed"])
    c = clip.clone().requires_grad_(True)
    db = ops._rasterize_db_torch(c, tri, rast)
    (g_clip,) = torch.autograd.grad(db, c, g_db)
    ref = R.rasterize_db_full(clip, tri, rast, g_db)
    out = dict(db=R.units(db.detach(), ref["db"], ref["mag"]), g_clip=R.units(g_clip, ref["g_clip"], ref["g_clip_mag"]))
    db_in = ref["db"].float()  # both sides start from the same fp32 rast_db
    a, d = attr.clone().requires_grad_(True), db_in.clone().requires_grad_(True)
    da = ops._interpolate_da_torch(a, rast, tri, d, diff)
    g_da = R.upstream(da.shape, sc["seed"] + 1)
    g_attr, g_rdb = torch.autograd.grad(da, [a, d], g_da)
    ref = R.interpolate_da_full(attr, rast, tri, db_in, diff, g_da)
    out.update(da=R.units(da.detach(), ref["da"], ref["mag"]), g_attr=R.units(g_attr, ref["g_attr"], ref["g_attr_mag"]),
               g_rast_db=R.units(g_rdb, ref["g_db"], ref["g_db_mag"]))
    return out


@pytest.mark.parametrize("name", sorted(R.SCENES))
@pytest.mark.parametrize("layer", [0, 1])
def test_torch_fp32_path_stays_within_the_recorded_units_on_every_pixel(name, layer):
    """The measurement behind PARENT_UNITS (tests/test_deriv_gpu.py): on every scene of the GPU test, first and second depth layer,
    every element of every quantity of the torch fp32 path lies within the recorded units.  No pixel is excluded; a scene for which
    this fails is to be replaced, not masked."""
    sc = R.scene(name)
    rast = _raster(sc, layer)
    assert int((rast[..., 3] > 0).sum()) > 0.2 * rast[..., 3].numel() or layer > 0
    # one thread: index_put's accumulation order on a multi-threaded CPU changes from run to run (g_attr of one scene was seen between
    # 1.83 and 2.43 units); the recorded figures are those of the sequential order, which every machine reproduces
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        got = parent_path_units(sc, rast, _ops())
    finally:
        torch.set_num_threads(threads)
    print(name, layer, {k: round(v, 3) for k, v in got.items()})
    for k, v in got.items():
        assert v <= PARENT_UNITS[k], (name, layer, k, v, PARENT_UNITS[k])


def _raster_ranges(sc):
    """Range mode as the stand-in rasterises it: image b over tri[first : first + count], the ids re-based to the full list."""
    from oracle import raster_ref

    layers = []
    for first, count in sc["ranges"].tolist():
        if count <= 0:
            layers.append(torch.zeros(1, sc["H"], sc["W"], 4))
            continue
        r = raster_ref.rasterize(sc["clip"], sc["tri"][first:first + count].contiguous(), (sc["H"], sc["W"]))
        r[..., 3] = torch.where(r[..., 3] > 0, r[..., 3] + float(first), r[..., 3])
        layers.append(r)
    return torch.cat(layers, 0)


@pytest.mark.parametrize("which", ["range", "empty", "chain"])
def test_torch_fp32_path_on_the_scenes_of_the_other_gpu_tests(which):
    """The same measurement on the remaining scenes of tests/test_deriv_gpu.py: range mode, the image nothing covers (every figure is
    zero there) and the textured-mesh chain's scene."""
    sc = dict(range=R.range_scene, empty=R.empty_scene, chain=R.chain_scene)[which]()
    rast = _raster_ranges(sc) if which == "range" else _raster(sc)
    covered = int((rast[..., 3] > 0).sum())
    assert covered == 0 if which == "empty" else covered > 0.2 * rast[..., 3].numel()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        got = parent_path_units(sc, rast, _ops())
    finally:
        torch.set_num_threads(threads)
    print(which, {k: round(v, 3) for k, v in got.items()})
    for k, v in got.items():
        assert v <= PARENT_UNITS[k], (which, k, v, PARENT_UNITS[k])


def test_bounds_catch_one_dropped_pixel():
    """Sensitivity, CPU only: the float64 gradients with ONE pixel's contribution removed from a vertex must violate the kernels' bound
    (4 x PARENT_UNITS x magnitude + 4 ulp), for g_clip and g_attr at a sample of vertices; the removed pixel is the one of median size
    among those that feed the vertex.  A dropped pixel of the per-pixel outputs (a zero where a value belongs) violates theirs."""
    rng = torch.Generator().manual_seed(0)
    for name in ("b1_square_uv", "b3_c13_all"):
        sc = R.scene(name)
        rast = _raster(sc)
        g_db = R.upstream(rast.shape, 3)
        rd = R.rasterize_db_full(sc["clip"], sc["tri"], rast, g_db)
        g_da = R.upstream((*rast.shape[:3], 2 * len(R.select(sc["diff_attrs"], sc["attr"].shape[2]))), 4)
        ia = R.interpolate_da_full(sc["attr"], rast, sc["tri"], rd["db"].float(), sc["diff_attrs"], g_da)
        for full, key, unit_key, comps in ((rd, "g_clip", "g_clip", [0, 1, 3]), (ia, "g_attr", "g_attr", None)):
            ref, mag = full[key].reshape(-1, full[key].shape[-1]), full[key + "_mag"].reshape(-1, full[key].shape[-1])
            assert R.violations(ref, ref, mag, PARENT_UNITS[unit_key]).numel() == 0
            fed = torch.nonzero(full["feeds"] > 1).reshape(-1)
            sample = fed[torch.randperm(fed.numel(), generator=rng)[:12]]
            assert sample.numel() >= 6
            for r in sample.tolist():
                where = torch.nonzero(full["rows"] == r)
                size = full["contrib"][where[:, 0], where[:, 1]].abs().amax(-1)
                pick = where[int(torch.argsort(size)[size.numel() // 2])]
                dropped = ref.clone()
                dropped[r] -= full["contrib"][pick[0], pick[1]]
                bad = R.violations(dropped, ref, mag, PARENT_UNITS[unit_key])
                assert r in bad[:, 0].tolist(), (name, key, r, int(full["feeds"][r]))
        for ref, mag, k in ((rd["db"], rd["mag"], "db"), (ia["da"], ia["mag"], "da"), (ia["g_db"], ia["g_db_mag"], "g_rast_db")):
            live = torch.nonzero(ref.abs().amax(-1) > 0)
            b, y, x = live[live.shape[0] // 2].tolist()
            dropped = ref.clone()
            dropped[b, y, x] = 0.0
            assert R.violations(dropped, ref, mag, PARENT_UNITS[k]).numel() > 0, (name, k)


def test_restatement_hands_no_gradient_back_from_pixels_without_a_triangle():
    """A consumer of out_da may hand back a non-finite gradient at a pixel no triangle covers (a mip-mapped lookup: uv_da = 0 there,
    the level of detail is log2(0)).  Nothing feeds such a pixel, so the restatement's gradients stay finite and equal those of a zero
    upstream gradient there -- on a scene and on an image that nothing covers (gradients: exact zeros)."""
    sc = R.scene("b3_odd_c3_subset")
    for rast in (_raster(sc), torch.zeros(sc["B"], sc["H"], sc["W"], 4)):
        empty = rast[..., 3] == 0
        assert bool(empty.any())
        g = R.upstream((*rast.shape[:3], 4), 7).double()
        grads = []
        for fill in (0.0, float("nan")):
            clip, attr = sc["clip"].double().requires_grad_(True), sc["attr"].double().requires_grad_(True)
            da = R.interpolate_da(attr, rast, sc["tri"], R.rasterize_db(clip, sc["tri"], rast), sc["diff_attrs"])
            up = g.clone()
            up[empty] = fill
            grads.append(torch.autograd.grad(da, [clip, attr], up))
        for zero, nan in zip(*grads):
            assert bool(torch.isfinite(nan).all()) and torch.equal(zero, nan)
            assert bool(empty.all()) == (float(nan.abs().max()) == 0.0)
