"""The environment-probe resamplers on the GPU: ops.latlong_to_cubemap / ops.cubemap_to_latlong (csrc/texture.hip with generated
coordinates, uv == NULL) against the float64 restatement tests/envmap_ref.py, forward and backward; the routes of util's two functions;
a .hdr probe in, a light, a .hdr probe out.

Forward bound: max |HIP - float64| <= c * 2^-23 * L * (max tex - min tex), L the larger source dimension -- the form a coordinate error
of c ulp takes through a bilinear tap.  RATIOS_LL / RATIOS_CUBE below record, per case, e_ref (the float32 restatement's own ratio on
the CPU) and the kernel's ratio as measured on an MI355X: lat-long -> cube, e_ref up to 0.574 and the kernel up to 0.575; cube ->
lat-long, where L = S is small and the tap's own roundings show, e_ref up to 1.557 and the kernel up to 1.503.  C_LL = 1.15 and C_CUBE =
3.006 are twice the kernel's worst, and the forward tests hold them under 8 x the worst e_ref of their
direction (ocml's atan2f / acosf / sinf / cosf are a few ulp where libm is one: a larger gap is a bug, not rounding).

Poles: a texel of the cube that looks along +-y (x^2 + z^2 < 1e-12: the centre of the +-y faces at odd sizes, at most 2 per cube) has
no defined longitude; random maps leave exactly those out, maps with constant top and bottom rows leave nothing out.

Backward: the gradient of the map against float64 autograd of the restatement within R.g_tex_bounds, the per-texel bound of
tests/test_texture_backward_gpu.py for the same scatter; the adjoint identity within the sum of that bound and its per-lookup one.
Measured worst error over bound: 0.03 .. 0.20 for the small cases, 0.85 for 64 x 128 -> 33 (there the generated longitude's own
float32 error, W * 2^-24 texels, is most of what that bound allows a lookup whose uv is given).
"""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import envmap_ref as E  # noqa: E402
import texture_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

EPS23 = 2.0 ** -23
CHANNELS = (1, 3, 4, 5)
LL_CASES = [((4, 8), (1, 1)), ((4, 8), (2, 2)), ((5, 7), (3, 3)), ((8, 16), (4, 4)), ((8, 16), (2, 3)), ((16, 32), (7, 7)), ((16, 32), (8, 8))]
LL_BIG = ((64, 128), (33, 33))
CUBE_CASES = [(S, res) for S in (1, 2, 4, 7) for res in ((1, 2), (3, 5), (8, 16), (16, 32))]

# Per case, the worst ratio over C in CHANNELS and both kinds of map: (e_ref, kernel).  e_ref is recomputed (and printed) by every run;
# the kernel's column was measured on an MI355X.
RATIOS_LL = {
    ((4, 8), (1, 1)): (0.050, 0.066), ((4, 8), (2, 2)): (0.512, 0.575), ((5, 7), (3, 3)): (0.302, 0.403), ((8, 16), (4, 4)): (0.374, 0.242),
    ((8, 16), (2, 3)): (0.224, 0.209), ((16, 32), (7, 7)): (0.400, 0.432), ((16, 32), (8, 8)): (0.425, 0.418),
    ((64, 128), (33, 33)): (0.574, 0.570),
}
RATIOS_CUBE = {
    (1, (1, 2)): (0.550, 0.550), (1, (3, 5)): (0.820, 0.820), (1, (8, 16)): (1.178, 1.092), (1, (16, 32)): (1.371, 1.402),
    (2, (1, 2)): (0.317, 0.317), (2, (3, 5)): (0.341, 0.457), (2, (8, 16)): (0.915, 0.915), (2, (16, 32)): (1.557, 1.503),
    (4, (1, 2)): (0.250, 0.250), (4, (3, 5)): (0.324, 0.401), (4, (8, 16)): (0.990, 0.972), (4, (16, 32)): (1.527, 1.401),
    (7, (1, 2)): (0.429, 0.429), (7, (3, 5)): (0.409, 0.395), (7, (8, 16)): (1.101, 1.101), (7, (16, 32)): (1.264, 1.224),
}
E_REF_LL, E_REF_CUBE = max(e for e, _ in RATIOS_LL.values()), max(e for e, _ in RATIOS_CUBE.values())  # 0.574, 1.557
C_LL, C_CUBE = 2 * max(k for _, k in RATIOS_LL.values()), 2 * max(k for _, k in RATIOS_CUBE.values())  # 1.15, 3.006


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("3danimals_amd.ops")


@pytest.fixture(scope="module")
def util():
    return importlib.import_module("3danimals_amd.model.render.util")


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * 131 ** i for i, k in enumerate(key)) % (2 ** 31))


def _latlong(size, C, seed, flat_rows=False):
    tex = torch.rand(*size, C, generator=_gen(*size, C, seed), dtype=torch.float32)
    if flat_rows:
        tex[0], tex[-1] = tex[0, :1].clone(), tex[-1, :1].clone()
    return tex


def _ratio(got, want, tex, L, live=None):
    err = (got.double().cpu() - want).abs()
    if live is not None:
        err = err[live]
    span = float(tex.max() - tex.min())
    return float(err.max()) / (EPS23 * L * span) if span > 0 else float(err.max())


def _constants_are_rounding_sized():
    assert C_LL <= 8 * E_REF_LL and C_CUBE <= 8 * E_REF_CUBE
    assert set(RATIOS_LL) == set(LL_CASES + [LL_BIG]) and set(RATIOS_CUBE) == set(CUBE_CASES)


@pytest.mark.parametrize("size, res", LL_CASES + [LL_BIG], ids=lambda v: "x".join(map(str, v)))
def test_latlong_to_cubemap_forward(dev, ops, size, res):
    _constants_are_rounding_sized()
    poles = E.pole_mask(res)
    assert int(poles.sum()) <= 2 and (int(poles.sum()) == 0 or (res[0] % 2 and res[1] % 2))
    worst = 0.0
    for C in (CHANNELS if (size, res) != LL_BIG else (3,)):
        for flat_rows in (False, True):
            tex = _latlong(size, C, 1, flat_rows)
            got = ops.latlong_to_cubemap(tex.to(dev), list(res))
            assert got.dtype == torch.float32 and tuple(got.shape) == (6, res[0], res[1], C) and got.device == dev
            want = E.latlong_to_cubemap(tex, res)
            e_ref = _ratio(E.latlong_to_cubemap(tex, res, torch.float32), want, tex, max(size), None if flat_rows else ~poles)
            r = _ratio(got, want, tex, max(size), None if flat_rows else ~poles)
            print(f"RATIO ll2c {size} {res} C{C} flat_rows={int(flat_rows)} e_ref={e_ref:.3f} hip={r:.3f}")
            worst = max(worst, r)
    assert worst <= C_LL, worst


@pytest.mark.parametrize("S, res", CUBE_CASES, ids=lambda v: str(v) if isinstance(v, int) else "x".join(map(str, v)))
def test_cubemap_to_latlong_forward(dev, ops, S, res):
    _constants_are_rounding_sized()
    worst = 0.0
    for C in CHANNELS:
        tex = torch.rand(6, S, S, C, generator=_gen(S, *res, C), dtype=torch.float32)
        got = ops.cubemap_to_latlong(tex.to(dev), list(res))
        assert got.dtype == torch.float32 and tuple(got.shape) == (res[0], res[1], C)
        want = E.cubemap_to_latlong(tex, res)
        e_ref = _ratio(E.cubemap_to_latlong(tex, res, torch.float32), want, tex, S)
        r = _ratio(got, want, tex, S)
        print(f"RATIO c2ll S{S} {res} C{C} e_ref={e_ref:.3f} hip={r:.3f}")
        worst = max(worst, r)
    assert worst <= C_CUBE, worst


# ------------------------------------------------------------------------------------------------ structured inputs
@pytest.mark.parametrize("size, res", [((5, 7), (3, 3)), ((16, 32), (8, 8)), ((16, 32), (7, 7))], ids=lambda v: "x".join(map(str, v)))
def test_structured_maps(dev, ops, size, res):
    H, W = size
    # a constant map returns the constant within 2 ulp, poles included
    for c in (0.7, 1.0, 3.25):
        out = ops.latlong_to_cubemap(torch.full((H, W, 4), c, dtype=torch.float32, device=dev), list(res)).cpu()
        assert float((out.double() - float(np.float32(c))).abs().max()) <= 2 * float(np.spacing(np.float32(c))), c
        # (the cube tap: up to 4 products, 3 sums and a corner's thirds, half an ulp each)
        cube = ops.cubemap_to_latlong(torch.full((6, 4, 4, 3), c, dtype=torch.float32, device=dev), [size[0], size[1]]).cpu()
        assert float((cube.double() - float(np.float32(c))).abs().max()) <= 4 * float(np.spacing(np.float32(c))), c
    # a row-only ramp isolates tv (no pole is left out: tu does not matter), a column-only ramp across the tu = 0 / 1 seam isolates tu
    rows = (torch.arange(H, dtype=torch.float32) / 4)[:, None, None].expand(H, W, 3).contiguous()
    cols = (torch.arange(W, dtype=torch.float32) / 4)[None, :, None].expand(H, W, 3).contiguous()
    live = ~E.pole_mask(res)
    for name, tex, L, keep in (("rows", rows, H, None), ("cols", cols, W, live)):
        got = ops.latlong_to_cubemap(tex.to(dev), list(res))
        r = _ratio(got, E.latlong_to_cubemap(tex, res), tex, L, keep)
        print(f"RATIO ramp {name} {size} {res} hip={r:.3f}")
        assert r <= C_LL, (name, r)
    if res[1] % 2:  # the +z face's centre column looks along the seam tu = 0 / 1: half of the last column, half of the first
        got = ops.latlong_to_cubemap(cols.to(dev), list(res)).cpu()
        mid = (0.5 * (cols[0, 0] + cols[0, -1]))[None].expand(res[0], 3)
        assert float((got[4, :, res[1] // 2] - mid).abs().max()) <= C_LL * EPS23 * W * float(cols.max() - cols.min())


# ------------------------------------------------------------------------------------------------ backward
def _backward_case(ops, dev, kind, tex, res, w):
    """(g of the map from the kernel, float64 g, its per-texel bound, out, float64 out, per-lookup bound on out)."""
    t = tex.to(dev).requires_grad_(True)
    fn = ops.latlong_to_cubemap if kind == "ll" else ops.cubemap_to_latlong
    out = fn(t, list(res))
    out.backward(w.to(dev))
    t64 = tex.double().requires_grad_(True)
    ref = (E.latlong_to_cubemap if kind == "ll" else E.cubemap_to_latlong)(t64, res)
    ref.backward(w.double())
    if kind == "ll":
        uv, _ = E.latlong_coords(res, torch.float64)
        kw, w4 = dict(filter_mode="linear", boundary_mode="wrap"), w
    else:
        uv, kw, w4 = E.cube_dirs(res, torch.float64), dict(filter_mode="linear", boundary_mode="cube"), w[None]
    bound = R.g_tex_bounds(tex[None].double(), uv, w4, **kw)[0][0]
    X = R.coord_scale(uv, tex[None], kind == "cube")
    lb = 16 * R.EPS * (64.0 + X + tex.shape[-1] + 1) * float(tex.abs().max())  # (test_texture_backward_gpu.lookup_bound)
    lb = lb if kind == "ll" else lb[0]
    return t.grad.double().cpu(), t64.grad, bound, out.detach().double().cpu(), ref.detach(), lb[..., None]


BWD_CASES = [("ll", (5, 7), (3, 3), 3), ("ll", (8, 16), (2, 3), 4), ("ll", (16, 32), (8, 8), 4), ("ll", (16, 32), (7, 7), 5),
             ("ll", (64, 128), (33, 33), 1), ("cube", 4, (8, 16), 4), ("cube", 7, (16, 32), 3), ("cube", 1, (3, 5), 5), ("cube", 2, (1, 2), 1)]


@pytest.mark.parametrize("kind, src, res, C", BWD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_backward_against_float64_and_the_adjoint_identity(dev, ops, kind, src, res, C):
    g = _gen(C, *res, 7)
    tex = torch.rand(*src, C, generator=g) if kind == "ll" else torch.rand(6, src, src, C, generator=g)
    shape = (6, res[0], res[1], C) if kind == "ll" else (res[0], res[1], C)
    w = torch.rand(shape, generator=g) * 2 - 1
    if kind == "ll":  # (a pole texel's gradient lands in a column nobody defines)
        w = w * (~E.pole_mask(res))[..., None]
    g1, want, bound, out, ref, lb = _backward_case(ops, dev, kind, tex, res, w)
    err = (g1 - want).abs()
    print(f"BWD {kind} {src} {res} C{C} worst err / bound = {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
    # run to run: the float atomics may land in another order; both runs stay inside the bound, and so does their difference
    g2 = _backward_case(ops, dev, kind, tex, res, w)[0]
    assert bool(((g2 - want).abs() <= bound).all()) and bool(((g2 - g1).abs() <= bound).all())
    # <A x, y> = <x, A^T y> with A the kernel's forward and A^T its backward
    lhs, rhs = float((out * w.double()).sum()), float((tex.double() * g1).sum())
    slack = float((lb.expand(out.shape) * w.double().abs()).sum()) + float((bound * tex.double().abs()).sum())
    assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)
    assert abs(float((ref * w.double()).sum()) - float((tex.double() * want).sum())) <= 1e-9 * (1 + abs(lhs))
    # g_out = 0 gives exactly 0
    t = tex.to(dev).requires_grad_(True)
    fn = ops.latlong_to_cubemap if kind == "ll" else ops.cubemap_to_latlong
    fn(t, list(res)).backward(torch.zeros(shape, device=dev))
    assert t.grad is not None and not bool(t.grad.any())


# ------------------------------------------------------------------------------------------------ route
def test_util_routes(dev, ops, util, monkeypatch):
    """CUDA float32: one a3d_texture_fwd (and one a3d_texture_bwd) with uv == NULL; HIP_ENVMAP = False: the six dr.texture calls of the
    statements.  The two routes agree within the forward bound."""
    seen = []
    real = ops.call

    def counted(name, *args, **kw):
        seen.append((name, args[1] if name == "a3d_texture_fwd" else args[2] if name == "a3d_texture_bwd" else 0))
        return real(name, *args, **kw)

    monkeypatch.setattr(ops, "call", counted)
    tex = _latlong((16, 32), 3, 5).to(dev)
    t = tex.clone().requires_grad_(True)
    a = util.latlong_to_cubemap(t, [8, 8])
    a.sum().backward()
    assert seen == [("a3d_texture_fwd", None), ("a3d_texture_bwd", None)], seen
    assert a.device == tex.device and t.grad is not None
    del seen[:]
    monkeypatch.setattr(util, "HIP_ENVMAP", False)
    b = util.latlong_to_cubemap(tex, [8, 8])
    assert [n for n, _ in seen] == ["a3d_texture_fwd"] * 6 and all(p is not None for _, p in seen), seen
    assert float((a.detach() - b).abs().max()) <= C_LL * EPS23 * 32 * float(tex.max() - tex.min())
    cube = torch.rand(6, 4, 4, 3, generator=_gen(9), dtype=torch.float32).to(dev)
    del seen[:]
    d = util.cubemap_to_latlong(cube, [8, 16])
    assert [n for n, _ in seen] == ["a3d_texture_fwd"] and seen[0][1] is not None
    monkeypatch.setattr(util, "HIP_ENVMAP", True)
    del seen[:]
    c = util.cubemap_to_latlong(cube, [8, 16])
    assert seen == [("a3d_texture_fwd", None)]
    assert float((c - d).abs().max()) <= C_CUBE * EPS23 * 4 * float(cube.max() - cube.min())
    # float64 maps on the GPU take the statements too
    del seen[:]
    e = util.latlong_to_cubemap(tex.double(), [8, 8])
    assert e.dtype == torch.float64 and not seen
    assert float((e - a.detach().double()).abs().max()) <= C_LL * EPS23 * 32 * float(tex.max() - tex.min())


# ------------------------------------------------------------------------------------------------ end to end
def test_hdr_probe_in_light_out(dev, util, tmp_path):
    light = importlib.import_module("3danimals_amd.model.render.light")
    hdrio = importlib.import_module("3danimals_amd.hdrio")
    rng = np.random.default_rng(3)
    probe = (rng.random((16, 32, 3)) * np.exp(rng.uniform(-2, 3, (16, 32, 1)))).astype(np.float32)
    fn = str(tmp_path / "probe.hdr")
    hdrio.write_hdr(fn, probe)
    with pytest.raises(AssertionError, match="Unknown envlight extension"):
        light.load_env(str(tmp_path / "probe.exr"))
    env = light._load_env_hdr(fn, scale=0.5, res=16, device=dev)
    assert isinstance(env, light.EnvironmentLight) and tuple(env.base.shape) == (6, 16, 16, 3) and env.base.device == dev
    half = torch.from_numpy(hdrio.read_hdr(fn)) * 0.5
    assert _ratio(env.base.detach(), E.latlong_to_cubemap(half, (16, 16)), half, 32) <= C_LL
    assert len(env.specular) >= 1 and tuple(env.diffuse.shape) == (6, 16, 16, 3)
    g = _gen(12, 10)
    B, H, W = 1, 12, 10
    nrm = torch.nn.functional.normalize(torch.randn(B, H, W, 3, generator=g), dim=-1).to(dev)
    pos = (torch.rand(B, H, W, 3, generator=g) - 0.5).to(dev)
    kd, ks = torch.rand(B, H, W, 3, generator=g).to(dev), torch.rand(B, H, W, 3, generator=g).to(dev)
    view = torch.tensor([[[[0.0, 0.0, 3.0]]]], device=dev)
    col = env.shade(pos, nrm, kd, ks, view)
    assert tuple(col.shape) == (B, H, W, 3) and bool(torch.isfinite(col).all())
    out = str(tmp_path / "light.hdr")
    light.save_env_map(out, env)
    back = hdrio.read_hdr(out)
    assert back.shape == (512, 1024, 3)
    want = util.cubemap_to_latlong(env.base.detach(), [512, 1024]).cpu().numpy().astype(np.float64)
    err = want.clip(min=0) - back
    assert (err >= 0).all() and (err <= want.max(axis=-1, keepdims=True).clip(min=0) / 128).all()
