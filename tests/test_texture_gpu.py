"""dr.texture on the MI355X (csrc/texture.hip through ops.texture and the nvdiffrast shim): known answers first, then the float64
restatement of the specification (tests/texture_ref.py) for the forward and every gradient."""
import importlib
import math
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("3danimals_amd.ops")


@pytest.fixture(scope="module")
def dr():
    sys.path.insert(0, os.path.join(ROOT, "3danimals_amd", "shims"))
    return importlib.import_module("nvdiffrast.torch")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, seed, lo=0.0, hi=1.0):
    return torch.rand(shape, generator=_g(seed), dtype=torch.float64) * (hi - lo) + lo


def _grads(fn, inputs, g_out):
    """(out, [grad of each input]) of fn(*inputs) . g_out by autograd (None where an input has no grad)."""
    ins = [None if t is None else t.detach().clone().requires_grad_(True) for t in inputs]
    out = fn(*ins)
    out.backward(g_out.to(out.dtype))
    return out.detach(), [None if t is None else t.grad for t in ins]


def _close(a, b, tol, what=""):
    a, b = a.double().cpu(), b.double().cpu()
    err = float((a - b).abs().max()) if a.numel() else 0.0
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    assert err <= tol * scale, (what, err, scale)


def _centres(n, device=None):
    c = (torch.arange(n, dtype=torch.float64) + 0.5) / n
    gy, gx = torch.meshgrid(c, c, indexing="ij")
    return torch.stack([gx, gy], -1)


# ------------------------------------------------------------------------------------------------ 2-D equivalence with the torch tap
@pytest.mark.parametrize("C", [1, 3, 4, 33])
def test_2d_nearest_and_linear_equal_the_torch_tap(dev, ops, dr, C):
    B = 3
    uv = _rand((B, 17, 23, 2), 1, -1.3, 2.2).float().to(dev)
    for bt in (1, B):
        tex = _rand((bt, 13, 9, C), 2 + C).float().to(dev)
        for boundary in ("wrap", "clamp", "zero"):
            for mode in ("nearest", "linear"):
                got = ops.texture(tex, uv, filter_mode=mode, boundary_mode=boundary)
                want = dr._torch_tap(tex, uv, mode, boundary)
                assert got.shape == want.shape
                _close(got, want, 1e-6, (bt, boundary, mode))
                shim = dr.texture(tex, uv, filter_mode=mode, boundary_mode=boundary)
                assert torch.equal(shim, got)
                # gradients against the tap's autograd
                g = _rand(want.shape, 9).float().to(dev)
                _, (gt_h, gu_h) = _grads(lambda t, u: ops.texture(t, u, filter_mode=mode, boundary_mode=boundary), [tex, uv], g)
                _, (gt_t, gu_t) = _grads(lambda t, u: dr._torch_tap(t, u, mode, boundary), [tex, uv], g)
                _close(gt_h, gt_t, 1e-5, ("g_tex", bt, boundary, mode))
                if mode == "linear":
                    _close(gu_h, gu_t, 1e-4 * max(tex.shape[1:3]), ("g_uv", bt, boundary, mode))
                else:
                    assert float(gu_h.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ level identities
def test_integer_and_fractional_bias_pick_and_blend_levels(dev, ops):
    tex = _rand((1, 32, 32, 3), 3).float().to(dev)
    chain = R.mip_chain(tex.double().cpu())
    for k in range(len(chain)):
        n = chain[k].shape[1]
        uv = _centres(n)[None].float().to(dev)
        bias = torch.full((1, n, n), float(k), device=dev)
        got = ops.texture(tex, uv, mip_level_bias=bias, boundary_mode="clamp")
        _close(got, chain[k], 1e-6, ("level", k))
        if k + 1 < len(chain):
            f = 0.375
            nxt = R.texture(chain[k + 1], uv.double().cpu(), filter_mode="linear", boundary_mode="clamp")
            got = ops.texture(tex, uv, mip_level_bias=bias + f, boundary_mode="clamp")
            _close(got, (1 - f) * chain[k] + f * nxt, 1e-6, ("blend", k))
    # beyond the ends: clamped, and no bias gradient there
    uv = _rand((1, 8, 8, 2), 4).float().to(dev)
    for b, level in ((-3.0, 0), (40.0, len(chain) - 1)):
        bias = torch.full((1, 8, 8), b, device=dev, requires_grad=True)
        out = ops.texture(tex, uv, mip_level_bias=bias, boundary_mode="wrap")
        want = R.texture(chain[level], uv.double().cpu(), filter_mode="linear", boundary_mode="wrap")
        _close(out, want, 1e-6, ("clamp", b))
        out.sum().backward()
        assert float(bias.grad.abs().max()) == 0.0


def test_lod_from_uv_da(dev, ops):
    """J = s I -> level log2 s; a rotated J the same; an anisotropic J log2 sigma_max (probed through a bias that cancels it)."""
    T = 64
    tex = _rand((1, T, T, 2), 5).float().to(dev)
    chain = R.mip_chain(tex.double().cpu())
    uv = _centres(4)[None].float().to(dev)  # (texel centres of every level down to 4 x 4)
    c, s = math.cos(0.6), math.sin(0.6)
    for sigma, J in ((4.0, (4, 0, 0, 4)), (4.0, (4 * c, -4 * s, 4 * s, 4 * c)), (8.0, (8 * c, -0.5 * s, 8 * s, 0.5 * c))):
        da = torch.tensor(J, dtype=torch.float32).div(T).to(dev).expand(1, 4, 4, 4).contiguous()
        got = ops.texture(tex, uv, uv_da=da, boundary_mode="clamp")
        want = R.texture(chain[int(math.log2(sigma))], uv.double().cpu(), filter_mode="linear", boundary_mode="clamp")
        _close(got, want, 1e-5, J)
    zero = torch.zeros(1, 4, 4, 4, device=dev, requires_grad=True)  # a zero J: level 0, finite gradients
    out = ops.texture(tex, uv, uv_da=zero, boundary_mode="clamp")
    _close(out, R.texture(tex.double().cpu(), uv.double().cpu(), filter_mode="linear", boundary_mode="clamp"), 1e-6, "zero J")
    out.sum().backward()
    assert bool(torch.isfinite(zero.grad).all()) and float(zero.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ cube maps
def _cube_dirs(n, seed):
    d = torch.randn(1, n, n, 3, generator=_g(seed), dtype=torch.float64)
    return d


def test_cube_convention_scale_and_constant(dev, ops):
    S = 8
    tex = _rand((1, 6, S, S, 3), 6).float().to(dev)
    ii = (torch.arange(S, dtype=torch.float64) * 2 + 1) / S - 1
    gy, gx = torch.meshgrid(ii, ii, indexing="ij")
    for f in range(6):  # normalise(cube_to_dir(face, centre)) returns the texel (reference model/render/util.py:96-103)
        d = R.cube_to_dir(torch.full_like(gx, f, dtype=torch.long), gx, gy)
        d = (d / d.norm(dim=-1, keepdim=True))[None].float().to(dev)
        _close(ops.texture(tex, d, filter_mode="linear", boundary_mode="cube")[0], tex[0, f], 1e-6, f)
        _close(ops.texture(tex, d, filter_mode="nearest", boundary_mode="cube")[0], tex[0, f], 0, f)
    d = _cube_dirs(64, 7).float().to(dev)
    a = ops.texture(tex, d, filter_mode="linear", boundary_mode="cube")
    _close(ops.texture(tex, 3.7 * d, filter_mode="linear", boundary_mode="cube"), a, 1e-6, "scale")
    _close(a, R.texture(tex.double().cpu(), d.double().cpu(), filter_mode="linear", boundary_mode="cube"), 1e-5, "restatement")
    one = torch.full((1, 6, S, S, 2), 0.75, device=dev)
    corners = torch.tensor([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=torch.float32).view(1, 1, 8, 3).to(dev)
    for dd in (d, corners):
        _close(ops.texture(one, dd, filter_mode="linear", boundary_mode="cube"), torch.full(dd.shape[:-1] + (2,), 0.75), 1e-6, "const")
        bias = torch.full(dd.shape[:-1], 1.5, device=dev)
        _close(ops.texture(one, dd, mip_level_bias=bias, boundary_mode="cube"), torch.full(dd.shape[:-1] + (2,), 0.75), 1e-6, "const tri")


def test_cube_is_continuous_across_all_twelve_edges(dev, ops):
    S = 16
    tex = _rand((1, 6, S, S, 3), 8).float().to(dev)
    eps = 1e-4
    t = torch.linspace(-0.95, 0.95, 41, dtype=torch.float64)
    dirs_a, dirs_b = [], []
    for axis_a in range(3):
        for axis_b in range(axis_a + 1, 3):
            for sa in (-1, 1):
                for sb in (-1, 1):  # the edge where |component a| = |component b| = 1, the third running along it
                    third = 3 - axis_a - axis_b
                    base = torch.zeros(t.shape[0], 3, dtype=torch.float64)
                    base[:, axis_a], base[:, axis_b], base[:, third] = sa, sb, t
                    p, q = base.clone(), base.clone()
                    p[:, axis_a] *= 1 + eps  # just on face a
                    q[:, axis_b] *= 1 + eps  # just on face b
                    dirs_a.append(p)
                    dirs_b.append(q)
    A = torch.cat(dirs_a)[None, None].float().to(dev)
    Bd = torch.cat(dirs_b)[None, None].float().to(dev)
    for mode in ("linear", "linear-mipmap-linear"):
        kw = {} if mode == "linear" else dict(mip_level_bias=torch.full(A.shape[:-1], 0.6, device=dev))
        ya = ops.texture(tex, A, filter_mode=mode, boundary_mode="cube", **kw)
        yb = ops.texture(tex, Bd, filter_mode=mode, boundary_mode="cube", **kw)
        assert float((ya - yb).abs().max()) < 5e-3, mode  # (the two points are 1e-4 apart: a seam would be a texel-sized jump)


def test_cube_gradients_against_the_restatement(dev, ops):
    S = 16
    tex = _rand((2, 6, S, S, 3), 9).float().to(dev)
    d = _cube_dirs(12, 10).expand(2, 12, 12, 3).contiguous()
    d[1] = torch.randn(12, 12, 3, generator=_g(11), dtype=torch.float64)
    da = (torch.randn(2, 12, 12, 6, generator=_g(12), dtype=torch.float64) * 0.02)
    bias = _rand((2, 12, 12), 13, -0.5, 3.5)
    g = _rand((2, 12, 12, 3), 14, -1, 1)
    for mode in ("linear", "linear-mipmap-linear", "linear-mipmap-nearest"):
        kw = dict(filter_mode=mode, boundary_mode="cube")
        fh = lambda t, u, a, b: ops.texture(t, u, a, b, **kw)
        fr = lambda t, u, a, b: R.texture(t, u, a, b, **kw)
        args = [tex, d.float(), da.float(), bias.float()] if mode != "linear" else [tex, d.float(), None, None]
        oh, gh = _grads(fh, [a.to(dev) if a is not None else None for a in args], g.float().to(dev))
        orf, gr = _grads(fr, [a.double().cpu() if a is not None else None for a in args], g)
        _close(oh, orf, 1e-5, (mode, "out"))
        _close(gh[0], gr[0], 1e-4, (mode, "g_tex"))
        _close(gh[1], gr[1], 2e-3, (mode, "g_uv"))
        assert float((gh[1].double().cpu() * d).sum(-1).abs().max()) < 1e-3 * float(gh[1].abs().max() + 1)  # g_uv . uv = 0
        if mode == "linear-mipmap-linear":
            _close(gh[2], gr[2], 2e-3, (mode, "g_uv_da"))
            _close(gh[3], gr[3], 1e-4, (mode, "g_bias"))
        elif mode == "linear-mipmap-nearest":
            assert float(gh[2].abs().max()) == 0 and float(gh[3].abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 2-D gradients
@pytest.mark.parametrize("boundary", ["wrap", "clamp", "zero"])
def test_2d_trilinear_gradients_against_the_restatement(dev, ops, boundary):
    B, T = 2, 32
    tex = _rand((B, T, T, 4), 15)
    uv = _rand((B, 10, 12, 2), 16, -0.2, 1.2)
    da = torch.randn(B, 10, 12, 4, generator=_g(17), dtype=torch.float64) * 0.05
    bias = _rand((B, 10, 12), 18, -1.0, 1.0)
    g = _rand((B, 10, 12, 4), 19, -1, 1)
    kw = dict(filter_mode="linear-mipmap-linear", boundary_mode=boundary)
    oh, gh = _grads(lambda t, u, a, b: ops.texture(t, u, a, b, **kw), [x.float().to(dev) for x in (tex, uv, da, bias)], g.float().to(dev))
    orf, gr = _grads(lambda t, u, a, b: R.texture(t, u, a, b, **kw), [tex, uv, da, bias], g)
    _close(oh, orf, 1e-5, "out")
    _close(gh[0], gr[0], 1e-5, "g_tex (through the internal stack's box filter)")
    _close(gh[1], gr[1], 1e-3, "g_uv")
    _close(gh[2], gr[2], 2e-3, "g_uv_da")
    _close(gh[3], gr[3], 1e-4, "g_bias")
    if boundary != "zero":  # partition of unity: each channel's g_tex over all levels sums to that of g_out
        _close(gh[0].double().sum((0, 1, 2)).cpu(), g.sum((0, 1, 2)), 1e-5, "unity")


def test_partition_of_unity_over_a_custom_stack_and_nearest(dev, ops):
    tex = _rand((1, 16, 16, 3), 20).float().to(dev).requires_grad_(True)
    mips = [_rand((1, 16 >> k, 16 >> k, 3), 20 + k).float().to(dev).requires_grad_(True) for k in range(1, 5)]
    uv = _rand((2, 20, 20, 2), 25, -1, 2).float().to(dev)
    bias = _rand((2, 20, 20), 26, -1, 5).float().to(dev)
    g = _rand((2, 20, 20, 3), 27, -1, 1).float().to(dev)
    for boundary in ("wrap", "clamp"):
        for t in [tex] + mips:
            t.grad = None
        ops.texture(tex, uv, mip_level_bias=bias, mip=mips, boundary_mode=boundary).backward(g)
        total = sum(t.grad.double().sum((0, 1, 2)) for t in [tex] + mips)
        _close(total, g.double().sum((0, 1, 2)), 1e-5, boundary)
        assert all(float(t.grad.abs().sum()) > 0 for t in [tex] + mips[:2])
    u = uv.clone().requires_grad_(True)
    ops.texture(tex, u, filter_mode="nearest").backward(g)
    assert float(u.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ reference-shaped calls
def test_texture2d_sample_pattern(dev, dr):
    """Texture2D.sample (reference model/render/texture.py:67-75): an avg-pooled parameter stack, uv_da, linear-mipmap-linear."""
    base = _rand((1, 64, 32, 3), 30)
    mips = [base]
    while mips[-1].shape[1] > 1 and mips[-1].shape[2] > 1:
        mips.append(R.box_down(mips[-1]))
    uv = _rand((2, 16, 16, 2), 31)
    da = torch.randn(2, 16, 16, 4, generator=_g(32), dtype=torch.float64) * 0.03
    g = _rand((2, 16, 16, 3), 33, -1, 1)
    ins = [m.float().to(dev) for m in mips] + [uv.float().to(dev), da.float().to(dev)]
    oh, gh = _grads(lambda *a: dr.texture(a[0], a[-2], a[-1], mip=list(a[1:-2]), filter_mode="linear-mipmap-linear"), ins, g.float().to(dev))
    orf, gr = _grads(lambda *a: R.texture(a[0], a[-2], a[-1], mip=list(a[1:-2]), filter_mode="linear-mipmap-linear"), mips + [uv, da], g)
    _close(oh, orf, 1e-5, "out")
    for k, (a, b) in enumerate(zip(gh, gr)):
        _close(a, b, 2e-3 if k >= len(mips) else 1e-5, k)


def test_environment_light_shade_pattern(dev, dr):
    """EnvironmentLight.shade (reference light.py:109-122): cube diffuse (linear), the FG table (2-D clamp), and the biased trilinear
    specular lookup over a [None]-batched level list."""
    S = 32
    spec = [_rand((6, S >> k, S >> k, 3), 40 + k) for k in range(3)]  # 32, 16, 8
    diffuse = _rand((6, 8, 8, 3), 45)
    lut = _rand((1, 16, 16, 2), 46)
    n = torch.randn(2, 12, 12, 3, generator=_g(47), dtype=torch.float64)
    r = torch.randn(2, 12, 12, 3, generator=_g(48), dtype=torch.float64)
    fg_uv = _rand((2, 12, 12, 2), 49)
    lvl = _rand((2, 12, 12), 50, 0, 2)
    g = _rand((2, 12, 12, 3), 51, -1, 1)
    g2 = _rand((2, 12, 12, 2), 52, -1, 1)

    def run(mod, d_, n_, r_, l_, u_, lv_, *sp):
        if mod is R:
            f = lambda *a, **k: R.texture(*a, **k)
        else:
            f = dr.texture
        dif = f(d_[None], n_, filter_mode="linear", boundary_mode="cube")
        fg = f(l_, u_, filter_mode="linear", boundary_mode="clamp")
        sp_ = f(sp[0][None], r_, mip=[m[None] for m in sp[1:]], mip_level_bias=lv_, filter_mode="linear-mipmap-linear", boundary_mode="cube")
        return dif, fg, sp_

    ins_r = [diffuse, n, r, lut, fg_uv, lvl] + spec
    ins_h = [x.float().to(dev).requires_grad_(True) for x in ins_r]
    ins_r = [x.clone().requires_grad_(True) for x in ins_r]
    oh = run(dr, *ins_h)
    orf = run(R, *ins_r)
    for a, b in zip(oh, orf):
        _close(a, b, 1e-5, "out")
    (oh[0] * g.float().to(dev)).sum().add((oh[1] * g2.float().to(dev)).sum()).add((oh[2] * g.float().to(dev)).sum()).backward()
    ((orf[0] * g).sum() + (orf[1] * g2).sum() + (orf[2] * g).sum()).backward()
    for k, (a, b) in enumerate(zip(ins_h, ins_r)):
        _close(a.grad, b.grad, 2e-3 if k in (1, 2, 4) else 1e-4, k)


def test_cubemap_mip_backward_tap(dev, dr):
    """cubemap_mip.backward (reference light.py:31-41): dout * 0.25 sampled at every texel direction of the finer level."""
    res = 16
    dout = _rand((6, res // 2, res // 2, 3), 60)
    ii = torch.linspace(-1.0 + 1.0 / res, 1.0 - 1.0 / res, res, dtype=torch.float64)
    gy, gx = torch.meshgrid(ii, ii, indexing="ij")
    for s in range(6):
        v = R.cube_to_dir(torch.full_like(gx, s, dtype=torch.long), gx, gy)
        v = v / v.norm(dim=-1, keepdim=True)
        g = _rand((1, res, res, 3), 61 + s, -1, 1)
        oh, gh = _grads(lambda t, u: dr.texture(t[None] * 0.25, u[None].contiguous(), filter_mode="linear", boundary_mode="cube"),
                        [dout.float().to(dev), v.float().to(dev)], g.float().to(dev))
        orf, gr = _grads(lambda t, u: R.texture(t[None] * 0.25, u[None], filter_mode="linear", boundary_mode="cube"), [dout, v], g)
        _close(oh, orf, 1e-6, s)
        _close(gh[0], gr[0], 1e-5, s)
        _close(gh[1], gr[1], 1e-3, s)


def test_construct_mip_equals_the_internal_stack(dev, dr, ops):
    tex = _rand((1, 6, 16, 16, 4), 70).float().to(dev)
    stack = dr.texture_construct_mip(tex, cube_mode=True)
    chain = R.mip_chain(tex.double().cpu())
    assert len(stack.levels) == len(chain) - 1
    for a, b in zip(stack.levels, chain[1:]):
        _close(a, b, 1e-6)
    d = _cube_dirs(8, 71).float().to(dev)
    bias = _rand((1, 8, 8), 72, 0, 4).float().to(dev)
    a = dr.texture(tex, d, mip=stack, mip_level_bias=bias, boundary_mode="cube")
    b = ops.texture(tex, d, mip_level_bias=bias, boundary_mode="cube")
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ robustness
def test_large_noncontiguous_and_reproducible(dev, ops, dr):
    B, H, W = 16, 512, 512
    tex = torch.rand(1, 256, 256, 3, device=dev)
    uv = torch.rand(B, H, W, 2, device=dev) * 1.5 - 0.25
    out = ops.texture(tex, uv, filter_mode="linear", boundary_mode="wrap")
    _close(out, dr._torch_tap(tex, uv, "linear", "wrap"), 1e-6, "large")
    assert torch.equal(out, ops.texture(tex, uv, filter_mode="linear", boundary_mode="wrap"))
    # non-contiguous inputs: a transposed uv, a channel slice of the texture
    uvt = uv[:2, :64, :64].transpose(1, 2)
    texs = torch.rand(1, 64, 64, 5, device=dev)[..., 1:4]
    _close(ops.texture(texs, uvt, boundary_mode="clamp"), dr._torch_tap(texs.contiguous(), uvt.contiguous(), "linear", "clamp"), 1e-6, "noncontig")
    # trilinear: bitwise reproducible forward, backward within 1e-6 relative
    da = torch.randn(4, 128, 128, 4, device=dev) * 0.01
    uv4 = uv[:4, :128, :128].contiguous()
    t2 = torch.rand(1, 512, 512, 4, device=dev)
    runs = []
    for _ in range(2):
        t = t2.clone().requires_grad_(True)
        u = uv4.clone().requires_grad_(True)
        o = ops.texture(t, u, uv_da=da)
        o.backward(torch.ones_like(o))
        runs.append((o.detach(), t.grad, u.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    _close(runs[0][1], runs[1][1], 1e-6, "g_tex reproducible")
