"""Environment light on the GPU (csrc/envlight.hip, ops.diffuse_cubemap / specular_bounds / specular_cubemap_raw, renderutils, light.py,
render.shade) against the float64 restatement tests/envlight_ref.py.

Bounds of the value tests: R.specular_terms / R.diffuse_terms derive a per-output fp32 bound from the operation count of one pair, the
conditioning of D in t and the length of the sum (the derivation is written next to C_DIR / C_DOT / C_T there); pairs whose dot lies
within R.D_AMBIGUOUS = 4e-6 of the cutoff may fall on either side, so their |w x| is added -- only where such outputs are at most 5 %
of the map; cases that pass an explicit cutoff must have none."""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import envlight_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROUGHNESS = (0.08, 0.22, 0.36, 0.5, 1.0)


def _mods():
    return (importlib.import_module("3danimals_amd.ops"), importlib.import_module("3danimals_amd.model.render.renderutils"),
            importlib.import_module("3danimals_amd.model.render.light"))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _maps(N, seed):
    """random in [0, 4]; one hot texel at a face centre, an edge and a corner (windows across one, two and three faces)."""
    g = _gen(seed)
    yield "random", torch.rand(6, N, N, 3, generator=g, dtype=torch.float64) * 4
    for name, (f, y, x) in (("centre", (4, N // 2, N // 2)), ("edge", (0, N // 2, N - 1)), ("corner", (2, 0, 0))):
        m = torch.zeros(6, N, N, 3, dtype=torch.float64)
        m[f, y, x] = torch.tensor([3.0, 1.0, 2.0], dtype=torch.float64)
        yield name, m


def _check(got, want, bound, amb, what):
    err = (got.double().cpu() - want).abs()
    lim = bound + amb
    print(f"{what}: max err {float(err.max()):.3e}, max err / bound {float((err / lim.clamp(min=1e-300)).max()):.3f}, max |value| {float(want.abs().max()):.3e}")
    assert bool((err <= lim).all()), (what, float((err - lim).max()))


@pytest.mark.parametrize("N", [1, 2, 5, 8, 16, 32])
def test_bounds_table_is_between_the_two_float64_boxes(N):
    ops, _, _ = _mods()
    for c in [R.cutoff_cosine(r) for r in ROUGHNESS] + [0.7071, -1.0]:
        got = ops.specular_bounds(N, c, "cuda")
        assert got.dtype == torch.int16 and tuple(got.shape) == (6, N, N, 6, 4)
        got = got.cpu().long().reshape(-1, 6, 4)
        inner, outer = R.boxes(N, c + R.D_AMBIGUOUS), R.boxes(N, c - R.D_AMBIGUOUS)
        lo, hi = [0, 2], [1, 3]
        assert bool((got[..., lo] <= inner[..., lo]).all() and (got[..., hi] >= inner[..., hi]).all()), (N, c, "misses a texel inside the cone")
        assert bool((got[..., lo] >= outer[..., lo]).all() and (got[..., hi] <= outer[..., hi]).all()), (N, c, "holds a texel outside the cone")
        empty = (outer[..., 0] > outer[..., 1]) if N > 1 else torch.zeros(6, 6, dtype=torch.bool)
        assert bool((got[empty] == torch.tensor([N - 1, 0, N - 1, 0])).all())


@pytest.mark.parametrize("N", [1, 2, 5, 8, 12, 16])
def test_diffuse_forward_backward_and_adjoint(N):
    ops, _, _ = _mods()
    for name, x in _maps(N, 100 + N):
        xg = x.float().cuda().requires_grad_(True)
        out = ops.diffuse_cubemap(xg)
        want, bound = R.diffuse_terms(x.float().double())
        _check(out.detach(), want, bound, 0, f"diffuse fwd N={N} {name}")
        go = torch.randn(6, N, N, 3, generator=_gen(7), dtype=torch.float64).float()
        gi, = torch.autograd.grad(out, xg, go.cuda())
        gwant, gbound = R.diffuse_terms(go.double(), transpose=True)
        _check(gi, gwant, gbound, 0, f"diffuse bwd N={N} {name}")
        gi2, = torch.autograd.grad(ops.diffuse_cubemap(xg), xg, go.cuda())
        assert torch.equal(gi, gi2)
        lhs, rhs = float((go.double() * out.detach().double().cpu()).sum()), float((gi.double().cpu() * x.float().double()).sum())
        assert abs(lhs - rhs) <= float((go.double().abs() * bound).sum() + (x.abs() * gbound).sum()), (lhs, rhs)


@pytest.mark.parametrize("N,roughness", [(16, r) for r in ROUGHNESS] + [(32, r) for r in ROUGHNESS] + [(12, r) for r in ROUGHNESS]
                         + [(8, 0.08), (8, 0.22), (8, 0.36), (8, 1.0), (5, 0.22), (5, 0.5), (1, 0.5), (2, 0.36), (2, 1.0)])
def test_specular_forward_backward_adjoint_and_reproducibility(N, roughness):
    """Every map of _maps (random, hot centre / edge / corner texel) at every size; N = 12 walks the partial 8 x 8 tiles of the kernel.
    The restatement's dense pair terms are computed once per (N, roughness) for all maps (their channels side by side).  Besides the raw
    sums, the quotient colour / weight is held to R.specular_mean_terms: there D's conditioning cancels, so at roughness 0.08 -- where
    the raw bound is loose -- the colours are checked to a few 1e-6."""
    ops, _, _ = _mods()
    c = R.cutoff_cosine(roughness)
    bounds = ops.specular_bounds(N, c, "cuda")
    maps = [(name, x.float().double()) for name, x in _maps(N, 200 + N)]
    one = torch.ones(6, N, N, 1, dtype=torch.float64)
    want_all, bound_all, amb_all, amb_any = R.specular_terms(torch.cat([x for _, x in maps] + [one], -1), roughness, c)
    assert int(amb_any.sum()) <= 0.05 * 6 * N * N, (N, roughness, int(amb_any.sum()))  # (the ambiguous term is a condition, not a loophole)
    mean_all, mbound_all, _ = R.specular_mean_terms(torch.cat([x for _, x in maps], -1), roughness, c)
    go = torch.randn(6, N, N, 4, generator=_gen(9), dtype=torch.float64).float()  # (channel 3 non-zero: it must be ignored)
    gwant, gbound, gamb, _ = R.specular_terms(go[..., :3].double(), roughness, c, transpose=True)
    for i, (name, x) in enumerate(maps):
        pick = lambda t: torch.cat((t[..., 3 * i:3 * i + 3], t[..., -1:]), -1)
        want, bound, amb = pick(want_all), pick(bound_all), pick(amb_all)
        xg = x.float().cuda().requires_grad_(True)
        out = ops.specular_cubemap_raw(xg, roughness, c, bounds)
        assert tuple(out.shape) == (6, N, N, 4)
        _check(out.detach(), want, bound, amb, f"specular fwd N={N} r={roughness} {name}")
        quot = (out.detach()[..., :3] / out.detach()[..., 3:]).double().cpu()
        merr, mb = (quot - mean_all[..., 3 * i:3 * i + 3]).abs(), mbound_all[..., 3 * i:3 * i + 3]
        print(f"colour / weight N={N} r={roughness} {name}: max err {float(merr.max()):.3e}, largest finite bound {float(mb[torch.isfinite(mb)].max()):.3e}")
        assert bool((merr <= mb).all()), (name, float((merr - mb).max()))
        gi, = torch.autograd.grad(out, xg, go.cuda())
        _check(gi, gwant, gbound, gamb, f"specular bwd N={N} r={roughness} {name}")
        gi2, = torch.autograd.grad(ops.specular_cubemap_raw(xg, roughness, c, bounds), xg, go.cuda())
        assert torch.equal(gi, gi2)  # a gather: reproducible run to run
        lhs = float((go[..., :3].double() * out.detach()[..., :3].double().cpu()).sum())
        rhs = float((gi.double().cpu() * x).sum())
        slack = float((go[..., :3].double().abs() * (bound + amb)[..., :3]).sum() + (x.abs() * (gbound + gamb)).sum())
        assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)


def test_explicit_clean_cutoff_and_everything_cutoff():
    """An explicit cutoff: 0.7071 at N = 16 is ambiguity-free (asserted); -1 keeps every texel with a positive dot."""
    ops, _, _ = _mods()
    N = 16
    x = torch.rand(6, N, N, 3, generator=_gen(5), dtype=torch.float64).float().double() * 4
    x4 = torch.cat((x, torch.ones(6, N, N, 1, dtype=torch.float64)), -1)
    want, bound, amb, amb_any = R.specular_terms(x4, 0.36, 0.7071)
    assert int(amb_any.sum()) == 0
    got = ops.specular_cubemap_raw(x.float().cuda(), 0.36, 0.7071, ops.specular_bounds(N, 0.7071, "cuda"))
    _check(got, want, bound, 0, "specular fwd explicit cutoff 0.7071")
    want, bound, amb, _ = R.specular_terms(x4, 1.0, -1.0)  # (the ambiguous pairs are the antipodes: their weight is 0)
    assert float(amb.max()) == 0
    got = ops.specular_cubemap_raw(x.float().cuda(), 1.0, -1.0, ops.specular_bounds(N, -1.0, "cuda"))
    _check(got, want, bound, 0, "specular fwd cutoff -1")


def test_public_api_composes_the_raw_ops_and_caches_the_table():
    ops, ru, _ = _mods()
    ru_ops = importlib.import_module("3danimals_amd.model.render.renderutils.ops")
    x = (torch.rand(6, 16, 16, 3, generator=_gen(1)) * 4).cuda()
    c, table = ru_ops.specular_bounds(16, 0.36, 0.99, x.device)
    assert c == R.cutoff_cosine(0.36) and ru_ops.specular_bounds(16, 0.36, 0.99, x.device)[1] is table
    raw = ops.specular_cubemap_raw(x, 0.36, c, table)
    assert torch.equal(ru.specular_cubemap(x, 0.36), raw[..., :3] / raw[..., 3:])
    assert torch.equal(ru.specular_cubemap(x, 0.36, cutoff=0.99, use_python=True), raw[..., :3] / raw[..., 3:])
    assert torch.equal(ru.diffuse_cubemap(x), ops.diffuse_cubemap(x))
    assert torch.equal(table, ops.specular_bounds(16, c, "cuda"))


def _gbuffers(seed, B=2, H=12, W=10):
    g = _gen(seed)
    pos = torch.randn(B, H, W, 3, generator=g, dtype=torch.float64) * 0.3
    n = torch.randn(B, H, W, 3, generator=g, dtype=torch.float64)
    n = n / n.norm(dim=-1, keepdim=True)
    kd = torch.rand(B, H, W, 3, generator=g, dtype=torch.float64)
    ks = torch.rand(B, H, W, 3, generator=g, dtype=torch.float64)
    view = torch.tensor([0.3, 0.2, 2.5], dtype=torch.float64).expand(B, H, W, 3).contiguous()
    return [t.float().double() for t in (pos, n, kd, ks, view)]


def test_environment_light_end_to_end():
    """create_trainable_env_rnd(64) -> build_mips (3 specular levels 64 / 32 / 16 + diffuse) -> shade, values and gradients against the
    restatement chain.  Tolerance of EVERY chained comparison (levels, d loss / d env_base, shade values, shade gradients): the
    restatement chain is run in float32 on the CPU, with autograd, on these inputs at test time; its largest deviation from float64 is
    taken per tensor (printed; e.g. 1.0e-3 on level 0, roughness 0.08: D's conditioning; 3e-7 .. 4e-4 of the largest magnitude on the
    shade gradients) and the GPU is allowed FOUR times that (other summation order, fma contraction) -- and never less than four
    float32 roundings (4 * 2^-22) of the tensor's largest magnitude, the resolution of the comparison itself."""
    ops, ru, light = _mods()
    render = importlib.import_module("3danimals_amd.model.render.render")
    torch.manual_seed(0)
    lgt = light.create_trainable_env_rnd(64)
    lgt.build_mips()
    assert [s.shape[1] for s in lgt.specular] == [64, 32, 16] and tuple(lgt.diffuse.shape) == (6, 16, 16, 3)
    base = lgt.base.detach().cpu().double().requires_grad_(True)
    spec, diff = R.build_mips(base)
    with torch.no_grad():
        s32, d32 = R.build_mips(base.detach().float())

    def tol(a32, a64):
        return 4 * max(float((a32.double() - a64).abs().max()), 2.0 ** -22 * float(a64.abs().max()))

    for i, (got, w32, want) in enumerate(zip(lgt.specular + [lgt.diffuse], s32 + [d32], spec + [diff])):
        err = float((got.detach().cpu().double() - want).abs().max())
        print(f"level {i}: GPU err {err:.3e}, float32 restatement err {float((w32.double() - want).abs().max()):.3e}, allowed {tol(w32, want.detach()):.3e}")
        assert err <= tol(w32, want.detach()), i
    # d loss / d env_base through the whole chain
    gs = [torch.randn(s.shape, generator=_gen(20 + i), dtype=torch.float64).float().double() for i, s in enumerate(spec + [diff])]
    loss64 = sum((g * s).sum() for g, s in zip(gs, spec + [diff]))
    g64, = torch.autograd.grad(loss64, base, retain_graph=True)
    b32 = base.detach().float().requires_grad_(True)
    sp32, df32 = R.build_mips(b32)
    g32, = torch.autograd.grad(sum((g.float() * s).sum() for g, s in zip(gs, sp32 + [df32])), b32, retain_graph=True)
    loss = sum((g.float().cuda() * s).sum() for g, s in zip(gs, lgt.specular + [lgt.diffuse]))
    ggot, = torch.autograd.grad(loss, lgt.base, retain_graph=True)
    err = float((ggot.cpu().double() - g64).abs().max())
    print(f"d loss / d env_base: GPU err {err:.3e}, float32 restatement err {float((g32.double() - g64).abs().max()):.3e}, allowed {tol(g32, g64):.3e}")
    assert err <= tol(g32, g64)
    # shade, with and without the specular term, rotated lookups included
    fg64 = R.fg_table()
    fg_got = light._fg_lut(lgt.base.device)
    # (evaluated in float64 on the device and rounded to float32 once: one rounding of values <= 1, 2^-24, doubled for the device's own libm)
    assert float((fg_got.cpu().double() - fg64).abs().max()) <= 2.0 ** -23 and float(fg_got.min()) >= 0 and float(fg_got.sum(-1).max()) <= 1 + 2.0 ** -22
    rot = torch.tensor([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    for specular, mtx in ((False, None), (True, None), (True, rot)):
        leaves64 = [t.clone().requires_grad_(True) for t in _gbuffers(3)[:4]]
        view = _gbuffers(3)[4]
        leaves_gpu = [t.detach().float().cuda().requires_grad_(True) for t in leaves64]
        lgt.xfm(None if mtx is None else mtx[None].cuda())
        got = lgt.shade(leaves_gpu[0], leaves_gpu[1], leaves_gpu[2], leaves_gpu[3], view.float().cuda(), specular=specular)
        want = R.shade(spec, diff, fg64, leaves64[0], leaves64[1], leaves64[2], leaves64[3], view, specular=specular,
                       mtx=None if mtx is None else mtx.double())
        leaves32 = [t.detach().float().requires_grad_(True) for t in leaves64]  # the float32 chain, from b32 on, with autograd
        w32 = R.shade(sp32, df32, fg64.float(), *leaves32, view.float(), specular=specular, mtx=mtx)
        err = float((got.detach().cpu().double() - want).abs().max())
        print(f"shade specular={specular} xfm={mtx is not None}: GPU err {err:.3e}, allowed {tol(w32.detach(), want.detach()):.3e}")
        assert err <= tol(w32.detach(), want.detach())
        go = torch.randn(want.shape, generator=_gen(4), dtype=torch.float64).float().double()
        grads64 = torch.autograd.grad((want * go).sum(), [base, leaves64[2], leaves64[3], leaves64[1]], retain_graph=True)
        grads32 = torch.autograd.grad((w32 * go.float()).sum(), [b32, leaves32[2], leaves32[3], leaves32[1]], retain_graph=True)
        grads = torch.autograd.grad((got * go.float().cuda()).sum(), [lgt.base, leaves_gpu[2], leaves_gpu[3], leaves_gpu[1]], retain_graph=True)
        for nm, a, b32_, b in zip(("env_base", "kd", "ks", "gb_normal"), grads, grads32, grads64):
            e = float((a.cpu().double() - b).abs().max())
            print(f"  g_{nm}: GPU err {e:.3e}, float32 restatement err {float((b32_.double() - b).abs().max()):.3e}, allowed {tol(b32_, b):.3e}, "
                  f"max |g| {float(b.abs().max()):.3e}")
            assert e <= tol(b32_, b), (nm, specular, mtx is not None)
    lgt.xfm(None)
    # render.shade: an environment light goes through lgt.shade where it used to raise
    pos, n, kd, ks, view = [t.float().cuda() for t in _gbuffers(3)]

    class Mat:
        bsdf = None

        def sample(self, p, feat=None):
            return torch.cat((kd, ks, torch.zeros_like(kd)), -1)

    w2c = torch.eye(4, device="cuda")[None].expand(2, 4, 4)
    for bsdf in ("pbr", "diffuse"):
        out = render.shade(pos, n, n, None, pos, w2c, view, lgt, Mat(), bsdf, two_sided_shading=False)["shaded"]
        nn = ru.prepare_shading_normal(pos, view, None, n, None, n, two_sided_shading=False, opengl=True, use_python=True)
        assert torch.equal(out[..., :3], lgt.shade(pos, nn, kd, ks, view, specular=bsdf == "pbr")) and bool((out[..., 3] == 1).all())


def test_covered_point_list_path_matches_the_dense_path():
    """render.shade(..., cover=mask) -- the point-list route render_layer / render_mesh take (_shade_covered -> _shade_points) -- with an
    EnvironmentLight, bsdf 'diffuse' and 'pbr', with and without a [1,4,4] lookup transform: the covered pixels carry what the dense
    route computes there (the same per-point arithmetic on another layout: a few float32 roundings are allowed, 4 * 2^-22 of the
    largest value), everything else is 0 with alpha 0; a per-image transform is refused on the one-image point list."""
    ops, ru, light = _mods()
    render = importlib.import_module("3danimals_amd.model.render.render")
    torch.manual_seed(2)
    lgt = light.create_trainable_env_rnd(64)  # (the smallest base the reference's roughness ladder divides: three levels)
    lgt.build_mips()
    pos, n, _, _, _ = [t.float().cuda() for t in _gbuffers(6, B=2, H=16, W=16)]
    view = torch.tensor([[0.3, 0.2, 2.5], [-0.4, 0.1, 2.0]], device="cuda").reshape(2, 1, 1, 3)
    cover = torch.rand(2, 16, 16, generator=_gen(8)).cuda() < 0.6

    class Mat:
        bsdf = None

        def sample(self, p, feat=None):
            return torch.cat((0.5 + 0.4 * torch.sin(3 * p), 0.5 + 0.4 * torch.cos(2 * p), torch.zeros_like(p)), -1)

    w2c = torch.eye(4, device="cuda")[None].expand(2, 4, 4).contiguous()
    rot = torch.tensor([[[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]], device="cuda")
    for bsdf in ("diffuse", "pbr"):
        for mtx in (None, rot):
            lgt.xfm(mtx)
            dense = render.shade(pos, n, n, None, pos, w2c, view, lgt, Mat(), bsdf)["shaded"]
            sparse = render.shade(pos, n, n, None, pos, w2c, view, lgt, Mat(), bsdf, cover=cover)["shaded"]
            assert tuple(sparse.shape) == (2, 16, 16, 4)
            diff = float((sparse[cover][:, :3] - dense[cover][:, :3]).abs().max())
            print(f"covered vs dense, bsdf={bsdf} xfm={mtx is not None}: max diff {diff:.3e}, max value {float(dense.abs().max()):.3e}")
            assert diff <= 4 * 2.0 ** -22 * float(dense[..., :3].abs().max())
            assert bool((sparse[cover][:, 3] == 1).all()) and bool((sparse[~cover] == 0).all())
    lgt.xfm(rot.expand(2, 4, 4))
    assert torch.equal(render.shade(pos, n, n, None, pos, w2c, view, lgt, Mat(), "pbr")["shaded"][..., 3], torch.ones(2, 16, 16, device="cuda"))
    with pytest.raises(ValueError, match="lookup transform"):
        render.shade(pos, n, n, None, pos, w2c, view, lgt, Mat(), "pbr", cover=cover)


def test_diffuse_refuses_maps_it_would_take_minutes_to_filter():
    ops, _, _ = _mods()
    with pytest.raises(ValueError, match="above the supported 256"):
        ops.diffuse_cubemap(torch.zeros(6, 512, 512, 3, device="cuda"))


def test_guard_mode_over_build_mips():
    """A3D_GUARD level 2 (canaries around every buffer, NaN-poisoned payloads) over one build_mips forward + backward at base 64."""
    L = importlib.import_module("3danimals_amd._lib")
    ops, ru, light = _mods()
    prev = L.set_guard(2)
    try:
        before = L.guard_stats["checks"]
        torch.manual_seed(1)
        lgt = light.create_trainable_env_rnd(64)
        lgt.build_mips()
        loss = sum((s * s).sum() for s in lgt.specular) + (lgt.diffuse * lgt.diffuse).sum()
        loss.backward()
        assert L.guard_stats["checks"] > before
        assert bool(torch.isfinite(lgt.base.grad).all()) and all(bool(torch.isfinite(s).all()) for s in lgt.specular + [lgt.diffuse])
    finally:
        L.set_guard(prev)
