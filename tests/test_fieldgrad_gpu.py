"""The eikonal regulariser's hand-written route on the GPU -- a3d_gemm_nt_relumask, a3d_harmonic_embed_jvp, a3d_field_grad_head_fwd / _bwd
through their ops wrappers, the value / gradient / adjoint chain hostnets builds from them, and DMTetGeometry with the route on against
off -- against the float64 statements of tests/fieldgrad_ref.py.  The statistic is fieldnet_ref's, |got - ref64| / (eps32 (sum |terms| +
|ref64|)); every bar is 4 x what the float32 CPU formulation of the same inputs reaches (for the embedding's tangent: the float32 torch
expression on this GPU, as for the embedding itself), measured against the reference and never against the kernels.  Masks are
threshold_backward's bit for bit, every output has the same bits on a second run, guard mode finds no canary touched on ragged M.

Each test prints its figures (FIG lines) before it asserts.

Measured on MI355X (largest ratio of a statistic to the float32 evaluation's figure; the bar is 4):
    NT GEMM 1.37 (M = 1000, K = 256)    split-K weight gradient 1.17 (M = 31, 52 columns)    head 1.00    embedding tangent 1.00
    chain  y 1.08  out 1.42  b 2.05  g_x 1.71  g_in 1.99  g_head 1.09  g_hidden 1.45  |  adjoint  dW_in 2.13  dW_l 1.71  dw_h 2.20  ds 1.58
    network, route on / off error against the float64 twin:  g_x 1.02, parameter gradients 0.41 .. 0.97, first bias 0 on both
Nothing exceeded the bar."""
import copy
import importlib
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fieldgrad_ref as G  # noqa: E402

F = G.F
pytestmark = pytest.mark.gpu


def _ops():
    return importlib.import_module("3danimals_amd.ops")


def _L():
    return importlib.import_module("3danimals_amd._lib")


def _hostnets():
    return importlib.import_module("3danimals_amd.hostnets")


def _bits(t):
    return t.view(torch.int32)


def _fig(what, value, floor):
    print(f"FIG {what} stat={value:.6g} floor={floor:.6g} ratio={value / floor if floor else 0.0:.3f}")


# ------------------------------------------------------------------------------------------------------------------ the NT GEMM
def _nt(inp, masked):
    return _ops().gemm_nt_relumask(inp["a"].cuda(), inp["w"].cuda(), inp["x"].cuda() if masked else None)


@pytest.mark.parametrize("k", G.GEMM_K)
def test_nt_gemm_against_float64(k):
    for m in G.GEMM_ROWS:
        inp = G.make_nt_inputs(m, k)
        assert F.has_the_special_values(inp["x"])
        plain = _nt(inp, False)
        for masked, got in ((False, plain), (True, _nt(inp, True))):
            v = F.check_gemm(got.cpu(), inp, masked, G.MARGIN * G.nt_floor(m), f"nt gemm M={m} K={k} masked={masked}")
            _fig(f"nt_gemm M={m} K={k} masked={masked}", v, G.nt_floor(m))
            assert torch.equal(_bits(got), _bits(_nt(inp, masked)))  # the same bits on a second run
            if masked:  # threshold_backward of the plain product, bit for bit: the denormal passes; 0.0, -0.0 and -1.5 do not
                assert torch.equal(_bits(got), _bits(torch.ops.aten.threshold_backward(plain, inp["x"].cuda(), 0)))
                assert got[0, 2] != 0 and got[m - 1, 132] != 0 and not got[0, :2].any() and got[0, 3] == 0 and got[m - 1, 131] == 0


def test_nt_gemm_keeps_non_finite_rows_to_themselves():
    """An infinity and a NaN in two rows of A: their masked entries are +0.0 (a select), every other row keeps its bits."""
    for m, k in ((33, 52), (129, 256)):
        inp = G.make_nt_inputs(m, k)
        dirty = dict(inp, a=F.with_nonfinite_rows(inp["a"]))
        bad = [r for r in F.nonfinite_rows(m) if r is not None]
        keep = torch.ones(m, dtype=torch.bool)
        keep[bad] = False
        clean, got = _nt(inp, True).cpu(), _nt(dirty, True).cpu()
        assert torch.equal(_bits(got[keep]), _bits(clean[keep]))
        passes = inp["x"][bad] > 0
        assert not bool(torch.isfinite(got[bad][passes]).any()) and bool((_bits(got[bad])[~passes] == 0).all())


@pytest.mark.parametrize("m,batch,c", G.TN_CASES)
def test_tn_splitk_against_float64(m, batch, c):
    """The weight-gradient product: below one chunk, ragged chunks, splits that get no row, several layers, the in_layer's 52 columns."""
    ops = _ops()
    p, q = G.make_tn_inputs(m, batch, c)
    got = ops.gemm_tn_splitk(p.cuda(), q.cuda())
    floor = G.tn_floor(m)
    _fig(f"tn_splitk M={m} B={batch} C={c}", F.within(F.statistic(got.cpu(), *G.tn_ref(p, q)), G.MARGIN * floor, f"tn_splitk M={m} B={batch} C={c}"), floor)
    assert torch.equal(_bits(got), _bits(ops.gemm_tn_splitk(p.cuda(), q.cuda())))  # the same bits on a second run


# ------------------------------------------------------------------------------------------------------------------ the embedding's tangent
def _jvp_float32(x, lam, freq, symmetrize):
    """The torch expression in float32 on x's device (the device's own sin / cos on both sides of the comparison)."""
    sgn = torch.ones_like(x)
    xs = x.clone()
    if symmetrize:
        sgn[:, 0] = torch.sign(x[:, 0])
        xs[:, 0] = xs[:, 0].abs()
    ang = xs[:, :, None] * freq
    l = (lam * sgn)[:, :, None]
    m = x.shape[0]
    return torch.cat([lam * sgn, (l * (freq * ang.cos())).reshape(m, -1), (-(l * (freq * ang.sin()))).reshape(m, -1), torch.zeros_like(x[:, :1])], -1)


@pytest.mark.parametrize("n", G.JVP_N)
def test_embed_jvp_against_float64(n):
    ops = _ops()
    freq = F.embed_freq(n)
    for m, symmetrize in itertools.product(G.GEMM_ROWS, (False, True)):
        x, gen = F.make_embed_inputs(n, m)  # zeros of both signs and denormals in x_0, huge arguments, the zeros of sin
        lam = torch.randn(m, 3, generator=gen)
        ref = G.embed_jvp(lam, x, freq, symmetrize, angle32=True)
        got = ops.harmonic_embed_jvp(x.cuda(), lam.cuda(), freq.cuda(), symmetrize, True)
        floor = F.statistic(_jvp_float32(x.cuda(), lam.cuda(), freq.cuda(), symmetrize).cpu(), ref, ref.abs())
        v = F.within(F.statistic(got.cpu(), ref, ref.abs()), G.MARGIN * floor, f"embed jvp n={n} M={m} symmetrize={symmetrize}")
        _fig(f"embed_jvp n={n} M={m} sym={symmetrize}", v, floor)
        got = got.cpu()
        assert not got[:, -1].any() and torch.equal(_bits(got), _bits(ops.harmonic_embed_jvp(x.cuda(), lam.cuda(), freq.cuda(), symmetrize, True).cpu()))
        if symmetrize:  # d|x_0|/dx_0 = 0 at +-0: the whole tangent along x_0 vanishes there
            at0 = x[:, 0] == 0
            cols = [0] + list(range(3, 3 + n)) + list(range(3 + 3 * n, 3 + 4 * n))
            assert bool(at0.any()) or m == 1
            assert not got[at0][:, cols].any()
        # without the ones column the layout is the embedding's own
        assert torch.equal(ops.harmonic_embed_jvp(x.cuda(), lam.cuda(), freq.cuda(), symmetrize, False).cpu(), got[:, :-1])


# ------------------------------------------------------------------------------------------------------------------ the head
@pytest.mark.parametrize("m", G.GEMM_ROWS)
def test_field_grad_head_against_float64(m):
    ops = _ops()
    inp = G.make_head_inputs(m)
    s, w, y, t = (inp[k].cuda() for k in ("s", "w", "y", "t"))
    b = ops.field_grad_head_fwd(s, w, y)
    # one product per entry: the float32 result is the correctly rounded one, and the mask is threshold_backward's
    want = torch.ops.aten.threshold_backward((inp["s"] * inp["w"]).expand(m, G.N).contiguous(), inp["y"], 0)
    assert torch.equal(_bits(b.cpu()), _bits(want))
    assert F.statistic(b.cpu(), G.head_fwd_ref(inp), G.head_fwd_ref(inp).abs()) <= 0.25
    assert b[0, 2] != 0 and not b[0, :2].any() and b[0, 3] == 0
    (gw_ref, gw_terms), (gs_ref, gs_terms) = G.head_bwd_ref(inp)
    floor = G.head_floor(m)
    g_w, g_s = ops.field_grad_head_bwd(s, t, w, need_s=True)
    _fig(f"head g_w M={m}", F.within(F.statistic(g_w.cpu(), gw_ref, gw_terms), G.MARGIN * floor["g_w"], f"head g_w M={m}"), floor["g_w"])
    _fig(f"head g_s M={m}", F.within(F.statistic(g_s.cpu(), gs_ref, gs_terms), G.MARGIN * floor["g_s"], f"head g_s M={m}"), floor["g_s"])
    again_w, again_s = ops.field_grad_head_bwd(s, t, w, need_s=True)
    assert torch.equal(_bits(g_w), _bits(again_w)) and torch.equal(_bits(g_s), _bits(again_s))
    only_w, none = ops.field_grad_head_bwd(s, t, w)
    assert none is None and torch.equal(_bits(only_w), _bits(g_w))


def test_guard_mode_finds_no_canary_touched_on_ragged_rows():
    L, ops = _L(), _ops()
    prev = L.set_guard(1)
    try:
        before = dict(L.guard_stats)
        for m in (1, 31, 33, 129, 1000):
            for k in G.GEMM_K:
                assert _nt(G.make_nt_inputs(m, k), True).shape == (m, G.N)
            x, gen = F.make_embed_inputs(8, m)
            ops.harmonic_embed_jvp(x.cuda(), torch.randn(m, 3, generator=gen).cuda(), F.embed_freq(8).cuda(), True, True)
            inp = G.make_head_inputs(m)
            ops.field_grad_head_fwd(inp["s"].cuda(), inp["w"].cuda(), inp["y"].cuda())
            ops.field_grad_head_bwd(inp["s"].cuda(), inp["t"].cuda(), inp["w"].cuda(), need_s=True)
            for c in (52, 256):
                p, q = G.make_tn_inputs(m, 2, c)
                ops.gemm_tn_splitk(p.cuda(), q.cuda())
            L.guard_check("test_fieldgrad_gpu")
        assert L.guard_stats["checks"] >= before["checks"] + 5 * 6 and L.guard_stats["allocations"] >= before["allocations"] + 5 * 8
    finally:
        L.set_guard(prev)


# ------------------------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("m,n_hidden", list(itertools.product(G.CHAIN_ROWS, G.CHAIN_LAYERS)))
def test_value_gradient_adjoint_chain_against_float64(m, n_hidden):
    """hostnets._field_value through autograd.grad(create_graph=True) and a second autograd.grad, as the regulariser drives it; the float64
    blocks are evaluated with the masks of the activations this run produced, and those activations are held to float64 here too."""
    H = _hostnets()
    symmetrize, n_freq = True, 8
    net, (x, s, lam) = G.make_net(n_hidden, n_freq), G.make_points(m)
    floor = G.chain_floor(m, n_hidden, n_freq, symmetrize)
    p = lambda t: t.cuda().requires_grad_(True)
    xa, sa, w_in, w_h, hidden = p(x), p(s), p(net["w_in"]), p(net["w_h"]), [p(w) for w in net["hidden"]]

    def run():
        out = H._field_value(xa, w_in, w_h, net["freq"].cuda(), symmetrize, *hidden)
        first = torch.autograd.grad([out], [xa, w_in, w_h, *hidden], grad_outputs=sa, create_graph=True)
        saved = out.grad_fn.saved_tensors[1], first[0].grad_fn.saved_tensors[6]  # y, b [L + 1, M, 256]: y is what the masks were taken from
        second = torch.autograd.grad((first[0] * lam.cuda()).sum(), [w_in, w_h, sa, *hidden])
        return out, first, second, saved

    out, first, second, (y, b) = run()
    ys = [t.cpu() for t in y.unbind(0)]
    fwd = G.forward_statistics(ys, out.detach().cpu(), x, net, symmetrize)
    got = dict(g_x=first[0].detach(), g_in=first[1].detach(), g_head=first[2].detach(), g_hidden=[g.detach() for g in first[3:]],
               a_in=second[0], a_head=second[1], a_s=second[2], a_hidden=list(second[3:]))
    res = G.chain_reference_statistics(got, x, s, lam, net, ys, [t.cpu() for t in b.unbind(0)], None, None, symmetrize)
    res.update(fwd)
    for name in sorted(res):
        _fig(f"chain M={m} L={n_hidden} {name}", res[name], floor[name])
    for name in sorted(res):
        F.within(res[name], G.MARGIN * floor[name], f"chain M={m} L={n_hidden} {name}")
    assert not second[0][:, -1].any()  # the ones column's tangent is 0: no gradient to the first bias
    out2, first2, second2, _ = run()  # the same bits on a second run
    assert torch.equal(_bits(out), _bits(out2))
    assert all(torch.equal(_bits(a_.detach()), _bits(b_.detach())) for a_, b_ in zip(first + second, first2 + second2))
    with pytest.raises(RuntimeError):  # a second-order gradient with respect to the points is not provided
        torch.autograd.grad((run()[1][0] * lam.cuda()).sum(), [xa])
    with pytest.raises(RuntimeError):  # nor a gradient through the first-order weight gradients (once-differentiable, cut from the graph)
        torch.autograd.grad(run()[1][1].sum(), [sa])


# ------------------------------------------------------------------------------------------------------------------ the network
def _geometry(dev, dtype=torch.float32):
    M = importlib.import_module("3danimals_amd.model.geometry.dmtet")
    tetgrid = importlib.import_module("3danimals_amd.tetgrid")
    torch.manual_seed(5)
    geo = M.DMTetGeometry(8, 7.0, num_layers=5, hidden_size=256, embedder_freq=8, symmetrize=True, device=dev, tet_grid=tetgrid.kuhn_grid(4))
    return geo.to(dev).to(dtype)


def _eikonal(geo, pts):
    p = pts.clone().requires_grad_(True)
    y = geo.get_sdf(pts=p)
    g = torch.autograd.grad([y], p, grad_outputs=torch.ones_like(y), create_graph=True)[0]
    loss = ((g.norm(dim=-1) - 1) ** 2).mean()
    params = list(geo.mlp.parameters())
    return g.detach(), [t if t is not None else torch.zeros_like(q) for t, q in zip(torch.autograd.grad(loss, params, allow_unused=True), params)]


@pytest.fixture(scope="module")
def network():
    geo = _geometry("cuda")
    pts = torch.rand(2000, 3, generator=torch.Generator().manual_seed(77)) * 4 - 2
    twin = _geometry("cpu")
    twin.load_state_dict({k: v.cpu() for k, v in geo.state_dict().items()})
    twin = twin.double()
    ref = _eikonal(twin, pts.double())
    return geo, pts, ref


def test_network_route_on_against_off(network):
    """DMTetGeometry at width 256, 5 layers, 2,000 points, loss ((|g| - 1)^2).mean(): the route's error against the float64 CPU twin is
    at most 4 x the error of the plain torch path (USE_FIELD_GRAD off) against the same twin, for g_x and every parameter gradient."""
    H = _hostnets()
    geo, pts, (g_ref, grads_ref) = network
    names = [n for n, _ in geo.mlp.named_parameters()]
    err = {}
    for on in (False, True):
        prev, H.USE_FIELD_GRAD = H.USE_FIELD_GRAD, on
        try:
            g, grads = _eikonal(geo, pts.cuda())
        finally:
            H.USE_FIELD_GRAD = prev
        rel = lambda a, r: float((a.double().cpu() - r).abs().max() / r.abs().max().clamp(min=1e-300))
        err[on] = dict(g_x=rel(g, g_ref), **{n: rel(a, r) for n, a, r in zip(names, grads, grads_ref)})
    for name in err[True]:
        print(f"FIG network {name} on={err[True][name]:.4g} off={err[False][name]:.4g} ratio={err[True][name] / err[False][name] if err[False][name] else 0.0:.3f}")
    for name in err[True]:
        assert err[True][name] <= G.MARGIN * err[False][name], f"{name}: {err[True][name]:.4g} against 4 x {err[False][name]:.4g}"


def test_graphed_route_equals_eager_at_width_256(network):
    """test_graphed_sdf_gradient_equals_eager at the width where the route is live: values and parameter gradients, bit for bit, and again
    after the parameters moved."""
    H = _hostnets()
    geo, pts, _ = network
    geo = copy.deepcopy(geo)
    pts = pts.cuda()
    params = list(geo.mlp.parameters())
    assert H.USE_FIELD_GRAD and geo.mlp._field_grad_ok(pts.clone().requires_grad_(True))
    geo.capture_sdf_gradient_graph(num_points=2000)
    assert (2000, pts.device) in geo._sdf_gradient_graphs

    def eager(p):
        p = p.clone().requires_grad_(True)
        y = geo.get_sdf(pts=p)
        return torch.autograd.grad([y], p, grad_outputs=torch.ones_like(y), create_graph=True)[0]

    loss = lambda g: ((g.norm(dim=-1) - 1) ** 2).mean()
    for _ in range(2):  # as captured, then after the parameters were scaled by 1.01
        ge = eager(pts)
        grads_e = torch.autograd.grad(loss(ge), params, allow_unused=True)
        gg = geo._graphed_sdf_gradient(pts)
        grads_g = torch.autograd.grad(loss(gg), params, allow_unused=True)
        assert torch.equal(ge, gg)
        for a, b_ in zip(grads_e, grads_g):
            assert (a is None and (b_ is None or float(b_.abs().max()) == 0.0)) or torch.equal(a, b_)
        with torch.no_grad():
            for p in params:
                p.mul_(1.01)
