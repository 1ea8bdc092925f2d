"""The weight-modulated SDF field (hostnets.CoordMLP_Mod) on the field kernels -- hostnets.USE_FIELD_MOD, DESIGN.md section 38 -- on the GPU at width
256, where the route is live, against the float64 CPU twin of tests/fieldmod_ref.py.

Criterion, everywhere: the error of the route (switch on) against the twin, max |got - ref64| / max |ref64|, is at most MARGIN (the factor 4 of
tests/fieldgrad_ref.py) times the error of the plain torch path of the SAME module (switch off) against the same twin -- for the value, for
d out / d x and for every parameter gradient, the style network's and the embedding's included.  Every test prints its figures (FIG lines)
before it asserts.

Measured on MI355X (largest on / off ratio; the bar is 4):
    eikonal route 1.61 (in_layer.weight, L = 5, M = 65; g_x 1.41, the embedding 1.44)    masks at exact zeros 1.55
    long lists 1.02    grad-free pass 1.00    DMTetGeometry: both regularisers and the embedding's gradient 1.00
Nothing exceeded the bar."""
import importlib
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fieldmod_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

EIKONAL_ROWS = (1, 63, 65, 200, 2000)  # around the 64-row tile of a3d_gemm_nt_relumask and the 64-row partials of a3d_field_grad_head_bwd
FIELD_KERNELS = {"a3d_gemm_nt_relumask", "a3d_gemm_tn_splitk", "a3d_field_grad_head_fwd", "a3d_gemm_nn_relumask", "a3d_field_head_bwd"}


def _hostnets():
    return importlib.import_module("3danimals_amd.hostnets")


def _L():
    return importlib.import_module("3danimals_amd._lib")


class _switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        H = _hostnets()
        self.prev, H.USE_FIELD_MOD = H.USE_FIELD_MOD, self.on

    def __exit__(self, *exc):
        _hostnets().USE_FIELD_MOD = self.prev
        return False


def _net(num_layers, n_freq, symmetrize, cout=1, min_max=None, seed=0):
    torch.manual_seed(1000 * num_layers + 10 * n_freq + seed)
    return _hostnets().CoordMLP_Mod(3, cout, num_layers, nf=256, n_harmonic_functions=n_freq, embedder_scalar=R.G.F.EMBED_SCALAR,
                                    symmetrize=symmetrize, min_max=min_max).cuda()


def _points(m, seed=0):
    gen = torch.Generator().manual_seed(7919 * m + seed)
    x = torch.rand(m, 3, generator=gen) * 4 - 2
    if m > 1:
        x[m - 1, 0] = 0.0  # d|x_0| / dx_0 = 0 there under symmetrize
    return x, 0.1 * torch.randn(1, 128, generator=gen)


def _named(net, grads, feat_grad):
    names = [n for n, _ in net.named_parameters()]
    params = list(net.parameters())
    out = {n: (g if g is not None else torch.zeros_like(p)) for n, g, p in zip(names, grads, params)}
    out["feat"] = feat_grad
    return out


def _eikonal(net, x, feat):
    """The regulariser's call: autograd.grad(sdf, points, create_graph=True), a loss on the result, gradients to everything."""
    xa, fa = x.cuda().requires_grad_(True), feat.cuda().requires_grad_(True)
    y = net(xa, feat=fa)
    g, = torch.autograd.grad([y], xa, grad_outputs=torch.ones_like(y), create_graph=True)
    loss = ((g.norm(dim=-1) - 1) ** 2).mean()
    grads = torch.autograd.grad(loss, list(net.parameters()) + [fa], allow_unused=True)
    return g.detach(), loss.detach(), _named(net, grads[:-1], grads[-1]), y


def _errors(got, ref):
    return {name: R.rel(got[name], ref[name]) for name in ref}


def _kernels(timer):
    return {n.split("[")[0] for n in timer.summary()}


# ------------------------------------------------------------------------------------------------------------------ the eikonal route
@pytest.mark.parametrize("num_layers,symmetrize,n_freq", list(itertools.product((2, 5), (False, True), (2, 8))))
def test_eikonal_route_against_float64(num_layers, symmetrize, n_freq):
    net = _net(num_layers, n_freq, symmetrize)
    params = R.to_float64(net.state_dict())
    for m in EIKONAL_ROWS:
        x, feat = _points(m)
        g_ref, loss_ref, grads_ref = R.eikonal(params, x, feat, net.embedder.frequencies, symmetrize)
        ref = dict(grads_ref, g_x=g_ref)
        err = {}
        for on in (False, True):
            with _switch(on):
                g, _, grads, y = _eikonal(net, x, feat)
            assert (type(y.grad_fn).__name__ == "_FieldValueBackward") == on
            err[on] = _errors(dict(grads, g_x=g), ref)
        assert set(err[True]) == {"g_x", "feat", "in_layer.weight", "in_layer.bias", *R.layer_keys(params), *R.STYLE_KEYS}
        R.check_ratio(err[True], err[False], f"eikonal L={num_layers} sym={symmetrize} n={n_freq} M={m}")


def test_eikonal_backward_has_the_same_bits_on_every_run():
    net = _net(5, 8, True)
    x, feat = _points(2000)
    with _switch(True):
        g1, l1, grads1, _ = _eikonal(net, x, feat)
        g2, l2, grads2, _ = _eikonal(net, x, feat)
    assert torch.equal(g1, g2) and torch.equal(l1, l2)
    for name in grads1:
        assert torch.equal(grads1[name], grads2[name]), name


def test_inherited_limit_no_second_order_gradient_to_the_points():
    net = _net(2, 8, False)
    x, feat = _points(65)
    with _switch(True):
        xa = x.cuda().requires_grad_(True)
        y = net(xa, feat=feat.cuda())
        g, = torch.autograd.grad([y], xa, grad_outputs=torch.ones_like(y), create_graph=True)
        with pytest.raises(RuntimeError):
            torch.autograd.grad(g.square().sum(), [xa])


# ------------------------------------------------------------------------------------------------------------------ masks at the boundary
def _boundary_case():
    """A field and 12 points with pre-activations that are exactly 0 or -0.0 -- rows of zeros and of -0.0 in every layer, and units of the
    in_layer that see only x and the sines, at the points (0,0,0) and (-0.0,-0.0,-0.0) -- and a seed at which every OTHER unit of the float64
    twin stays 2e-5 away from 0, a hundred float32 roundings of a pre-activation of this size: both precisions then have the same masks."""
    n_freq = 2
    for seed in range(64):
        net = _net(3, n_freq, True, seed=seed)
        with torch.no_grad():
            net.in_layer.weight[0:4, 3 + 3 * n_freq:] = 0.0  # no cosine, no bias: 0 at the origin
            net.in_layer.bias[0:4] = 0.0
            net.in_layer.weight[4:6] = 0.0
            net.in_layer.bias[4:6] = 0.0
            net.in_layer.weight[6:8] = -0.0
            net.in_layer.bias[6:8] = -0.0
            net.mlp.linear_0.weight[0:3] = 0.0
            net.mlp.linear_0.weight[3:5] = -0.0
            net.mlp.linear_1.weight[0:2] = 0.0
            net.mlp.linear_1.weight[2:3] = -0.0
        x, feat = _points(12, seed)
        x[0] = 0.0
        x[1] = -0.0
        x[11, 0] = 0.7
        params = R.to_float64(net.state_dict())
        pre = []
        R.field(params, x.double(), feat.double(), net.embedder.frequencies, True, pre=pre)
        zero = [torch.zeros_like(p, dtype=torch.bool) for p in pre]
        zero[0][:2, 0:4] = True
        zero[0][:, 4:8] = True
        zero[1][:, 0:5] = True
        zero[2][:, 0:3] = True
        assert all(bool((p[z] == 0).all()) for p, z in zip(pre, zero))
        if all(float(p[~z].abs().min()) > 2e-5 for p, z in zip(pre, zero)):
            return net, x, feat, params, [p > 0 for p in pre]
    raise AssertionError("no seed below 64 keeps the other units away from 0")


def test_masks_at_exact_zeros_of_both_signs():
    net, x, feat, params, masks = _boundary_case()
    g_ref, _, grads_ref = R.eikonal(params, x, feat, net.embedder.frequencies, True)
    ref = dict(grads_ref, g_x=g_ref)
    err = {}
    for on in (False, True):
        with _switch(on):
            g, _, grads, y = _eikonal(net, x, feat)
        err[on] = _errors(dict(grads, g_x=g), ref)
        if on:
            acts = y.grad_fn.saved_tensors[1]  # _FieldValue's y [L + 1, M, 256]: what the masks are taken from
            assert tuple(acts.shape) == (3, 12, 256)
            for l in range(3):  # a unit at +-0 is off; every other unit has the twin's sign
                assert torch.equal(acts[l].cpu() > 0, masks[l]), l
            # ... so the rows behind a unit that is off everywhere get no gradient at all, as in the twin
            assert not grads["mlp.linear_0.weight"][0:5].any() and not grads["mlp.linear_1.weight"][0:3].any()
            assert not grads["in_layer.weight"][4:8].any()
            assert not grads_ref["mlp.linear_0.weight"][0:5].any() and not grads_ref["in_layer.weight"][4:8].any()
            assert float(g[0, 0]) == 0.0 and float(g[1, 0]) == 0.0  # d|x_0| / dx_0 at +-0
    R.check_ratio(err[True], err[False], "boundary")


# ------------------------------------------------------------------------------------------------------------------ long lists
_LONG = {}


def _long_case(extra_rows):
    """(net, x, feat, c, out_ref, grads_ref) at M = SPLITK_MIN_ROWS + extra_rows; the twin is evaluated once."""
    if extra_rows not in _LONG:
        H = _hostnets()
        m = H.SPLITK_MIN_ROWS + extra_rows
        if extra_rows:  # three output channels behind the min_max map: the fused head's forward too
            net = _net(3, 8, True, cout=3, min_max=torch.tensor([[-1.0, 1.0], [0.0, 2.0], [0.25, 0.5]]))
        else:
            net = _net(3, 8, True)
        x, feat = _points(m)
        c = torch.randn(m, net.mlp.layers()[-1].weight.shape[0], generator=torch.Generator().manual_seed(m))
        out_ref, grads_ref = R.linear_functional(R.to_float64(net.state_dict()), x, feat, net.embedder.frequencies, c, True,
                                                 net.min_max.cpu() if net.min_max is not None else None)
        _LONG[extra_rows] = (net, x, feat, c, out_ref, grads_ref)
    return _LONG[extra_rows]


def _linear_functional(net, x, feat, c):
    fa = feat.cuda().requires_grad_(True)
    out = net(x.cuda(), feat=fa)
    grads = torch.autograd.grad((out * c.cuda()).sum(), list(net.parameters()) + [fa], allow_unused=True)
    return out, _named(net, grads[:-1], grads[-1])


@pytest.mark.parametrize("extra_parts", (0, 1))
def test_long_list_against_float64(extra_parts):
    H = _hostnets()
    net, x, feat, c, out_ref, grads_ref = _long_case(extra_parts * H.SPLITK_PARTS)
    ref = dict(grads_ref, out=out_ref)
    err = {}
    for on in (False, True):
        with _switch(on):
            out, grads = _linear_functional(net, x, feat, c)
        assert (type(out.grad_fn).__name__ == "_FieldStackHeadBackward") == on
        err[on] = _errors(dict(grads, out=out), ref)
    R.check_ratio(err[True], err[False], f"long list M={x.shape[0]}")


def test_grad_free_pass_against_float64(monkeypatch):
    """The grid pass: no_grad over a long list takes the fused input stage and ReLU in every GEMM's epilogue; the values are held to the
    twin like everything else (the epilogue GEMM need not have the bits of GEMM + ReLU)."""
    net, x, feat, _, out_ref, _ = _long_case(0)
    calls = []
    plain = torch._addmm_activation
    monkeypatch.setattr(torch, "_addmm_activation", lambda *a, **k: (calls.append(1), plain(*a, **k))[1])
    err, count, kernels = {}, {}, {}
    for on in (False, True):
        del calls[:]
        with _switch(on), torch.no_grad(), _L().KernelTimer() as timer:
            out = net(x.cuda(), feat=feat.cuda())
        err[on], count[on], kernels[on] = dict(out=R.rel(out, out_ref)), len(calls), _kernels(timer)
    assert count == {False: 0, True: 3} and "a3d_harmonic_embed_fwd" in kernels[True] and not kernels[False]
    R.check_ratio(err[True], err[False], "grad-free pass")


# ------------------------------------------------------------------------------------------------------------------ what ran
def test_route_record():
    H, L = _hostnets(), _L()
    assert H.USE_FIELD_MOD is (os.environ.get("A3D_FIELD_MOD", "0") not in ("0", ""))  # off unless the environment asks for it
    short = _net(5, 8, True)
    x, feat = _points(200)
    long_net, lx, lfeat, c, _, _ = _long_case(0)
    seen = {}
    for on in (False, True):
        with _switch(on):
            with L.KernelTimer() as timer:
                _eikonal(short, x, feat)
            seen[on, "eikonal"] = _kernels(timer)
            with L.KernelTimer() as timer:
                _linear_functional(long_net, lx, lfeat, c)
            seen[on, "long"] = _kernels(timer)
    assert {"a3d_gemm_nt_relumask", "a3d_gemm_tn_splitk", "a3d_field_grad_head_fwd"} <= seen[True, "eikonal"], seen[True, "eikonal"]
    assert {"a3d_gemm_nn_relumask", "a3d_field_head_bwd"} <= seen[True, "long"], seen[True, "long"]
    assert not (seen[False, "eikonal"] | seen[False, "long"]) & FIELD_KERNELS, (seen[False, "eikonal"], seen[False, "long"])


# ------------------------------------------------------------------------------------------------------------------ DMTetGeometry
def _bce_reg(sdf, edges):
    """reference dmtet.py:161-169 in the dtype of ``sdf``."""
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    pair = sdf[edges.reshape(-1)].reshape(-1, 2)
    pair = pair[torch.sign(pair[..., 0]) != torch.sign(pair[..., 1])]
    return bce(pair[..., 0], (pair[..., 1] > 0).to(sdf.dtype)) + bce(pair[..., 1], (pair[..., 0] > 0).to(sdf.dtype))


def test_conditioned_geometry_on_against_off():
    """DMTetGeometry(condition_choice='mod') on a generated 4^3 Kuhn grid: getMesh(feats) + get_sdf_reg_loss(feats) with the switch on and
    off extract the same triangles, and both regularisers and the embedding's gradient are held to the twin."""
    M = importlib.import_module("3danimals_amd.model.geometry.dmtet")
    tetgrid = importlib.import_module("3danimals_amd.tetgrid")
    scale = 7.0
    torch.manual_seed(5)
    geo = M.DMTetGeometry(8, scale, num_layers=5, hidden_size=256, embedder_freq=8, symmetrize=True, condition_choice="mod", init_sdf="sphere",
                          device="cuda", tet_grid=tetgrid.kuhn_grid(4)).cuda()
    feat = 0.1 * torch.randn(128, generator=torch.Generator().manual_seed(6))
    seen = []
    hook = geo.mlp.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
    got = {}
    try:
        for on in (False, True):
            fa = feat.cuda().requires_grad_(True)
            with _switch(on):
                mesh = geo.getMesh(feats=fa)
                torch.manual_seed(123)  # the regulariser's sample: the same points both times
                with _L().KernelTimer() as timer:
                    reg = geo.get_sdf_reg_loss(feats=fa)
                    g_feat, = torch.autograd.grad(reg["sdf_bce_reg_loss"] + reg["sdf_gradient_reg_loss"], fa)
            ran = _kernels(timer)  # the regulariser through DMTetGeometry: the hand-written gradient chain and its adjoint, or none of it
            want = {"a3d_field_grad_head_fwd", "a3d_gemm_nn_relumask", "a3d_gemm_nt_relumask", "a3d_gemm_tn_splitk"}
            assert (want <= ran) if on else not (ran & FIELD_KERNELS), ran
            pts = seen[-1].detach().cpu()
            got[on] = dict(faces=int(mesh.t_pos_idx.shape[-2]), pts=pts, bce=reg["sdf_bce_reg_loss"].detach(),
                           eikonal=reg["sdf_gradient_reg_loss"].detach(), feat=g_feat)
    finally:
        hook.remove()
    assert got[True]["faces"] == got[False]["faces"] > 0
    assert torch.equal(got[True]["pts"], got[False]["pts"]) and got[True]["pts"].shape[0] > 5000
    # the twin: the sphere prior of get_sdf behind the field, at the sampled points (|x_0| already taken by get_sdf) and on the grid
    params = R.to_float64(geo.mlp.state_dict())
    freq = geo.mlp.embedder.frequencies
    prior = lambda p: scale * 0.25 - p.norm(dim=-1, keepdim=True)
    _, eik_ref, eik_grads = R.eikonal(params, got[True]["pts"], feat, freq, False, extra=prior)
    verts = geo.verts.detach().cpu().double()
    verts = torch.cat([verts[:, :1].abs(), verts[:, 1:]], -1)
    f64 = feat.double().requires_grad_(True)
    bce_ref = _bce_reg((R.field(params, verts, f64, freq) + prior(verts)).squeeze(-1), geo.all_edges.cpu().long()).mean()
    bce_grad, = torch.autograd.grad(bce_ref, f64)
    ref = dict(bce=bce_ref.detach(), eikonal=eik_ref, feat=eik_grads["feat"] + bce_grad)
    err = {on: {k: R.rel(got[on][k], ref[k]) for k in ref} for on in (False, True)}
    R.check_ratio(err[True], err[False], "geometry")


def test_grid_pass_of_get_mesh_reaches_the_epilogue_fused_forward(monkeypatch):
    """getMesh(feats) on a grid of more than SPLITK_MIN_ROWS vertices (41^3): _get_mesh_surface_backward's grad-free pass over the grid takes
    the fused input stage and one epilogue GEMM per ReLU layer; the surface rows, a short list, and everything with the switch off take none.
    The same triangles either way."""
    M = importlib.import_module("3danimals_amd.model.geometry.dmtet")
    tetgrid = importlib.import_module("3danimals_amd.tetgrid")
    torch.manual_seed(5)
    geo = M.DMTetGeometry(80, 7.0, num_layers=3, hidden_size=256, embedder_freq=8, symmetrize=True, condition_choice="mod", init_sdf="sphere",
                          device="cuda", tet_grid=tetgrid.kuhn_grid(40)).cuda()
    assert geo.verts.shape[0] >= _hostnets().SPLITK_MIN_ROWS and geo.surface_only_backward
    feat = (0.1 * torch.randn(128, generator=torch.Generator().manual_seed(6))).cuda().requires_grad_(True)
    calls = []
    plain = torch._addmm_activation
    monkeypatch.setattr(torch, "_addmm_activation", lambda *a, **k: (calls.append(a[1].shape[0]), plain(*a, **k))[1])
    faces, rows = {}, {}
    for on in (False, True):
        del calls[:]
        with _switch(on), _L().KernelTimer() as timer:
            mesh = geo.getMesh(feats=feat)
        faces[on], rows[on] = int(mesh.t_pos_idx.shape[-2]), list(calls)
        assert ("a3d_harmonic_embed_fwd" in _kernels(timer)) == on
    assert rows[False] == [] and rows[True] == [geo.verts.shape[0]] * 3, rows
    assert faces[True] == faces[False] > 0
