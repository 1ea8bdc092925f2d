"""The weight-modulated field's route (hostnets.USE_FIELD_MOD) without a GPU: MLP_Mod.effective_weights is bit for bit the
weight Linear_Mod.forward multiplies with, the switch changes nothing on CPU tensors, the gate's structural half over widths, frequencies,
dropout, depths and the reference formulation, the state_dict layout -- and tests/fieldmod_ref.py against the module itself in float64."""
import importlib
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fieldmod_ref as R  # noqa: E402

hostnets = importlib.import_module("3danimals_amd.hostnets")


class _switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev, hostnets.USE_FIELD_MOD = hostnets.USE_FIELD_MOD, self.on

    def __exit__(self, *exc):
        hostnets.USE_FIELD_MOD = self.prev
        return False


def _styles(n, gen):
    base = torch.randn(n, generator=gen)
    zeros = base.clone()
    zeros[::3] = 0.0
    zeros[1] = -0.0
    huge = base.clone()
    huge[n // 2] = 3e18  # its square is finite in float32, the sum still is
    return dict(plain=base, zeros=zeros, huge=huge, all_zero=torch.zeros(n), batch=torch.stack([base, huge]))


def test_the_switch_ships_off():
    assert hostnets.USE_FIELD_MOD is (os.environ.get("A3D_FIELD_MOD", "0") not in ("0", ""))


@pytest.mark.parametrize("out_features", (256, 1))
def test_effective_weight_is_the_weight_forward_multiplies_with(out_features, monkeypatch):
    gen = torch.Generator().manual_seed(11 + out_features)
    layer = hostnets.Linear_Mod(256, out_features, bias=False)
    with torch.no_grad():
        layer.weight.copy_(torch.randn(out_features, 256, generator=gen) * 0.1)
        layer.weight[0, :7] = 0.0
    x = torch.randn(5, 256, generator=gen)
    seen = []
    plain_linear = hostnets.F.linear

    def spy(inp, weight, bias=None):
        seen.append(weight)
        return plain_linear(inp, weight, bias)

    for name, style in _styles(256, gen).items():
        # the reference's three statements (MLPs.py:234-240), restated here
        s = style.reshape(-1, style.shape[-1])[0] if style.dim() > 1 else style
        w = layer.weight * s.unsqueeze(0)
        w = w / ((w * w).sum(dim=-1, keepdim=True) + 1e-5).sqrt()
        got = layer.effective_weight(style)
        assert torch.equal(got, w), name
        assert bool(torch.isfinite(got).all()), name
        del seen[:]
        monkeypatch.setattr(hostnets.F, "linear", spy)
        try:
            out = layer(x, style)
        finally:
            monkeypatch.setattr(hostnets.F, "linear", plain_linear)
        assert len(seen) == 1 and torch.equal(seen[0], got), name
        assert torch.equal(out, plain_linear(x, got)), name
        if name == "all_zero":  # the 1e-5 term decides: 0 / sqrt(1e-5), not 0 / 0
            assert not got.any()
    # differentiable, to the weight and to the style
    style = _styles(256, gen)["plain"].clone().requires_grad_(True)
    g_w, g_s = torch.autograd.grad(layer.effective_weight(style).square().sum(), [layer.weight, style])
    assert bool(g_w.any()) and bool(g_s.any())


def test_effective_weights_lists_every_layer_once():
    gen = torch.Generator().manual_seed(5)
    style = torch.randn(1, 256, generator=gen)
    for num_layers, cout in ((1, 1), (2, 1), (5, 3)):
        mlp = hostnets.MLP_Mod(256, cout, num_layers, 256)
        ws = mlp.effective_weights(style)
        layers = [mlp.network] if num_layers == 1 else [getattr(mlp, f"linear_{i}") for i in range(num_layers)]
        assert len(ws) == num_layers and tuple(ws[-1].shape) == (cout, 256)
        assert all(torch.equal(w, l.effective_weight(style)) for w, l in zip(ws, layers))
        # ... and the stack over them is the module's forward
        x = torch.randn(9, 256, generator=gen)
        h = x
        for i, w in enumerate(ws):
            h = torch.nn.functional.linear(h, w)
            if i < num_layers - 1:
                h = torch.relu(h)
        assert torch.equal(h, mlp(x, style))


def _net(seed=0, **kw):
    torch.manual_seed(seed)
    cfg = dict(cin=3, cout=1, num_layers=5, nf=256, n_harmonic_functions=8, embedder_scalar=R.G.F.EMBED_SCALAR)
    cfg.update(kw)
    return hostnets.CoordMLP_Mod(**cfg)


@pytest.mark.parametrize("nf,symmetrize", ((256, True), (32, False)))
def test_on_cpu_tensors_the_switch_changes_nothing(nf, symmetrize):
    net = _net(nf=nf, symmetrize=symmetrize, num_layers=3)
    gen = torch.Generator().manual_seed(3)
    x0 = torch.rand(40, 3, generator=gen) * 4 - 2
    feat0 = torch.randn(1, 128, generator=gen)
    results = []
    for on in (False, True):
        with _switch(on):
            x, feat = x0.clone().requires_grad_(True), feat0.clone().requires_grad_(True)
            out = net(x, feat=feat)
            g, = torch.autograd.grad([out], x, grad_outputs=torch.ones_like(out), create_graph=True)
            loss = ((g.norm(dim=-1) - 1) ** 2).mean() + out.mean()
            grads = torch.autograd.grad(loss, list(net.parameters()) + [feat])
            with torch.no_grad():
                plain = net.sample(x0, feat0)
            results.append((out.detach(), g.detach(), plain, *grads))
    assert all(torch.equal(a, b) for a, b in zip(*results))


class _OnDevice:
    """Says it is a float32 tensor on the GPU: the gate's structural half needs no device."""
    is_cuda, dtype, requires_grad = True, torch.float32, True

    def __init__(self, *shape):
        self.shape = shape

    def dim(self):
        return len(self.shape)


def test_the_gate_over_widths_frequencies_dropout_depths_and_the_reference_formulation():
    x, feat = _OnDevice(10000, 3), _OnDevice(1, 128)
    want = {}
    for nf, n_freq, dropout, num_layers, reference in itertools.product((64, 256), (7, 8), (0, 0.1), (1, 2, 5), (False, True)):
        net = _net(nf=nf, n_harmonic_functions=n_freq, dropout=dropout, num_layers=num_layers)
        hostnets.reference_formulation(reference)
        try:
            with _switch(True):
                got = net._field_mod_ok(x, feat)
            with _switch(False):
                assert not net._field_mod_ok(x, feat)
        finally:
            hostnets.reference_formulation(False)
        want[(nf, n_freq, dropout, num_layers, reference)] = got
        assert got == (nf == 256 and n_freq == 8 and dropout == 0 and num_layers >= 2 and not reference), (nf, n_freq, dropout, num_layers, reference)
    assert sum(want.values()) == 2  # width 256, even frequencies, no dropout, 2 or 5 layers, not the reference formulation
    ok = _net()
    with _switch(True):
        assert ok._field_mod_ok(x, feat)
        for bad_x in (_OnDevice(10000, 2), _OnDevice(10, 100, 3), torch.zeros(8, 3), _OnDevice(0, 3)):
            assert not ok._field_mod_ok(bad_x, feat)
        double = _OnDevice(10000, 3)
        double.dtype = torch.float64
        half_feat = _OnDevice(1, 128)
        half_feat.dtype = torch.float16
        assert not ok._field_mod_ok(double, feat) and not ok._field_mod_ok(x, half_feat) and not ok._field_mod_ok(x, torch.zeros(1, 128))
        assert not _net(n_harmonic_functions=0)._field_mod_ok(x, feat) and not _net(embed_concat_pts=False)._field_mod_ok(x, feat)
        assert _net(cout=3, min_max=torch.tensor([[0.0, 1.0]] * 3))._field_mod_ok(x, feat)  # a wider head with a map: the stack routes take it


def test_the_gates_it_shares_are_coordmlps_own_functions():
    for name in ("_fused_input_ok", "_fused_input", "_stack_input_ok", "_field_grad_input_ok", "_fused_head_of", "_w_in", "_stack_node"):
        assert getattr(hostnets.CoordMLP_Mod, name) is getattr(hostnets.CoordMLP, name), name


def test_state_dict_layout_and_initialisation_are_unchanged():
    net = _net()
    keys = ["in_layer.weight", "in_layer.bias"] + [f"mlp.linear_{i}.weight" for i in range(5)] + list(R.STYLE_KEYS)
    assert list(net.state_dict()) == keys
    assert list(_net(num_layers=1).state_dict()) == ["in_layer.weight", "in_layer.bias", "mlp.network.weight", *R.STYLE_KEYS]
    assert sorted(_net(min_max=torch.tensor([[0.0, 1.0]])).state_dict()) == sorted(keys + ["min_max"])
    # the same draws from the generator as before the route existed: in_layer, the MLP_Mod layers in order, the style network
    torch.manual_seed(0)
    lin = torch.nn.Linear(3 + 6 * 8, 256)
    first = hostnets.Linear_Mod(256, 256, bias=False)
    assert torch.equal(net.in_layer.weight, lin.weight) and torch.equal(net.in_layer.bias, lin.bias)
    assert torch.equal(net.mlp.linear_0.weight, first.weight)


@pytest.mark.parametrize("num_layers,symmetrize,n_freq", ((1, False, 4), (3, True, 8)))
def test_the_float64_twin_is_the_modules_function(num_layers, symmetrize, n_freq):
    net = _net(nf=32, num_layers=num_layers, symmetrize=symmetrize, n_harmonic_functions=n_freq, cout=2,
               min_max=torch.tensor([[-1.0, 2.0], [0.5, 0.75]])).double()
    gen = torch.Generator().manual_seed(9)
    x = (torch.rand(33, 3, generator=gen) * 4 - 2).double()
    feat = torch.randn(1, 128, generator=gen).double()
    c = torch.randn(33, 2, generator=gen).double()
    params = R.to_float64(net.state_dict())
    freq = net.embedder.frequencies
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)
    # a linear functional of the mapped output
    fa = feat.clone().requires_grad_(True)
    out = net(x, feat=fa)
    grads = torch.autograd.grad((out * c).sum(), list(net.parameters()) + [fa])
    out_ref, grads_ref = R.linear_functional(params, x, feat, freq, c, symmetrize, net.min_max)
    assert close(out_ref, out.detach())
    for (name, _), g in zip(list(net.named_parameters()) + [("feat", None)], grads):
        assert close(grads_ref[name], g), name
    # the eikonal term of the first output channel's field (a scalar head)
    scalar = _net(nf=32, num_layers=max(num_layers, 2), symmetrize=symmetrize, n_harmonic_functions=n_freq).double()
    xa, fa = x.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    y = scalar(xa, feat=fa)
    g, = torch.autograd.grad([y], xa, grad_outputs=torch.ones_like(y), create_graph=True)
    loss = ((g.norm(dim=-1) - 1) ** 2).mean()
    grads = torch.autograd.grad(loss, list(scalar.parameters()) + [fa], allow_unused=True)
    g_ref, loss_ref, grads_ref = R.eikonal(R.to_float64(scalar.state_dict()), x, feat, scalar.embedder.frequencies, symmetrize)
    assert close(g_ref, g.detach()) and close(loss_ref, loss.detach())
    for (name, _), got in zip(list(scalar.named_parameters()) + [("feat", None)], grads):
        assert close(grads_ref[name], got if got is not None else torch.zeros_like(grads_ref[name])), name
