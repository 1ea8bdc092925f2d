"""tests/fieldgrad_ref.py against torch itself, without a GPU: the float64 statements of the field's value, input gradient and the adjoint
of that gradient equal torch's own double backward of the plain F.linear / relu / HarmonicEmbedding formulation in float64 to 1e-12
relative, for L in {1, 4} hidden layers, n in {8, 10} frequencies (K0 = 52 and 64) and symmetrize on and off -- so what the GPU tests
compare the kernels against is the function autograd differentiates.  Plus the route's gate and what the loaded library refuses, which need no GPU either."""
import importlib
import itertools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fieldgrad_ref as G  # noqa: E402

hostnets = importlib.import_module("3danimals_amd.hostnets")
TOL = 1e-12


def _close(got, ref, what):
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= TOL * max(scale, 1e-300), f"{what}: max |difference| {err:.3g} against a largest entry of {scale:.3g}"


@pytest.mark.parametrize("n_hidden,n_freq,symmetrize", list(itertools.product((1, 4), (8, 10), (False, True))))
def test_the_three_blocks_equal_torchs_double_backward_in_float64(n_hidden, n_freq, symmetrize):
    m = 37
    net = G.make_net(n_hidden, n_freq, dtype=torch.float64)
    x, s, lam = (t.double() for t in G.make_points(m))
    x[1, 0] = -0.7  # a negative x_0: the sign of d|x_0|/dx_0
    emb = hostnets.HarmonicEmbedding(n_freq, G.F.EMBED_SCALAR)
    assert torch.equal(emb.frequencies, net["freq"])
    weight = net["w_in"][:, :-1].clone().requires_grad_(True)
    bias = net["w_in"][:, -1].clone().requires_grad_(True)
    hidden = [w.clone().requires_grad_(True) for w in net["hidden"]]
    w_h = net["w_h"].clone().requires_grad_(True)
    xa, sa = x.clone().requires_grad_(True), s.clone().requires_grad_(True)
    xs = torch.cat([xa[..., :1].abs(), xa[..., 1:]], -1) if symmetrize else xa
    h = torch.relu(F.linear(torch.cat([xs, emb(xs)], -1), weight, bias))
    ys = [h]
    for w in hidden:
        ys.append(torch.relu(F.linear(ys[-1], w)))
    out = F.linear(ys[-1], w_h)
    g_x, = torch.autograd.grad([out], [xa], grad_outputs=sa, create_graph=True)
    params = [weight, bias, *hidden, w_h, sa]
    first = torch.autograd.grad([out], params[:-1], grad_outputs=s, retain_graph=True)
    second = torch.autograd.grad((g_x * lam).sum(), params)

    e = G.embed(x, net["freq"], symmetrize)
    ys_ref, out_ref = G.value(e, net["w_in"], net["hidden"], net["w_h"])
    _close(out_ref, out.detach(), "value")
    masks = G.masks_of(ys_ref)
    assert all(torch.equal(a, b.detach() > 0) for a, b in zip(masks, ys))
    gval, _ = G.gradient(s, e, ys_ref, masks, net["w_in"], net["hidden"], net["w_h"])
    _close(G.embed_vjp(gval["v"], x, net["freq"], symmetrize)[0], g_x.detach(), "g_x")
    _close(gval["g_in"][:, :-1], first[0], "first-order dW_in")
    _close(gval["g_in"][:, -1], first[1], "first-order d bias")
    for l in range(n_hidden):
        _close(gval["g_hidden"][l], first[2 + l], f"first-order dW_{l + 1}")
    _close(gval["g_head"], first[2 + n_hidden], "first-order dw_h")
    aval, _ = G.adjoint(G.embed_jvp(lam, x, net["freq"], symmetrize), s, gval["b"], masks, net["w_in"], net["hidden"], net["w_h"])
    _close(aval["g_in"][:, :-1], second[0], "adjoint dW_in")
    _close(aval["g_in"][:, -1], second[1], "adjoint d bias")
    assert float(second[1].abs().max()) == 0.0  # the ones column's tangent is 0: the eikonal term has no gradient to the first bias
    for l in range(n_hidden):
        _close(aval["g_hidden"][l], second[2 + l], f"adjoint dW_{l + 1}")
    _close(aval["g_head"], second[2 + n_hidden], "adjoint dw_h")
    _close(aval["g_s"], second[3 + n_hidden], "adjoint ds")


def test_the_jvp_is_the_transpose_of_the_vjp():
    """<J lam, v> == <lam, J^T v> for random v, lam, under symmetrize with x_0 = +-0 and with float32-rounded angles."""
    for n, symmetrize in itertools.product(G.JVP_N, (False, True)):
        x, _, lam = G.make_points(33)
        freq = G.F.embed_freq(n)
        v = torch.randn(33, 4 + 6 * n, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
        lhs = (G.embed_jvp(lam, x, freq, symmetrize, angle32=True) * v).sum()
        rhs = (lam.double() * G.embed_vjp(v, x, freq, symmetrize, angle32=True)[0]).sum()
        assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs))
        if symmetrize:
            assert not G.embed_jvp(lam, x, freq, True)[0].reshape(-1)[[0] + list(range(3, 3 + n)) + list(range(3 + 3 * n, 3 + 4 * n))].any()


def test_the_gate_takes_only_the_standard_scalar_field():
    """Without a GPU every input fails the gate on is_cuda; the structural half is checked on a stand-in that says it is on the device."""
    class OnDevice:
        is_cuda, dtype, shape, requires_grad = True, torch.float32, (10000, 3), True

        def dim(self):
            return 2

    std = dict(cin=3, cout=1, num_layers=5, nf=256, n_harmonic_functions=8)
    ok = hostnets.CoordMLP(**std)
    assert ok._field_grad_ok(OnDevice())
    assert not ok._field_grad_ok(torch.zeros(8, 3, requires_grad=True))  # a CPU tensor
    for change in (dict(requires_grad=False), dict(shape=(hostnets.SPLITK_MIN_ROWS, 3)), dict(shape=(10000, 2)), dict(dtype=torch.float64)):
        other = OnDevice()
        for k, v in change.items():
            setattr(other, k, v)
        assert not ok._field_grad_ok(other), change
    with torch.no_grad():
        assert not ok._field_grad_ok(OnDevice())
    for change in (dict(nf=32), dict(cout=3), dict(num_layers=1), dict(activation="tanh"), dict(dropout=0.1), dict(n_harmonic_functions=7),
                   dict(n_harmonic_functions=0), dict(embed_concat_pts=False), dict(min_max=torch.tensor([[0.0, 1.0]])), dict(extra_feat_dim=4)):
        assert not hostnets.CoordMLP(**dict(std, **change))._field_grad_ok(OnDevice()), change
    prev, hostnets.USE_FIELD_GRAD = hostnets.USE_FIELD_GRAD, False
    try:
        assert not ok._field_grad_ok(OnDevice())
    finally:
        hostnets.USE_FIELD_GRAD = prev
    prev = hostnets.reference_formulation(True)
    try:  # the reference formulation never reaches the gate: forward returns before it
        x = torch.rand(4, 3, requires_grad=True)
        assert ok(x).shape == (4, 1)
    finally:
        hostnets.reference_formulation(False)


def test_scratch_sizes_and_argument_refusal_through_the_loaded_library():
    """(csrc/fieldgrad.h itself is held to its entry of _lib.INTERNAL_SURFACES by tests/test_abi_cpu.py, like every header.)"""
    lib = importlib.import_module("3danimals_amd._lib").lib()
    assert lib.a3d_field_grad_head_scratch_bytes(1) == 1024 and lib.a3d_field_grad_head_scratch_bytes(65) == 2048
    assert lib.a3d_field_grad_head_scratch_bytes(0) == 0
    # refused before anything is launched: a K that is no multiple of 4, an N other than 256, a missing operand
    assert lib.a3d_gemm_nt_relumask(None, None, None, 8, 256, 50, None, None) != 0
    assert lib.a3d_gemm_nt_relumask(None, None, None, 8, 128, 64, None, None) != 0
    assert lib.a3d_gemm_nt_relumask(None, None, None, 8, 256, 64, None, None) != 0
    assert lib.a3d_gemm_nt_relumask(None, None, None, 0, 256, 64, None, None) == 0  # an empty list is no work
    assert lib.a3d_field_grad_head_fwd(None, None, None, 8, None, None) != 0
    assert lib.a3d_harmonic_embed_jvp(None, None, None, 0, 0, 1, 8, None, None) != 0
