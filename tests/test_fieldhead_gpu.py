"""The fields' output stage on the GPU (csrc/fieldhead.hip through ops.field_head_fwd / field_head_bwd and hostnets._FieldStackHead) against
the float64 statements of tests/fieldhead_ref.py: the error statistic stays within 4x of what a float32 evaluation on the CPU reaches
on the same inputs, the ReLU mask is threshold_backward's bit for bit, the weight gradient has the same bits on every run, the network
with the fused stage agrees with the layer-by-layer one, and guard mode finds no canary touched.

Measured on MI355X (largest statistic over all cases | largest ratio to the CPU's figure for the same row count; the bar is 4):
    s 0.55 | 0.78    out 0.83 | 0.78    g_h 9.6 | 1.19    g_w 3.4 | 1.04  (2569 at M = 1, the CPU's own figure there: a denormal product)
"""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fieldhead_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _ops():
    return importlib.import_module("3danimals_amd.ops")


def _run(inp, act):
    ops = _ops()
    dev = {k: (None if v is None else v.cuda()) for k, v in inp.items()}
    s, out = ops.field_head_fwd(dev["h"], dev["w"], dev["lo"], dev["scale"], act)
    g_h, g_w = ops.field_head_bwd(dev["g_out"], s, dev["h"], dev["w"], dev["scale"], act)
    return dev, dict(s=s, out=out, g_h=g_h, g_w=g_w)


@pytest.mark.parametrize("c", R.CHANNELS)
@pytest.mark.parametrize("m", R.ROWS)
def test_kernels_against_float64_within_four_times_the_float32_cpu_evaluation(m, c):
    floor = R.noise_floor()
    for act, with_map in R.MODES:
        inp = R.make_inputs(m, c, with_map)
        assert R.has_the_special_values(inp["h"])
        dev, got = _run(inp, act)
        assert (got["s"] is None) == (not act and not with_map)
        stats = R.statistics({k: (None if v is None else v.cpu()) for k, v in got.items()}, inp, act)
        print(f"M={m} C={c} act={act} map={with_map}: " + "  ".join(f"{k} {v:.3f} (cpu {floor[k, m]:.3f})" for k, v in stats.items()))
        # the mask, bit for bit: exactly +0.0 where threshold_backward gives 0, and nowhere else (no product of these inputs underflows)
        passes = torch.ops.aten.threshold_backward(torch.ones_like(dev["h"]), dev["h"], 0) != 0
        assert torch.equal(passes.cpu(), inp["h"] > 0)
        assert torch.equal(got["g_h"] != 0, passes) and bool((got["g_h"].view(torch.int32)[~passes] == 0).all())
        assert passes[0, 2] and not passes[0, 0] and not passes[0, 1] and not passes[0, 3]  # the denormal; 0.0, -0.0 and -1.5
        for name, v in stats.items():
            assert v <= R.MARGIN * floor[name, m], (name, m, c, act, with_map, v, floor[name, m])
        # the same bits on a second run
        _, again = _run(inp, act)
        for name in R.QUANTITIES:
            if got[name] is not None:
                assert torch.equal(got[name].view(torch.int32), again[name].view(torch.int32)), name


def test_s_is_ignored_without_the_sigmoid_and_inputs_are_left_alone():
    ops = _ops()
    inp = R.make_inputs(257, 9, True)
    dev = {k: v.cuda() for k, v in inp.items()}
    keep = {k: v.clone() for k, v in dev.items()}
    s, out = ops.field_head_fwd(dev["h"], dev["w"], dev["lo"], dev["scale"], 0)
    assert torch.equal(out, s * dev["scale"] + dev["lo"])
    a = ops.field_head_bwd(dev["g_out"], None, dev["h"], dev["w"], dev["scale"], 0)
    b = ops.field_head_bwd(dev["g_out"], s, dev["h"], dev["w"], dev["scale"], 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in dev:
        assert torch.equal(dev[k].view(torch.int32), keep[k].view(torch.int32)), k
    # a non-contiguous gradient (an expanded one, as a sum's adjoint is) is read as what it stands for
    g = torch.full((1, 1), 0.5, device="cuda").expand(257, 9)
    c = ops.field_head_bwd(g, None, dev["h"], dev["w"], dev["scale"], 0)
    d = ops.field_head_bwd(g.contiguous(), None, dev["h"], dev["w"], dev["scale"], 0)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


@pytest.mark.parametrize("kind", ["sigmoid16", "plain3"])
def test_network_with_the_fused_stage_matches_the_layer_by_layer_tail(kind):
    """The bars of test_gpu_parity.py::test_field_stack_matches_layer_by_layer_path."""
    hostnets = importlib.import_module("3danimals_amd.hostnets")
    torch.manual_seed(1)
    if kind == "sigmoid16":
        lo = torch.linspace(-0.5, 0.25, 16)
        net, c = hostnets.CoordMLP(3, 16, 5, nf=256, activation="sigmoid", min_max=torch.stack([lo, lo + torch.linspace(0.5, 2.0, 16)], 1)).cuda(), 16
    else:
        net, c = hostnets.CoordMLP(3, 3, 5, nf=256).cuda(), 3
    g = torch.Generator().manual_seed(3)
    P = hostnets.SPLITK_MIN_ROWS + 8192
    x0 = (torch.rand(P, 3, generator=g) * 2 - 1).cuda()
    w = torch.rand(P, c, generator=g).cuda()
    calls = []
    ops = _ops()
    real = ops.field_head_bwd

    def run(use_head):
        hostnets.USE_FIELD_HEAD = use_head
        ops.field_head_bwd = lambda *a, **k: (calls.append(use_head), real(*a, **k))[1]
        try:
            x = x0.clone().requires_grad_(True)
            out = net.sample(x)
            return out.detach(), torch.autograd.grad((out * w).sum(), [x] + list(net.parameters()))
        finally:
            hostnets.USE_FIELD_HEAD = True
            ops.field_head_bwd = real

    (oa, ga), (ob, gb) = run(True), run(False)
    assert calls == [True]  # the fused stage ran, and only when switched on
    print(f"{kind}: out max|d| {float((oa - ob).abs().max()):.3e}; " + " ".join(f"{float((u - v).abs().max() / v.abs().max()):.2e}" for u, v in zip(ga, gb)))
    assert torch.allclose(oa, ob, atol=2e-6)
    for u, v in zip(ga, gb):
        assert float((u - v).abs().max()) <= 1e-4 * float(v.abs().max()) + 1e-7


def test_guard_mode_finds_no_canary_touched_on_a_ragged_list():
    L = importlib.import_module("3danimals_amd._lib")
    prev = L.set_guard(1)
    try:
        before = dict(L.guard_stats)
        for m, c, act, with_map in ((2 * R.WG_ROWS + 1, 9, 1, True), (1037, 16, 1, True), (31, 3, 0, False), (1, 1, 0, True)):
            _, got = _run(R.make_inputs(m, c, with_map), act)  # (ops.call checks every live canary after each entry point and raises)
            assert got["g_h"].shape == (m, 256) and got["g_w"].shape == (c, 256)
            L.guard_check("test_fieldhead_gpu")
        assert L.guard_stats["checks"] >= before["checks"] + 12 and L.guard_stats["allocations"] >= before["allocations"] + 4 * 4
    finally:
        L.set_guard(prev)
