"""prepare_shading_normal with a perturbed normal on the GPU, through renderutils / ops.shading_normal and through the C ABI directly.

Parity rule (bsdf_cases.parity): the kernel's error against the float64 restatement (tests/tangent_ref.py, held to the reference's
goldens by tests/test_tangent_cpu.py) is bounded by the error of the float32 torch statements on the same inputs, per tensor:
max e(hip) <= 4 max e(twin32) and mean e(hip) <= 2 mean e(twin32).  Pixels within 1e-5 of a kink are left out of the GRADIENT comparison
only, and may be at most 1 % of a case.
"""
import ctypes
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bsdf_cases as BC  # noqa: E402
import tangent_cases as C  # noqa: E402
import tangent_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
variants = pytest.mark.parametrize("two_sided,opengl", C.VARIANTS)


def _ru():
    return importlib.import_module("3danimals_amd.model.render.renderutils")


def _ops():
    return importlib.import_module("3danimals_amd.ops")


def _grads(out, xs, g_out):
    return out.detach().cpu(), [g.cpu() for g in torch.autograd.grad(out, xs, g_out.to(device=out.device, dtype=out.dtype))]


def _hip(inputs, g_out, two_sided, opengl):
    xs = [t.cuda().requires_grad_(True) for t in inputs]
    return _grads(_ru().prepare_shading_normal(*xs, two_sided_shading=two_sided, opengl=opengl), xs, g_out)


def _twin32(inputs, g_out, two_sided, opengl):
    xs = [t.clone().requires_grad_(True) for t in inputs]
    return _grads(_ru().prepare_shading_normal(*xs, two_sided_shading=two_sided, opengl=opengl, use_python=True), xs, g_out)


def _x64(inputs, g_out, two_sided, opengl):
    xs = [t.double().requires_grad_(True) for t in inputs]
    return _grads(R.shading_normal(*xs, two_sided, opengl), xs, g_out)


def _compare(what, inputs, g_out, two_sided, opengl):
    out, gs = _hip(inputs, g_out, two_sided, opengl)
    o32, g32 = _twin32(inputs, g_out, two_sided, opengl)
    o64, g64 = _x64(inputs, g_out, two_sided, opengl)
    assert out.shape == o64.shape and out.dtype == torch.float32
    BC.parity(f"{what} out", out, o32, o64)
    bad = C.sn_near_kink(inputs, two_sided, opengl)
    share = float(bad.double().mean())
    assert share <= C.KINK_CAP, (what, share)
    for i, (g, a, b) in enumerate(zip(gs, g32, g64)):
        assert g.shape == inputs[i].shape and g.dtype == torch.float32, (what, i, g.shape)
        full = tuple(b.shape[:-1]) == tuple(bad.shape)  # (a reduced gradient sums over the pixels: nothing to leave out)
        if not full:
            assert not bool(bad.any()), what
        BC.parity(f"{what} grad {i}", g, a, b, ~bad if full else None)
    out2, gs2 = _hip(inputs, g_out, two_sided, opengl)  # bit-identical across two calls
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(gs, gs2))
    return out, gs


def _g_out(inputs, seed):
    return torch.randn(C.sn_out_shape(inputs), generator=torch.Generator().manual_seed(3000 + seed))


@variants
@pytest.mark.parametrize("kind", ["cond", "wild"])
def test_parity_on_512_pixels(kind, two_sided, opengl):
    seed = {k: s for k, ts, gl, s in C.SN_GOLDEN_CASES if (ts, gl) == (two_sided, opengl)}[kind]
    inputs = C.make_sn_inputs(kind, 512, seed, opengl)
    _compare(f"{kind} {two_sided} {opengl}", inputs, _g_out(inputs, seed), two_sided, opengl)


@variants
def test_broadcast_view_and_constant_perturbation(two_sided, opengl):
    """[2,16,16] with view_pos [2,1,1,3] and perturbed_nrm [1,1,1,3]: both reduce shapes beside four per-pixel gradients."""
    seed = {k: s for k, ts, gl, s in C.SN_GOLDEN_CASES if (ts, gl) == (two_sided, opengl)}["bcast"]
    inputs = C.make_sn_inputs("bcast", 512, seed, opengl)
    plan = _ops()._BsdfPlan("shading_normal", tuple(inputs))
    assert plan.run == [None, 256, 512, None, None, None] and plan.seg == 256
    out, gs = _compare(f"bcast {two_sided} {opengl}", inputs, _g_out(inputs, seed), two_sided, opengl)
    assert float(gs[1].abs().min()) > 0  # the ramp is live: the viewers do receive a gradient
    # the same inputs expanded in memory: same values, the reduced gradients are the sums of the expanded case's
    expanded = [t.expand(2, 16, 16, 3).contiguous() for t in inputs]
    oe, ge = _hip(expanded, _g_out(inputs, seed), two_sided, opengl)
    _, g64 = _x64(expanded, _g_out(inputs, seed), two_sided, opengl)
    _, g32 = _twin32(expanded, _g_out(inputs, seed), two_sided, opengl)
    assert torch.equal(oe, out)
    for i in (1, 2):
        BC.parity(f"bcast grad {i} vs summed expanded", gs[i], g32[i].sum_to_size(inputs[i].shape), g64[i].sum_to_size(inputs[i].shape))


@variants
@pytest.mark.parametrize("shape,seed", [((1025,), 31), ((3109,), 32), ((3, 5, 7), 33)])
def test_tile_edges(shape, seed, two_sided, opengl):
    """A3D_BSDF_TILE = 1024: one segment of 1025 pixels (a second work-group with one pixel), 1024 + 2 x 1024 + 37, and [3,5,7] which
    merges to 105 pixels, no multiple of anything.  Parity per shape, and every shape is also the head of a larger call whose rows it
    must reproduce bit for bit (the kernel is per pixel)."""
    n = 1
    for v in shape:
        n *= v
    for kind in ("cond", "wild"):
        flat = C.make_sn_inputs(kind, n, seed, opengl)
        inputs = [t.reshape(*shape, 3) for t in flat]
        g_out = _g_out(inputs, seed)
        out, gs = _compare(f"{kind} {shape} {two_sided} {opengl}", inputs, g_out, two_sided, opengl)
        assert out.shape == (*shape, 3)
        tail = C.make_sn_inputs("wild", 1500, seed + 50, opengl)
        big = [torch.cat([a, b]) for a, b in zip(flat, tail)]
        g_big = torch.cat([g_out.reshape(n, 3), torch.ones(1500, 3)])
        ob, gb = _hip(big, g_big, two_sided, opengl)
        assert torch.equal(ob[:n], out.reshape(n, 3))
        for i in range(6):
            assert torch.equal(gb[i][:n], gs[i].reshape(n, 3)), (kind, shape, i)


@variants
def test_strided_views_are_read_in_place(two_sided, opengl):
    """perturbed_nrm = all_tex[..., 6:9] of a [2,8,8,9] buffer (pixel stride 9, channel stride 1, as render.py slices it) and smooth_nrm a
    permuted view of channel-first storage: no copy (the plan keeps the strides), same bits as the contiguous call, parity."""
    flat = C.make_sn_inputs("cond", 128, 34, opengl)
    inputs = [t.reshape(2, 8, 8, 3) for t in flat]
    g_out = _g_out(inputs, 34)
    out, gs = _compare(f"strided (contiguous twin) {two_sided} {opengl}", inputs, g_out, two_sided, opengl)
    all_tex = torch.rand(2, 8, 8, 9, generator=torch.Generator().manual_seed(1))
    all_tex[..., 6:9] = inputs[2]
    all_tex = all_tex.cuda().requires_grad_(True)
    chw = inputs[3].permute(0, 3, 1, 2).contiguous().cuda().requires_grad_(True)
    xs = [t.cuda().requires_grad_(True) for t in inputs]
    xs[2], xs[3] = all_tex[..., 6:9], chw.permute(0, 2, 3, 1)
    assert xs[2].stride() == (576, 72, 9, 1) and xs[3].stride() == (192, 8, 1, 64)
    plan = _ops()._BsdfPlan("shading_normal", tuple(xs))
    assert plan.shape == [2, 64] and plan.strides[2] == [576, 9] and plan.cstrides[2] == 1 and plan.strides[3] == [192, 1] and plan.cstrides[3] == 64
    o = _ru().prepare_shading_normal(*xs, two_sided_shading=two_sided, opengl=opengl)
    leaves = xs[:2] + [all_tex, chw] + xs[4:]
    g = torch.autograd.grad(o, leaves, g_out.cuda())
    assert torch.equal(o.cpu(), out)
    assert torch.equal(g[2][..., 6:9].cpu(), gs[2]) and float(g[2][..., :6].abs().max()) == 0.0
    assert torch.equal(g[3].permute(0, 2, 3, 1).cpu(), gs[3])
    for i in (0, 1, 4, 5):
        assert torch.equal(g[i].cpu(), gs[i])


def test_none_and_use_python_do_not_depend_on_the_switch():
    """perturbed_nrm=None and use_python=True run the statements they ran before: bit-identical with the switch off."""
    ru = _ru()
    rops = importlib.import_module("3danimals_amd.model.render.renderutils.ops")
    inputs = [t.cuda() for t in C.make_sn_inputs("wild", 512, 7)]
    g_out = _g_out(inputs, 7).cuda()

    def run(**kw):
        xs = [t.clone().requires_grad_(True) for t in inputs]
        per = None if kw.pop("none", False) else xs[2]
        out = ru.prepare_shading_normal(xs[0], xs[1], per, xs[3], xs[4], xs[5], **kw)
        leaves = [x for i, x in enumerate(xs) if not (per is None and i in (2, 4))]
        return [out.detach()] + list(torch.autograd.grad(out, leaves, g_out))

    assert rops.HIP_SHADING_NORMAL is True
    on = [run(none=True), run(use_python=True), run(none=True, two_sided_shading=False), run()]
    rops.HIP_SHADING_NORMAL = False
    try:
        off = [run(none=True), run(use_python=True), run(none=True, two_sided_shading=False), run()]
    finally:
        rops.HIP_SHADING_NORMAL = True
    for a, b in zip(on[:3], off[:3]):
        assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    assert torch.equal(off[3][0], on[1][0])  # switched off, the default call IS the statements
    assert float((on[3][0] - off[3][0]).abs().max()) < 1e-5  # ... and switched on it is the kernel, the same values to rounding


def test_through_the_c_abi_directly():
    """a3d_shading_normal_fwd / _bwd with a descriptor written by hand: one dimension of 1500 pixels, unit strides, every gradient direct --
    the same bits as the call through ops; and the rows of a two-segment descriptor."""
    L = importlib.import_module("3danimals_amd._lib")
    n = 1500
    inputs = [t.cuda() for t in C.make_sn_inputs("wild", n, 9)]
    g_out = _g_out(inputs, 9).cuda()
    d = L.BsdfDesc(size=ctypes.sizeof(L.BsdfDesc), op=L.SHADING_NORMAL_OP, variant=3, ndim=1, seg=n)
    d.shape[0] = n
    out = torch.empty(n, 3, device="cuda")
    grads = [torch.empty(n, 3, device="cuda") for _ in range(6)]
    for i, t in enumerate(inputs):
        getattr(d, "in")[i], d.stride[4 * i], d.cstride[i] = t.data_ptr(), 3, 1
        d.g_mode[i], d.g_in[i] = 1, grads[i].data_ptr()
    d.out, d.g_out = out.data_ptr(), g_out.data_ptr()
    assert L.lib().a3d_shading_normal_rows(ctypes.byref(d)) == 2
    L.call("a3d_shading_normal_fwd", ctypes.byref(d), L.stream())
    L.call("a3d_shading_normal_bwd", ctypes.byref(d), L.stream())
    xs = [t.clone().requires_grad_(True) for t in inputs]
    o = _ops().shading_normal(*xs)
    g = torch.autograd.grad(o, xs, g_out)
    assert torch.equal(o, out) and all(torch.equal(a, b) for a, b in zip(g, grads))
    with pytest.raises(L.A3DError, match="a3d_bsdf_fwd"):  # the BSDF entry points refuse the new code
        L.call("a3d_bsdf_fwd", ctypes.byref(d), L.stream())
