"""Shading BSDFs and HDR image loss on the GPU, every call through the public functions of renderutils and so through the C ABI.

Parity rule (bsdf_cases.parity): the kernel's error against the float64 evaluation is bounded by the error of the reference's own
float32 formulation on the same inputs, per tensor, with e(x) = |x - x64| / (|x64| + median |x64|):
max e(hip) <= 4 max e(twin32) and mean e(hip) <= 2 mean e(twin32).  The float32 side is the recorded float32 golden for the committed
cases and the torch twin in float32 (held to the goldens by tests/test_bsdf_cpu.py) for generated ones.
"""
import importlib
import os
import sys

import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bsdf_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
BSDFS = ("lambert", "frostbite_diffuse", "pbr_specular", "pbr_bsdf_lambert", "pbr_bsdf_frostbite")


def _ru():
    return importlib.import_module("3danimals_amd.model.render.renderutils")


def _run(name, inputs, g_out, device="cuda", dtype=torch.float32, **kw):
    xs = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in inputs]
    out = C.call_public(_ru(), name, xs, **kw)
    gs = torch.autograd.grad(out, xs, g_out.to(device=device, dtype=dtype).reshape(out.shape))
    return out.detach().cpu(), [g.cpu() for g in gs]


def _compare(what, name, inputs, g_out, twin32=None, x64=None, exclude_kinks=False):
    out, gs = _run(name, inputs, g_out)
    o64, g64 = x64 if x64 is not None else _run(name, inputs, g_out, device="cpu", dtype=torch.float64, use_python=True)
    o32, g32 = twin32 if twin32 is not None else _run(name, inputs, g_out, device="cpu", use_python=True)
    assert out.shape == o64.shape and out.dtype == torch.float32
    C.parity(f"{what} out", out, o32, o64)
    keep = None
    if exclude_kinks:
        bad = C.near_kink(name, inputs)
        assert float(bad.double().mean()) <= 0.01, (what, float(bad.double().mean()))
        keep = ~bad
    for i, (g, a, b) in enumerate(zip(gs, g32, g64)):
        assert g.shape == inputs[i].shape, (what, i, g.shape)
        full = keep is not None and tuple(b.shape[:-1]) == tuple(keep.shape)
        C.parity(f"{what} grad {i}", g, a, b, keep if full else None)
    return out, gs


@pytest.mark.parametrize("name,kind,seed", [c for c in C.GOLDEN_CASES if not c[0].startswith("_")])
def test_parity_on_the_recorded_cases(name, kind, seed):
    """Measured on an MI355X: per-pixel tensors max ratios 0.66 .. 2.9, mean ratios 0.95 .. 1.09; the reduced gradients of the 'bcast'
    cases (3 or 6 numbers, arithmetic carried in double) 0.006 .. 0.17."""
    g = golden(f"bsdf_{name}_{kind}.npz")
    n_in = sum(k.startswith("in_") for k in g.files)
    t = lambda k: torch.from_numpy(g[k])
    inputs = [t(f"in_{i}") for i in range(n_in)]
    _compare(f"{name} {kind} (golden)", name, inputs, t("g_out"), twin32=(t("out32"), [t(f"g32_{i}") for i in range(n_in)]),
             x64=(t("out64"), [t(f"g64_{i}") for i in range(n_in)]), exclude_kinks=kind == "wild")


@pytest.mark.parametrize("name", BSDFS)
@pytest.mark.parametrize("kind,seed", [("cond", 11), ("wild", 0), ("wild", 1), ("wild", 2)])
def test_parity_on_generated_sets(name, kind, seed):
    n = 16384
    inputs = C.make_inputs(name, kind, n, seed)
    g_out = torch.randn(C.out_shape(name, inputs), generator=torch.Generator().manual_seed(50 + seed))
    _compare(f"{name} {kind} seed {seed}", name, inputs, g_out, exclude_kinks=kind == "wild")


def test_kinks_hand_placed_on_either_side_of_every_clamp():
    """Values and gradients against the twin in float32 on the same device, with inputs a few ulps to either side of each kink: the
    subgradient taken must be the twin's (an element ON the wrong side would differ by the whole derivative, not by rounding)."""
    ru = _ru()
    z = torch.tensor([0.0, 0.0, 1.0])
    dirs = lambda c: torch.stack([torch.tensor([(1 - ci * ci) ** 0.5, 0.0, ci]) for ci in c])
    cs = [-1e-3, 0.0, 5e-5, 1e-4 - 1e-6, 1e-4 + 1e-6, 0.5, 1 - 1e-4 - 1e-6, 1 - 1e-4 + 1e-6, 1.0]
    wo = dirs(cs)
    n = len(cs)
    nrm, wi = z.expand(n, 3).contiguous(), dirs([0.7] * n)
    alpha = torch.tensor([[0.0], [0.0064 - 1e-5], [0.0064 + 1e-5], [0.5], [1 - 1e-5], [1 + 1e-5], [2.0], [0.3], [0.3]])
    col = torch.full((n, 3), 0.4)

    def both(fn, inputs):
        res = []
        for py in (False, True):
            xs = [t.cuda().requires_grad_(True) for t in inputs]
            out = fn(*xs, use_python=py)
            res.append((out.detach(), torch.autograd.grad(out.sum(), xs)))
        (o, g), (o2, g2) = res
        # Per element: 16 x the twin's own float32-against-float64 difference at the same point (two float32 evaluations in another
        # operation order differ by a few of those next to a clamp of the GGX denominator), plus 4 ulp of the element and 1e-6 of the
        # tensor's largest magnitude for terms that cancel to 0.  A WRONG subgradient differs by the whole derivative.  A row the
        # twin zeroes exactly (a branch not taken) must be zero exactly.
        x64 = [t.cuda().double().requires_grad_(True) for t in inputs]
        o64 = fn(*x64, use_python=True)
        g64 = torch.autograd.grad(o64.sum(), x64)
        for a, b, c in [(o, o2, o64.detach())] + list(zip(g, g2, g64)):
            lim = 16 * (b.double() - c).abs() + 4 * 2.0 ** -24 * c.abs() + 1e-6 * c.abs().max()
            bad = ((a.double() - c).abs() > lim).nonzero().tolist()
            assert not bad, [(r, a[tuple(r)].item(), b[tuple(r)].item(), c[tuple(r)].item()) for r in bad[:8]]
            dead = ((b == 0) & (c == 0)).all(-1)  # rows the twin zeroes as a whole: the branch not taken
            assert bool((a[dead] == 0).all())

    both(ru.lambert, [nrm, wo])
    both(ru.lambert, [wo, nrm])
    both(ru.frostbite_diffuse, [nrm, wi, wo, torch.full((n, 1), 0.6)])
    both(ru.frostbite_diffuse, [nrm, wo, wi, torch.full((n, 1), 0.6)])
    both(ru.pbr_specular, [col, nrm, wo, wi, torch.full((n, 1), 0.3)])
    both(ru.pbr_specular, [col, nrm, wi, wo, torch.full((n, 1), 0.3)])
    both(ru.pbr_specular, [col, nrm, wi, dirs([0.6] * n), alpha])
    both(ru.pbr_specular, [col, nrm, wi, wi, alpha])  # wo = wi: woDotH above its clamp, nDotH inside
    both(ru.pbr_specular, [col, nrm, nrm, nrm, alpha])  # every cosine above its clamp
    zero = torch.zeros(n, 3)
    both(ru.pbr_specular, [col, nrm, wi, -wi, alpha])  # wo + wi = 0: normalize at the 1e-12 floor
    for lobe in ("lambert", "frostbite"):
        arm = torch.cat([torch.full((n, 1), 0.2), alpha.clamp(min=0).sqrt(), torch.full((n, 1), 0.5)], -1)
        f = lambda *a, use_python: ru.pbr_bsdf(*a, bsdf=lobe, use_python=use_python)
        both(f, [col, arm, zero, nrm, wo * 2, wi * 3])
        both(f, [col, arm, zero, nrm, wi * 2, wo * 3])
        both(f, [col, arm, zero + 1, nrm, zero + 1, wi * 3])  # the view point ON the surface point: normalize of the zero vector


@pytest.mark.parametrize("lobe", ["lambert", "frostbite"])
def test_broadcast_inputs_and_strided_views(lobe):
    """Measured on an MI355X: the reduced gradients (3 or 9 numbers each; that backward carries its arithmetic in double) come out at
    0.006 .. 0.17 of the twin's float32 error, max and mean."""
    ru = _ru()
    name = "pbr_bsdf_" + lobe
    B, H, W = 3, 40, 56  # H W = 2240: three work-groups per segment, the last one partial
    gen = torch.Generator().manual_seed(5)
    cond = C.make_inputs(name, "bcast", 512, 3)
    ys, xs = torch.meshgrid(torch.linspace(-0.5, 0.5, H), torch.linspace(-0.5, 0.5, W), indexing="ij")
    pos = torch.stack([xs, ys, torch.zeros_like(xs)], -1)[None].repeat(B, 1, 1, 1) + 0.02 * (torch.rand(B, H, W, 3, generator=gen) - 0.5)
    nrm = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.1 * (torch.rand(B, H, W, 3, generator=gen) - 0.5), dim=-1)
    arm = torch.stack([torch.rand(B, H, W, generator=gen), 0.1 + 0.89 * torch.rand(B, H, W, generator=gen), torch.rand(B, H, W, generator=gen)], -1)
    kd = cond[0]
    view1, light1 = torch.tensor([2.0, 0.5, 2.0]).view(1, 1, 1, 3), cond[5]
    viewB = torch.tensor([[2.0, 0.5, 2.0], [1.8, -0.4, 2.2], [2.2, 0.1, 1.9]]).view(B, 1, 1, 3)
    g_out = torch.randn(B, H, W, 3, generator=gen)
    for what, view, light in (("[1,1,1,3]", view1, light1), ("[B,1,1,3]", viewB, light1.expand(B, 1, 1, 3).contiguous())):
        inputs = [kd, arm, pos, nrm, view, light]
        out, gs = _compare(f"{name} broadcast view/light {what}", name, inputs, g_out)
        assert [tuple(g.shape) for g in gs] == [tuple(t.shape) for t in inputs]
        # the same inputs expanded in memory: the broadcast gradients are the sums of the expanded case's, within the parity rule
        expanded = [t.expand(B, H, W, 3).contiguous() for t in inputs]
        _, ge64 = _run(name, expanded, g_out, device="cpu", dtype=torch.float64, use_python=True)
        _, ge32 = _run(name, expanded, g_out, device="cpu", use_python=True)
        oe, ge = _run(name, expanded, g_out)
        assert torch.equal(oe, out)
        for i in (0, 4, 5):
            C.parity(f"{name} {what} grad {i} vs summed expanded", gs[i], ge32[i].sum_to_size(inputs[i].shape), ge64[i].sum_to_size(inputs[i].shape))
        # bit-identical across two runs
        out2, gs2 = _run(name, inputs, g_out)
        assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(gs, gs2))
        # through non-contiguous views: every second column of a wider buffer, channels of a 4-channel buffer
        views = []
        for t in inputs:
            if t.shape[2] == W:
                buf = torch.zeros(B, H, 2 * W, 4)
                buf[:, :, ::2, :3] = t
                views.append(("strided", buf))
            else:
                views.append(("plain", t))
        xs_ = []
        for kind_, t in views:
            t = t.cuda()
            xs_.append((t[:, :, ::2, :3] if kind_ == "strided" else t).requires_grad_(True))
        assert not xs_[1].is_contiguous()
        o3 = ru.pbr_bsdf(*xs_, bsdf=lobe)
        g3 = torch.autograd.grad(o3, xs_, g_out.cuda())
        assert torch.equal(o3.cpu(), out) and all(torch.equal(a.cpu(), b) for a, b in zip(g3, gs))
    # a pattern that is not reduced in the launch: kd constant over the batch only ([1,H,W,3]), arm one value per row ([B,H,1,3])
    inputs = [torch.rand(1, H, W, 3, generator=gen), arm[:, :, :1].contiguous(), pos, nrm, viewB, light1]
    _compare(f"{name} inner broadcast", name, inputs, g_out)


@pytest.mark.parametrize("name", BSDFS)
def test_shapes(name):
    """Sizes around the wave and the tile: 1, 63, 64, 65 pixels, a [3,37,29] image, [2,1,1025].  The parity rule compares the max and the
    mean of two independent roundings and says little over a handful of numbers, so it is held on a 16,384-pixel conditioned set, and
    every small shape is the HEAD of that set: its result and gradients must be bit-identical to the corresponding rows of the large
    call (the kernels are per pixel).  That is exact, and it is what catches a wrong bound or tail."""
    big = C.make_inputs(name, "cond", 16384, 21)
    g_big = torch.randn(C.out_shape(name, big), generator=torch.Generator().manual_seed(3))
    out, gs = _compare(f"{name} 16384 (shape sweep)", name, big, g_big)
    for shape in [(1,), (63,), (64,), (65,), (3, 37, 29), (2, 1, 1025)]:
        n = 1
        for v in shape:
            n *= v
        head = lambda t: t[:n].reshape(*shape, t.shape[-1]).contiguous()
        o, g = _run(name, [head(t) for t in big], head(g_big))
        assert o.shape == (*shape, 3 if name.startswith("pbr") else 1) and torch.equal(o, head(out)), (name, shape)
        for i, (u, v) in enumerate(zip(g, gs)):
            assert torch.equal(u, head(v)), (name, shape, i)


@pytest.mark.parametrize("lobe", ["lambert", "frostbite"])
def test_expanded_views_are_read_in_place_and_get_gradients_of_their_shape(lobe):
    """expand() without contiguous() -- the ordinary way to pass a camera, a light or a constant colour: stride 0 along dimensions of
    size > 1.  The gradient of such a view has the VIEW's shape (autograd sums it into the base): light.expand(B,1,1,3) gets B rows,
    kd.expand(B,H,W,3) one row per pixel.  Values and gradients against the twin on the same views, and the bases' gradients."""
    ru = _ru()
    name = "pbr_bsdf_" + lobe
    B, H, W = 3, 40, 56
    gen = torch.Generator().manual_seed(9)
    cond = C.make_inputs(name, "bcast", 512, 3)
    ys, xs = torch.meshgrid(torch.linspace(-0.5, 0.5, H), torch.linspace(-0.5, 0.5, W), indexing="ij")
    pos = torch.stack([xs, ys, torch.zeros_like(xs)], -1)[None].repeat(B, 1, 1, 1) + 0.02 * (torch.rand(B, H, W, 3, generator=gen) - 0.5)
    nrm = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.1 * (torch.rand(B, H, W, 3, generator=gen) - 0.5), dim=-1)
    arm = torch.stack([torch.rand(B, H, W, generator=gen), 0.1 + 0.89 * torch.rand(B, H, W, generator=gen), torch.rand(B, H, W, generator=gen)], -1)
    bases = [cond[0], arm, pos, nrm, torch.tensor([2.0, 0.5, 2.0]).view(1, 1, 1, 3), cond[5]]
    g_out = torch.randn(B, H, W, 3, generator=gen)

    def run(device, dtype, **kw):
        leaves = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in bases]
        views = [leaves[0].expand(B, H, W, 3), leaves[1], leaves[2], leaves[3], leaves[4].expand(B, 1, 1, 3), leaves[5].expand(B, 1, 1, 3)]
        assert views[0].stride() == (0, 0, 0, 1) and views[5].stride(0) == 0 and views[4].stride(0) == 0
        out = ru.pbr_bsdf(*views, bsdf=lobe, **kw)
        gs = torch.autograd.grad(out, views + leaves, g_out.to(device=device, dtype=dtype))
        return out.detach().cpu(), [g.cpu() for g in gs]

    out, gs = run("cuda", torch.float32)
    o64, g64 = run("cpu", torch.float64, use_python=True)
    o32, g32 = run("cpu", torch.float32, use_python=True)
    C.parity(f"{name} expanded views out", out, o32, o64)
    want = [(B, H, W, 3)] * 4 + [(B, 1, 1, 3)] * 2 + [tuple(t.shape) for t in bases]
    assert [tuple(g.shape) for g in gs] == want
    for i, (g, a, b) in enumerate(zip(gs, g32, g64)):
        C.parity(f"{name} expanded views grad {i}", g, a, b)
    # the same values as with the bases passed as they are
    o_b, g_b = _run(name, bases, g_out)
    assert torch.equal(out, o_b)
    # lambert and image_loss with an expanded operand
    n1 = torch.nn.functional.normalize(torch.rand(1, 1, 3, generator=gen) + 0.2, dim=-1)
    wi = torch.nn.functional.normalize(torch.rand(H, W, 3, generator=gen) + 0.2, dim=-1)
    for f, args in ((lambda a, b, **kw: ru.lambert(a, b, **kw), (n1, wi)),
                    (lambda a, b, **kw: ru.image_loss(a, b, "mse", "log_srgb", **kw), (n1 * 3, wi * 2))):
        res = []
        for device, dtype, kw in (("cuda", torch.float32, {}), ("cpu", torch.float32, dict(use_python=True)), ("cpu", torch.float64, dict(use_python=True))):
            leaves = [t.to(device=device, dtype=dtype).requires_grad_(True) for t in args]
            view = leaves[0].expand(H, W, 3)  # (the gradient of the VIEW is the kernel's, one row per pixel; the leaf's is torch's sum of it)
            o = f(view, leaves[1], **kw)
            res.append([o.detach().cpu()] + [g.cpu() for g in torch.autograd.grad(o.sum(), [view, leaves[1], leaves[0]])])
        assert [tuple(g.shape) for g in res[0][1:]] == [(H, W, 3), (H, W, 3), (1, 1, 3)]
        for j in (1, 2):
            C.parity(f"expanded operand grad {j}", res[0][j], res[1][j], res[2][j])


def test_large_image_and_zero_elements():
    ru = _ru()
    B, H, W = 16, 512, 512
    gen = torch.Generator(device="cuda").manual_seed(1)
    full = [torch.rand(B, H, W, 3, device="cuda", generator=gen).requires_grad_(True) for _ in range(4)]
    view = torch.rand(B, 1, 1, 3, device="cuda", generator=gen).requires_grad_(True)
    light = torch.rand(1, 1, 1, 3, device="cuda", generator=gen).requires_grad_(True)
    xs = full + [view, light]
    out = ru.pbr_bsdf(*xs)
    go = torch.randn(out.shape, device="cuda", generator=gen)
    gs = torch.autograd.grad(out, xs, go)
    assert out.shape == (B, H, W, 3) and [g.shape for g in gs] == [x.shape for x in xs]
    sl = slice(5, 7)  # two images against the twin in float64
    x64 = [x.detach()[sl].double().requires_grad_(True) if x.shape[0] == B else x.detach().double().requires_grad_(True) for x in xs]
    o64 = ru.pbr_bsdf(*x64, use_python=True)
    g64 = torch.autograd.grad(o64, x64, go[sl].double())
    x32 = [x.detach().float().requires_grad_(True) for x in x64]
    o32 = ru.pbr_bsdf(*x32, use_python=True)
    g32 = torch.autograd.grad(o32, x32, go[sl])
    C.parity("pbr_bsdf [16,512,512] out (2 images)", out[sl].detach().cpu(), o32.detach().cpu(), o64.detach().cpu())
    bad = C.near_kink("pbr_bsdf_lambert", [x.detach().cpu() for x in x64])
    for i in range(4):
        C.parity(f"pbr_bsdf [16,512,512] grad {i} (2 images)", gs[i][sl].cpu(), g32[i].cpu(), g64[i].cpu(), ~bad)
    C.parity("pbr_bsdf [16,512,512] grad view (2 images)", gs[4][sl].cpu(), g32[4].cpu(), g64[4].cpu())
    assert float(bad.double().mean()) <= 0.01
    # light_pos [1,1,1,3] sums over all 16 images: against the twin on the whole batch, float32 and float64 on the GPU
    for dtype, device, store in ((torch.float32, "cuda", g32), (torch.float64, "cuda", g64)):
        xw = [x.detach().to(device=device, dtype=dtype).requires_grad_(True) for x in xs]
        ow = ru.pbr_bsdf(*xw, use_python=True)
        store_light, = torch.autograd.grad(ow, [xw[5]], go.to(device=device, dtype=dtype))
        if dtype == torch.float32:
            l32 = store_light.cpu()
        else:
            l64 = store_light.cpu()
        del xw, ow
    C.parity("pbr_bsdf [16,512,512] grad light", gs[5].cpu(), l32, l64)
    L = importlib.import_module("3danimals_amd._lib")
    with L.KernelTimer() as timer:
        for name in BSDFS:
            inputs = [t.reshape(0, 5, t.shape[-1]) for t in C.make_inputs(name, "wild", 0, 0)]
            xs = [t.cuda().requires_grad_(True) for t in inputs]
            out = C.call_public(ru, name, xs)
            assert out.shape == (0, 5, 3 if name.startswith("pbr") else 1)
            gs = torch.autograd.grad(out.sum(), xs)
            assert all(g.shape == x.shape for g, x in zip(gs, xs))
        assert torch.isnan(ru.image_loss(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, device="cuda")))
    assert timer.summary() == {}  # zero elements: no call into the library, no launch


@pytest.mark.parametrize("loss", C.LOSSES)
@pytest.mark.parametrize("tm", C.TONEMAPS)
def test_image_loss(loss, tm):
    ru = _ru()
    g = golden(f"bsdf_image_loss_{loss}_{tm}.npz")
    t = lambda k: torch.from_numpy(g[k])
    cases = [("golden", t("in_0"), t("in_1"), (t("out32"), [t("g32_0"), t("g32_1")]), (t("out64"), [t("g64_0"), t("g64_1")]))]
    img, target = C.make_images(4 * 96 * 100 * 3, 13)
    cases.append(("generated [4,96,100,3]", img.reshape(4, 96, 100, 3), target.reshape(4, 96, 100, 3), None, None))
    for what, a, b, twin32, x64 in cases:
        go = torch.tensor(1.5)
        f = lambda x, y, **kw: ru.image_loss(x, y, loss, tm, **kw)

        def run(device, dtype, **kw):
            xs = [a.to(device=device, dtype=dtype).requires_grad_(True), b.to(device=device, dtype=dtype).requires_grad_(True)]
            out = f(*xs, **kw)
            return out.detach().cpu(), [v.cpu() for v in torch.autograd.grad(out, xs, go.to(device=device, dtype=dtype))]

        out, gs = run("cuda", torch.float32)
        o64, g64 = x64 or run("cpu", torch.float64, use_python=True)
        o32, g32 = twin32 or run("cpu", torch.float32, use_python=True)
        assert out.shape == () and out.dtype == torch.float32
        # the scalar: one number, so the rule's right-hand side can be 0 by luck (the twin's pairwise sum landing on the float64 value);
        # the floor is 4 ulp of the result whatever n is -- the kernel carries the sum in double and rounds once
        err, ref = abs(float(out) - float(o64)), abs(float(o32) - float(o64))
        print(f"image_loss {loss} {tm} {what}: |hip - x64| {err:.3e}, |twin32 - x64| {ref:.3e}, value {float(o64):.6e}")
        assert err <= max(4 * ref, 4 * 2.0 ** -24 * abs(float(o64)))
        for i in range(2):
            C.parity(f"image_loss {loss} {tm} {what} grad {i}", gs[i], g32[i], g64[i])
        out2, gs2 = run("cuda", torch.float32)
        assert torch.equal(out, out2) and all(torch.equal(u, v) for u, v in zip(gs, gs2))
    # outside the tone map's clamp the gradient is 0; at the bounds it passes; the values are the twin's
    if tm == "log_srgb":
        a = torch.tensor([70000.0, 65535.0, 65536.0, -1.0, -1e-6, 0.0, 1e-3, 3.14e-3, 2.0], device="cuda").requires_grad_(True)
        b = torch.tensor([1.0, 2.0, 3.0, 0.5, 0.25, 1e-4, 70000.0, -2.0, 2.5], device="cuda").requires_grad_(True)
        res = []
        for py in (False, True):
            out = ru.image_loss(a, b, loss, tm, use_python=py)
            res.append((out.detach(), torch.autograd.grad(out, [a, b])))
        assert torch.allclose(res[0][0], res[1][0], rtol=1e-5)
        for u, v in zip(res[0][1], res[1][1]):
            assert torch.allclose(u, v, rtol=1e-4, atol=1e-9), (u, v)
        ga, gb = res[0][1]
        assert float(ga[0]) == 0 and float(ga[2]) == 0 and float(ga[3]) == 0 and float(ga[4]) == 0 and float(gb[6]) == 0 and float(gb[7]) == 0
        assert float(ga[1].abs()) > 0 and float(ga[5].abs()) > 0


@pytest.mark.parametrize("loss,tm", [("l1", "none"), ("relmse", "log_srgb")])
def test_image_loss_on_layouts_the_contiguous_kernel_does_not_take(loss, tm):
    """Contiguous, 16-byte aligned images of 4 m elements run the 16-byte-per-lane kernel; everything else the strided one: an odd
    element count, a view that starts one float into its buffer, every second column of a wider image, and a target broadcast over
    the batch, over the pixels ([B,1,1,3]: its gradient is reduced in the launch) and over the channels.  Values within 4 ulp (or 4 x
    the twin's error), gradients within the parity rule, gradient shapes the inputs'."""
    ru = _ru()
    B, H, W = 3, 33, 37  # 10,989 elements per image set: odd
    img, target = (t.reshape(-1)[: B * H * W * 3].reshape(B, H, W, 3) for t in C.make_images(4 * 9000, 17))
    buf_a, buf_b = torch.zeros(img.numel() + 1), torch.zeros(B, H, 2 * W, 3)
    buf_a[1:] = img.reshape(-1)
    buf_b[:, :, ::2] = target
    layouts = {
        "odd n": lambda a, b: (a, b),
        "misaligned": lambda a, b: (buf_a.to(a)[1:].view(B, H, W, 3), b),
        "strided": lambda a, b: (a, buf_b.to(b)[:, :, ::2]),
        "target [1,H,W,3]": lambda a, b: (a, b[:1]),
        "target [B,1,1,3]": lambda a, b: (a, b[:, :1, :1]),
        "target [B,H,W,1]": lambda a, b: (a, b[..., :1]),
    }
    for what, make in layouts.items():
        res = []
        for device, dtype, kw in (("cuda", torch.float32, {}), ("cpu", torch.float32, dict(use_python=True)), ("cpu", torch.float64, dict(use_python=True))):
            a, b = make(img.to(device=device, dtype=dtype), target.to(device=device, dtype=dtype))
            a, b = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
            if device == "cuda" and what in ("misaligned", "strided"):
                assert a.data_ptr() % 16 != 0 or not b.is_contiguous()
            out = ru.image_loss(a, b, loss, tm, **kw)
            ga, gb = torch.autograd.grad(out, [a, b])
            assert ga.shape == a.shape and gb.shape == b.shape
            res.append((float(out), ga.cpu(), gb.cpu()))
        (o, ga, gb), (o32, a32, b32), (o64, a64, b64) = res
        print(f"image_loss {loss} {tm} {what}: |hip - x64| {abs(o - o64):.3e}, |twin32 - x64| {abs(o32 - o64):.3e}")
        assert abs(o - o64) <= max(4 * abs(o32 - o64), 4 * 2.0 ** -24 * abs(o64)), what
        C.parity(f"image_loss {loss} {tm} {what} grad img", ga, a32, a64)
        C.parity(f"image_loss {loss} {tm} {what} grad target", gb, b32, b64)


def test_fallbacks_and_anomaly_mode():
    ru = _ru()
    ops = importlib.import_module("3danimals_amd.ops")
    L = importlib.import_module("3danimals_amd._lib")
    inputs = [t.cuda() for t in C.make_inputs("pbr_bsdf_lambert", "cond", 256, 1)]
    with L.KernelTimer() as t:
        ru.pbr_bsdf(*inputs)
        ru.image_loss(inputs[0], inputs[1])
    assert set(t.summary()) == {"a3d_bsdf_fwd[pbr_bsdf]", "a3d_image_loss_fwd[0]"}
    with L.KernelTimer() as t:
        o64 = ru.pbr_bsdf(*[x.double() for x in inputs])  # float64 on the GPU: the twin
        opy = ru.pbr_bsdf(*inputs, use_python=True)
        ru.image_loss(inputs[0].double(), inputs[1].double(), "mse")
        ru.lambert(inputs[3].cpu(), inputs[3].cpu())
        for f in (ru._fresnel_shlick, ru._masking_smith):
            f(inputs[0][:, :1], inputs[1][:, :1], inputs[2][:, :1])
    assert t.summary() == {} and o64.dtype == torch.float64 and opy.dtype == torch.float32
    bad = [x.clone() for x in inputs]
    bad[2][3, 1] = float("nan")
    with torch.autograd.detect_anomaly(check_nan=False):
        with pytest.raises(AssertionError, match="Output of pbr_bsdf contains inf or NaN"):
            ru.pbr_bsdf(*bad)
        with pytest.raises(AssertionError, match="Output of image_loss contains inf or NaN"):
            ru.image_loss(bad[2], inputs[2])
    with pytest.raises(ValueError, match="float32"):
        ops.bsdf("lambert", (inputs[0].double(), inputs[1].double()))


def test_recover_a_constant_albedo_with_adam():
    """End to end: a constant kd [1,1,1,3] recovered from a pbr_bsdf-shaded target under image_loss(l1, log_srgb) with Adam.  The loss
    trajectory of the HIP path against the twin's on the same GPU, bounded by the parity rule's margin (4 x) over the difference between
    the twin's float32 and float64 trajectories over the same steps."""
    ru = _ru()
    cond = C.make_inputs("pbr_bsdf_lambert", "bcast", 512, 3)
    rest = [t.cuda() for t in cond[1:]]
    target = ru.pbr_bsdf(torch.tensor([0.7, 0.4, 0.2], device="cuda").view(1, 1, 1, 3), *rest, use_python=True)

    def trajectory(dtype, use_python):
        kd = torch.full((1, 1, 1, 3), 0.5, device="cuda", dtype=dtype, requires_grad=True)
        opt = torch.optim.Adam([kd], lr=0.02)
        r = [t.to(dtype) for t in rest]
        tgt = target.to(dtype)
        losses = []
        for _ in range(60):
            opt.zero_grad()
            loss = ru.image_loss(ru.pbr_bsdf(kd, *r, use_python=use_python), tgt, "l1", "log_srgb", use_python=use_python)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        return torch.tensor(losses, dtype=torch.float64), kd.detach().double().cpu().reshape(3)

    hip, kd_hip = trajectory(torch.float32, False)
    t32, _ = trajectory(torch.float32, True)
    t64, _ = trajectory(torch.float64, True)
    d_hip, d_twin = float((hip - t64).abs().max()), float((t32 - t64).abs().max())
    print(f"adam: loss {float(hip[0]):.4e} -> {float(hip[-1]):.4e}; max |hip - twin64| {d_hip:.3e}, max |twin32 - twin64| {d_twin:.3e}, ratio {d_hip / max(d_twin, 1e-300):.3f}")
    assert float(hip[-1]) < 0.2 * float(hip[0]) and float((kd_hip - torch.tensor([0.7, 0.4, 0.2], dtype=torch.float64)).abs().max()) < 0.05
    assert d_hip <= 4 * d_twin
