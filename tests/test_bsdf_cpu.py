"""Shading BSDFs and HDR image loss without a GPU: the public names and signatures, the torch twins in float64 against the reference's
float64 goldens, the op and loss codes of ops.py against include/a3d_bsdf.h, argument validation before any
launch, the call plan of ops.bsdf (merged dimensions, strides, runs), and known answers of the twins."""
import ctypes
import importlib
import inspect
import json
import math
import os
import sys

import pytest
import torch

from conftest import GOLDEN, golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check as A  # noqa: E402
import bsdf_cases as C  # noqa: E402

NAMES = ("lambert", "frostbite_diffuse", "pbr_specular", "pbr_bsdf", "image_loss", "_fresnel_shlick", "_ndf_ggx", "_lambda_ggx", "_masking_smith")
ENTRIES = ("a3d_bsdf_fwd", "a3d_bsdf_bwd", "a3d_image_loss_fwd", "a3d_image_loss_bwd")


def _ru():
    return importlib.import_module("3danimals_amd.model.render.renderutils")


def test_the_nine_names_have_the_recorded_signatures():
    ru = _ru()
    rec = json.load(open(os.path.join(GOLDEN, "overlay_interface.json")))["modules"]["model.render.renderutils"]["callables"]
    for name in NAMES:
        fn = getattr(ru, name)
        got = [[p.name, p.kind.name, p.default is not inspect.Parameter.empty, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(fn).parameters.values()]
        assert got == rec[name]["params"], (name, got, rec[name]["params"])
    assert "not provided" not in ru.__doc__


@pytest.mark.parametrize("name,kind,seed", C.GOLDEN_CASES)
def test_float64_twin_reproduces_the_float64_goldens(name, kind, seed):
    """Values and gradients to rounding: 1e-12 relative to the tensor's largest magnitude (the level test_envlight_cpu.py uses for a
    float64 restatement).  The recorded inputs are what bsdf_cases.make_inputs builds."""
    ru = _ru()
    g = golden(f"bsdf_{name.lstrip('_')}_{kind}.npz")
    built = C.make_inputs(name, kind, C.GOLDEN_PIXELS, seed)
    n_in = len(built)
    for i in range(n_in):
        assert torch.equal(torch.from_numpy(g[f"in_{i}"]), built[i]), (name, kind, i)
    xs = [torch.from_numpy(g[f"in_{i}"]).double().requires_grad_(True) for i in range(n_in)]
    out = C.call_public(ru, name, xs, use_python=True)
    want = torch.from_numpy(g["out64"])
    assert out.shape == want.shape and out.dtype == torch.float64
    assert float((out.detach() - want).abs().max()) <= 1e-12 * float(want.abs().max()), (name, kind)
    gs = torch.autograd.grad(out, xs, torch.from_numpy(g["g_out"]).double().reshape(out.shape))
    for i, gi in enumerate(gs):
        w = torch.from_numpy(g[f"g64_{i}"])
        assert gi.shape == w.shape and float((gi - w).abs().max()) <= 1e-12 * max(float(w.abs().max()), 1e-300), (name, kind, i)
    # the float32 twin is the recorded float32 evaluation (same operations in the same order)
    x32 = [torch.from_numpy(g[f"in_{i}"]) for i in range(n_in)]
    x32 = [t.requires_grad_(True) for t in x32]
    o32 = C.call_public(ru, name, x32, use_python=True)
    g32 = torch.autograd.grad(o32, x32, torch.from_numpy(g["g_out"]).reshape(o32.shape))
    # (bit-identical where the goldens were recorded; 4 ulp of the largest magnitude for another CPU's vector width)
    for got, key in [(o32.detach(), "out32")] + [(gi, f"g32_{i}") for i, gi in enumerate(g32)]:
        w = torch.from_numpy(g[key])
        assert float((got - w).abs().max()) <= 4 * 2.0 ** -24 * float(w.abs().max()), (name, kind, key)


@pytest.mark.parametrize("loss", C.LOSSES)
@pytest.mark.parametrize("tm", C.TONEMAPS)
def test_float64_image_loss_twin_reproduces_the_goldens(loss, tm):
    ru = _ru()
    g = golden(f"bsdf_image_loss_{loss}_{tm}.npz")
    a, b = (torch.from_numpy(g[f"in_{i}"]).double().requires_grad_(True) for i in range(2))
    out = ru.image_loss(a, b, loss, tm, use_python=True)
    assert out.shape == () and float(out) == pytest.approx(float(g["out64"]), rel=1e-12)
    ga, gb = torch.autograd.grad(out, [a, b], torch.tensor(float(g["g_out"]), dtype=torch.float64))
    for got, key in ((ga, "g64_0"), (gb, "g64_1")):
        w = torch.from_numpy(g[key])
        assert float((got - w).abs().max()) <= 1e-12 * float(w.abs().max())
    assert bool(((a - b).abs() >= 1e-3 * 0.999).all()) and float(a.min()) >= 0.05  # the conditioning the builder promises


def test_second_header_matches_the_second_table_and_the_first_surface_is_untouched():
    """What is this surface's own (tests/test_abi_cpu.py holds its table, BsdfDesc and the constants to include/a3d_bsdf.h as it does
    for every surface): the entry points the tests below call, and the op / loss codes of ops.py against the header's macros."""
    assert set(ENTRIES) < set(A.prototypes("a3d_bsdf.h"))
    macros = A.defines("a3d_bsdf.h")
    ops = importlib.import_module("3danimals_amd.ops")
    for name, (code, _, _) in ops.BSDF_OPS.items():
        macro = {"lambert": "LAMBERT", "frostbite_diffuse": "FROSTBITE", "pbr_specular": "PBR_SPECULAR", "pbr_bsdf": "PBR", "image_loss": "IMAGE_LOSS"}[name]
        assert macros["A3D_BSDF_" + macro] == code
    for name, code in ops.IMAGE_LOSSES.items():
        assert macros["A3D_LOSS_" + name.upper()] == code


def _desc(L, **kw):
    fake = 0x1000  # non-NULL, never dereferenced
    d = L.BsdfDesc(size=ctypes.sizeof(L.BsdfDesc), op=3, ndim=1, seg=8, out=fake, scratch=fake, g_out=fake)
    d.shape[0] = 8
    for i in range(6):
        getattr(d, "in")[i] = fake
        d.stride[4 * i] = 3
        d.cstride[i] = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_a_short_or_invalid_descriptor_is_refused_before_anything_is_launched():
    """None of the pointers below is ever dereferenced and nothing is launched (this runs without a GPU)."""
    L = importlib.import_module("3danimals_amd._lib")
    lib = L.lib()

    def refused(name, d, *words):
        assert getattr(lib, name)(ctypes.byref(d), None) == -1, name
        msg = lib.a3d_last_error().decode()
        assert "invalid argument" in msg and name in msg and all(w in msg for w in words), (name, msg)

    for name in ENTRIES:
        op = 4 if "image_loss" in name else 3
        refused(name, _desc(L, op=op, size=ctypes.sizeof(L.BsdfDesc) - 4), "size")
        refused(name, _desc(L, op=17), "op")  # unknown op (and a BSDF code for the loss, a loss code for the BSDFs)
        refused(name, _desc(L, op=4 if op == 3 else 3), "op")
        refused(name, _desc(L, op=op, ndim=0), "ndim")
        refused(name, _desc(L, op=op, ndim=5), "ndim")
        d = _desc(L, op=op)
        d.shape[0] = -8
        refused(name, d, "shape")
        refused(name, _desc(L, op=op, seg=3), "seg")  # does not divide the pixel count
        refused(name, _desc(L, op=op, seg=0), "seg")
        d = _desc(L, op=op)
        d.stride[0] = -3
        refused(name, d, "stride")
        d = _desc(L, op=op)
        getattr(d, "in")[1] = None
        refused(name, d, "in[1]")
    refused("a3d_image_loss_fwd", _desc(L, op=4, variant=8), "variant")
    refused("a3d_bsdf_fwd", _desc(L, op=3, variant=2), "variant")
    refused("a3d_bsdf_fwd", _desc(L, out=None), "out")
    refused("a3d_bsdf_bwd", _desc(L, g_out=None), "g_out")
    d = _desc(L)
    d.g_mode[0] = 3
    refused("a3d_bsdf_bwd", d, "gmode")
    d = _desc(L)
    d.g_mode[0] = 1  # a wanted gradient without a buffer
    refused("a3d_bsdf_bwd", d, "g_in")
    d = _desc(L)  # a reduced gradient of an input that is NOT constant over the run
    d.g_mode[0], d.seg_div[0], d.g_in[0], d.g_final[0] = 2, 1, 0x1000, 0x1000
    refused("a3d_bsdf_bwd", d, "in[0]", "REDUCE", "constant over")
    assert lib.a3d_bsdf_rows(ctypes.byref(_desc(L, size=8))) == -1 and lib.a3d_bsdf_rows(ctypes.byref(_desc(L, seg=3))) == -1
    d = _desc(L, ndim=2, seg=3000)
    d.shape[0], d.shape[1] = 5, 3000
    assert lib.a3d_bsdf_rows(ctypes.byref(d)) == 5 * 3
    # zero pixels: accepted, nothing to do
    d = _desc(L)
    d.shape[0] = 0
    assert lib.a3d_bsdf_fwd(ctypes.byref(d), None) == 0


def test_call_plan_merges_dimensions_and_finds_the_runs():
    ops = importlib.import_module("3danimals_amd.ops")
    L = importlib.import_module("3danimals_amd._lib")
    B, H, W = 3, 20, 24
    full = [torch.zeros(B, H, W, 3) for _ in range(4)]
    view, light = torch.zeros(B, 1, 1, 3), torch.zeros(1, 1, 1, 3)
    p = ops._BsdfPlan("pbr_bsdf", (full[0], full[1], full[2], full[3], view, light))
    assert p.shape == [B, H * W] and p.strides[0] == [H * W * 3, 3] and p.strides[4] == [3, 0] and p.strides[5] == [0, 0]
    assert p.run == [None, None, None, None, H * W, B * H * W] and p.seg == H * W and p.rows() == B * 1 and p.lead == (B, H, W)
    d = p.desc()
    assert L.lib().a3d_bsdf_rows(ctypes.byref(d)) == p.rows()
    # everything contiguous and full: one dimension, one segment
    p = ops._BsdfPlan("pbr_bsdf", tuple(full + full[:2]))
    assert p.shape == [B * H * W] and p.seg == B * H * W and p.run == [None] * 6 and p.rows() == math.ceil(B * H * W / L.BSDF_TILE)
    # a non-contiguous view keeps its strides; a constant colour [1,1,1,3] is a run of everything; a [1,H,W,3] input is summed by torch
    wide = torch.zeros(B, H, 2 * W, 3)[:, :, ::2]
    p = ops._BsdfPlan("pbr_bsdf", (light, wide, full[0], torch.zeros(1, H, W, 3), view, light))
    assert p.shape == [B, H * W] and p.strides[1] == [H * 2 * W * 3, 6] and p.strides[3] == [0, 3]  # (H and W still merge: 2 W 3 = 6 W)
    rows = torch.zeros(B, H + 1, W, 3)[:, 1:]
    assert ops._BsdfPlan("lambert", (rows, torch.zeros(B, H, 2 * W, 3)[:, :, :W])).shape == [B, H, W]
    assert p.run == [B * H * W, None, None, None, H * W, B * H * W] and p.seg == H * W
    # short runs are not reduced in the launch; channel broadcast is a channel stride of 0
    p = ops._BsdfPlan("pbr_specular", (torch.zeros(4, 1, 1), torch.zeros(4, 8, 3), torch.zeros(4, 8, 3), torch.zeros(4, 8, 3), torch.zeros(4, 8, 1)))
    assert p.run[0] is None and p.cstrides[0] == 0 and p.seg == 32
    p = ops._BsdfPlan("lambert", (torch.zeros(0, 3), torch.zeros(0, 3)))
    assert p.n == 0
    with pytest.raises(ValueError, match="last dimension"):
        ops._BsdfPlan("lambert", (torch.zeros(4, 2), torch.zeros(4, 3)))
    with pytest.raises(L.A3DError, match="no CPU fallback"):
        ops.bsdf("lambert", (torch.zeros(4, 3), torch.zeros(4, 3)))
    with pytest.raises(L.A3DError, match="no CPU fallback"):
        ops.image_loss(torch.zeros(4, 3), torch.zeros(4, 3))


def test_known_answers_of_the_twins():
    ru = _ru()
    n = torch.nn.functional.normalize(torch.randn(50, 3, generator=torch.Generator().manual_seed(0)).double(), dim=-1)
    assert torch.allclose(ru.lambert(n, n, use_python=True), torch.full((50, 1), 1 / math.pi, dtype=torch.float64), rtol=1e-14)
    assert ru.lambert(n, n).shape == (50, 1) and ru.frostbite_diffuse(n, n, n, torch.rand(50, 1).double()).shape == (50, 1)  # (CPU: the twin)
    # pbr_specular is 0 when either cosine is <= 1e-4
    z = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64)
    graze = torch.tensor([[math.sqrt(1 - 1e-8), 0.0, 1e-4]], dtype=torch.float64)
    up = torch.tensor([[0.6, 0.0, 0.8]], dtype=torch.float64)
    col, alpha = torch.full((1, 3), 0.5, dtype=torch.float64), torch.full((1, 1), 0.3, dtype=torch.float64)
    assert float(ru.pbr_specular(col, z, graze, up, alpha, use_python=True).abs().max()) == 0.0
    assert float(ru.pbr_specular(col, z, up, graze, alpha, use_python=True).abs().max()) == 0.0
    assert float(ru.pbr_specular(col, z, up, -up, alpha, use_python=True).abs().max()) == 0.0
    assert float(ru.pbr_specular(col, z, up, up, alpha, use_python=True).min()) > 0.0
    # Schlick at normal incidence: the cosine is clamped to 1 - 1e-4, so f0 + (f90 - f0) 1e-20 -- f0 in float32
    f0, f90 = torch.tensor([0.04, 0.5]), torch.tensor([1.0, 1.0])
    assert torch.equal(ru._fresnel_shlick(f0, f90, torch.ones(2)), f0)
    zero = torch.zeros(2, dtype=torch.float64)  # (with f0 = 0 the 1e-20 is not rounded away)
    got = ru._fresnel_shlick(zero, torch.tensor([1.0, 3.0], dtype=torch.float64), torch.ones(2, dtype=torch.float64), use_python=True)
    assert torch.allclose(got, torch.tensor([1e-20, 3e-20], dtype=torch.float64), rtol=1e-9, atol=0)
    # Smith masking of two normal-incidence cosines: tan^2 = (1 - c^2) / c^2 at c = 1 - 1e-4
    a2 = torch.tensor([0.25], dtype=torch.float64)
    c = 1 - 1e-4
    lam = 0.5 * (math.sqrt(1 + 0.25 * (1 - c * c) / (c * c)) - 1)
    one = torch.ones(1, dtype=torch.float64)
    assert float(ru._masking_smith(a2, one, one, use_python=True)) == pytest.approx(1 / (1 + 2 * lam), rel=1e-14)
    assert float(ru._lambda_ggx(a2, one)) == pytest.approx(lam, rel=1e-12) and float(ru._ndf_ggx(one, one)) == pytest.approx(1 / math.pi, rel=1e-12)
    # image_loss(x, x) = 0 in all eight modes; zero gradient under MSE
    x = (torch.rand(4, 8, 8, 3, generator=torch.Generator().manual_seed(1)) * 5).double().requires_grad_(True)
    for loss in C.LOSSES:
        for tm in C.TONEMAPS:
            assert float(ru.image_loss(x, x.detach().clone(), loss, tm, use_python=True)) == 0.0, (loss, tm)
    g, = torch.autograd.grad(ru.image_loss(x, x.detach().clone(), "mse", "log_srgb", use_python=True), x)
    assert float(g.abs().max()) == 0.0
    assert float(ru.image_loss(x, x.detach() + 1, "nonsense")) == pytest.approx(1.0, rel=1e-12)  # any other name is l1, as in the reference


def test_wild_seeds_keep_the_kink_share_below_one_percent():
    """The seeds the GPU test uses for its wild sets (torch.rand everything): the share of pixels within 1e-5 of a kink."""
    for name in ("lambert", "frostbite_diffuse", "pbr_specular", "pbr_bsdf_lambert", "pbr_bsdf_frostbite"):
        for seed in (0, 1, 2):
            share = float(C.near_kink(name, C.make_inputs(name, "wild", 16384, seed)).double().mean())
            assert share <= 0.01, (name, seed, share)
