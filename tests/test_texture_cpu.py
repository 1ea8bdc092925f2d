"""Texture sampling without a GPU: the ABI surface of csrc/texture.hip, the descriptor's size check, the mip-chain size rule, the custom
stack's validation, the shim surface, and closed forms of the float64 restatement (tests/texture_ref.py)."""
import ctypes
import importlib
import math
import os
import re
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_ref as R  # noqa: E402

ENTRIES = ("a3d_texture_fwd", "a3d_texture_bwd", "a3d_texture_mip_fwd", "a3d_texture_mip_bwd")


def test_texture_prototypes_are_declared_and_bound():
    L = importlib.import_module("3danimals_amd._lib")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "a3d.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.SIGNATURES, name
        assert hasattr(L.lib(), name), name
    assert L.ABI_VERSION == 405


def test_tex_desc_matches_the_header_field_for_field():
    L = importlib.import_module("3danimals_amd._lib")
    header = open(os.path.join(ROOT, "include", "a3d.h")).read()  # (field for field: tests/test_abi_cpu.py; here the known answers)
    assert re.search(r"#define A3D_TEX_MAX_LEVELS 16\b", header)
    assert ctypes.sizeof(L.TexDesc) == 4 * 6 + 4 * 32 + 8 * 32 + 0


def test_a_short_tex_desc_is_refused_before_anything_is_launched():
    """A descriptor shorter than the library's (a caller built against an older header) is refused with A3D_EINVAL by all four entry
    points before a pointer is touched (none of the pointers below is ever dereferenced; no GPU needed)."""
    L = importlib.import_module("3danimals_amd._lib")
    lib = L.lib()
    fake = 0x1000
    d = L.TexDesc(size=ctypes.sizeof(L.TexDesc) - 4, C=3, tex_batch=1, filter=1, boundary=0, levels=1)
    d.height[0] = d.width[0] = 4
    d.level[0] = fake
    calls = {
        "a3d_texture_fwd": lambda: lib.a3d_texture_fwd(ctypes.byref(d), fake, None, None, 1, 4, 4, fake, None),
        "a3d_texture_bwd": lambda: lib.a3d_texture_bwd(ctypes.byref(d), fake, fake, None, None, 1, 4, 4, fake, None, None, None),
        "a3d_texture_mip_fwd": lambda: lib.a3d_texture_mip_fwd(ctypes.byref(d), None),
        "a3d_texture_mip_bwd": lambda: lib.a3d_texture_mip_bwd(ctypes.byref(d), None),
    }
    for name, fn in calls.items():
        assert fn() == -1, name
        msg = lib.a3d_last_error().decode()
        assert "size" in msg and "invalid argument" in msg and name in msg, (name, msg)
    # a full-size descriptor with a bad stack is refused too (the halving rule of the mip entry points)
    d.size, d.levels = ctypes.sizeof(L.TexDesc), 2
    d.height[1], d.width[1], d.level[1] = 3, 2, fake
    assert lib.a3d_texture_mip_fwd(ctypes.byref(d), None) == -1 and "halving rule" in lib.a3d_last_error().decode()


def test_mip_chain_size_rule():
    ops = importlib.import_module("3danimals_amd.ops")
    assert ops.texture_mip_sizes(8, 8) == [(8, 8), (4, 4), (2, 2), (1, 1)]
    assert ops.texture_mip_sizes(8, 2) == [(8, 2), (4, 1), (2, 1), (1, 1)]
    assert ops.texture_mip_sizes(1, 16) == [(1, 16), (1, 8), (1, 4), (1, 2), (1, 1)]
    assert ops.texture_mip_sizes(12, 8) == [(12, 8), (6, 4), (3, 2)]  # stops at the first odd dimension > 1
    assert ops.texture_mip_sizes(5, 4) == [(5, 4)]
    assert ops.texture_mip_sizes(1, 1) == [(1, 1)]
    assert ops.texture_mip_sizes(64, 64, max_mip_level=2) == [(64, 64), (32, 32), (16, 16)]
    assert ops.texture_mip_sizes(64, 64, max_mip_level=0) == [(64, 64)]
    assert len(ops.texture_mip_sizes(1 << 20, 1)) == ops.TEX_MAX_LEVELS
    for h, w, mx in ((8, 8, None), (12, 8, None), (1, 16, 2), (6, 6, None)):
        assert ops.texture_mip_sizes(h, w, mx) == R.mip_sizes(h, w, mx)
    # the restatement's chain has those sizes and is a box mean
    t = torch.arange(2 * 4 * 2 * 1, dtype=torch.float64).reshape(2, 4, 2, 1)
    chain = R.mip_chain(t)
    assert [tuple(c.shape[1:3]) for c in chain] == [(4, 2), (2, 1), (1, 1)]
    assert torch.equal(chain[1][0, 0, 0], t[0, :2, :2].mean().reshape(1)) and torch.allclose(chain[2][1], t[1].mean().reshape(1, 1, 1))


def test_malformed_custom_mip_stack_raises_value_error():
    ops = importlib.import_module("3danimals_amd.ops")
    tex, uv = torch.zeros(1, 8, 8, 3), torch.zeros(1, 2, 2, 2)
    for bad in ([torch.zeros(1, 4, 3, 3)], [torch.zeros(1, 4, 4, 3), torch.zeros(1, 1, 1, 3)], [torch.zeros(1, 4, 4, 2)],
                [torch.zeros(1, 4, 4, 3)] * 4, [torch.zeros(2, 4, 4, 3)]):
        with pytest.raises(ValueError):
            ops.texture(tex, uv, mip=bad, filter_mode="linear-mipmap-linear")
    with pytest.raises(ValueError):  # cube levels must be [Bt, 6, S, S, C]
        ops.texture(torch.zeros(1, 6, 8, 8, 3), torch.ones(1, 1, 1, 3), mip=[torch.zeros(1, 6, 4, 2, 3)], filter_mode="linear-mipmap-linear",
                    boundary_mode="cube")
    with pytest.raises(ValueError):
        ops.texture(tex, uv, uv_da=torch.zeros(1, 2, 2, 3))


def test_shim_texture_surface():
    sys.path.insert(0, os.path.join(ROOT, "3danimals_amd", "shims"))
    try:
        dr = importlib.import_module("nvdiffrast.torch")
        assert callable(dr.texture_construct_mip)
        with pytest.raises(NotImplementedError, match="GPU"):
            dr.texture_construct_mip(torch.zeros(1, 8, 8, 3))
        with pytest.raises(NotImplementedError, match="GPU"):
            dr.texture(torch.zeros(1, 6, 2, 2, 1), torch.ones(1, 1, 1, 3), boundary_mode="cube")
        with pytest.raises(NotImplementedError, match="GPU"):
            dr.texture(torch.zeros(1, 8, 8, 1), torch.zeros(1, 1, 1, 2), mip_level_bias=torch.zeros(1, 1, 1))
    finally:
        sys.path.remove(os.path.join(ROOT, "3danimals_amd", "shims"))


def test_restatement_closed_forms():
    # LOD: J = s I -> log2 s; rotation-invariant; anisotropic -> log2 sigma_max; zero -> -inf without NaN
    s = torch.tensor([4.0], dtype=torch.float64)
    z = torch.zeros(1, dtype=torch.float64)
    assert float(R.lod_from_jacobian(s, z, z, s)) == pytest.approx(2.0)
    c, si = math.cos(0.7), math.sin(0.7)
    J = [torch.tensor([v], dtype=torch.float64) for v in (3 * c, -3 * si, 3 * si, 3 * c)]
    assert float(R.lod_from_jacobian(*J)) == pytest.approx(math.log2(3))
    assert float(R.lod_from_jacobian(torch.tensor([8.0], dtype=torch.float64), z, z, torch.tensor([0.5], dtype=torch.float64))) == pytest.approx(3.0)
    assert float(R.lod_from_jacobian(z, z, z, z)) == -math.inf
    # cube faces: centre of texel (i, j) of face f, as the reference's cube_to_dir points at it, returns that texel
    S = 4
    tex = torch.arange(6 * S * S, dtype=torch.float64).reshape(1, 6, S, S, 1)
    ii = (torch.arange(S, dtype=torch.float64) * 2 + 1) / S - 1
    gy, gx = torch.meshgrid(ii, ii, indexing="ij")
    for f in range(6):
        d = R.cube_to_dir(torch.full_like(gx, f, dtype=torch.long), gx, gy)
        d = d / d.norm(dim=-1, keepdim=True)
        out = R.texture(tex, d[None], filter_mode="linear", boundary_mode="cube")
        assert torch.allclose(out[0, ..., 0], tex[0, f, ..., 0]), f
        assert torch.allclose(R.texture(tex, 3.7 * d[None], filter_mode="linear", boundary_mode="cube"), out)
    # constant texture -> constant result everywhere, corners included
    g = torch.Generator().manual_seed(0)
    d = torch.randn(1, 64, 64, 3, generator=g, dtype=torch.float64)
    one = torch.full((1, 6, S, S, 2), 0.25, dtype=torch.float64)
    assert torch.allclose(R.texture(one, d, filter_mode="linear", boundary_mode="cube"), torch.full((1, 64, 64, 2), 0.25, dtype=torch.float64))
    corner = torch.tensor([[[[1.0, 1.0, 1.0]]]], dtype=torch.float64)
    assert torch.allclose(R.texture(one, corner, filter_mode="linear", boundary_mode="cube"), torch.full((1, 1, 1, 2), 0.25, dtype=torch.float64))
    # 2-D: a bias of k at texel centres of level k returns that level's texel; k + f blends
    tex2 = torch.rand(1, 8, 8, 3, generator=g, dtype=torch.float64)
    chain = R.mip_chain(tex2)
    uv = ((torch.stack(torch.meshgrid(torch.arange(4), torch.arange(4), indexing="ij")[::-1], -1).double() + 0.5) / 4)[None]  # level 1 centres
    for k, want in ((1.0, chain[1]), (1.25, 0.75 * chain[1] + 0.25 * R.texture(chain[2], uv, filter_mode="linear", boundary_mode="clamp"))):
        got = R.texture(tex2, uv, mip_level_bias=torch.full((1, 4, 4), k, dtype=torch.float64), boundary_mode="clamp")
        assert torch.allclose(got, want), k


# ------------------------------------------------------------------------------------------------ premises of test_texture_backward_gpu.py
def _all_grads(dtype, f, mode, boundary, uv=None):
    to = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(True)
    tex, u, b = to(f["tex"]), to(f["uv"] if uv is None else uv), to(f["bias"])
    mip = None if f["mip"] is None else [to(m) for m in f["mip"]]
    out = R.texture(tex, u, None, b, mip=mip, filter_mode=mode, boundary_mode=boundary)
    out.backward(f["g"].to(dtype))
    return [out.detach()] + [t.grad if t.grad is not None else torch.zeros_like(t) for t in [tex, u] + (mip or []) + ([b] if b is not None else [])]


@pytest.mark.parametrize("mode", ["nearest", "linear", "linear-mipmap-nearest", "linear-mipmap-linear"])
def test_exact_fields_are_exact_in_fp32(mode):
    """The generator's fields (R.exact_field) give bit-identical outputs and gradients from the restatement in float32 and float64: no
    fp32 operation rounds, so the GPU tests may compare with torch.equal whatever order the kernel's float atomics add in."""
    shapes = [(3, 31, 31), (1, 17, 9), (3, 23, 3)]
    for i, pattern in enumerate(R.PATTERNS):
        B, H, W = shapes[i % 3]
        for size in ((32, 16), (1, 16), (1, 1)):
            for k in (0, 1, 2):
                f = R.exact_field(pattern, B, H, W, size, (1, 3, 5, 8)[i % 4], mode, seed=10 * i + k, k=k, tex_batch=B if i % 2 else 1)
                for boundary in ("wrap", "clamp", "zero"):
                    a, b = _all_grads(torch.float32, f, mode, boundary), _all_grads(torch.float64, f, mode, boundary)
                    for j, (x, y) in enumerate(zip(a, b)):
                        assert torch.equal(x.double(), y), (pattern, size, k, boundary, j, float((x.double() - y).abs().max()))


def _drop_one_families():
    g = R._gen(7)
    f = R.exact_field("mag33", 2, 16, 16, (16, 16), 3, "linear-mipmap-linear", seed=1, k=1)
    yield "exact mag33, custom stack", f["tex"], f["uv"], f["g"], None, f["bias"], f["mip"], dict(filter_mode="linear-mipmap-linear", boundary_mode="wrap")
    f = R.exact_field("run3", 1, 17, 5, (16, 16), 4, "linear", seed=2)
    yield "exact run3, narrow", f["tex"], f["uv"], f["g"], None, None, None, dict(filter_mode="linear", boundary_mode="zero")
    tex = torch.rand(1, 32, 16, 4, generator=g, dtype=torch.float64)
    uv = torch.rand(2, 12, 20, 2, generator=g, dtype=torch.float64) * 1.4 - 0.2
    da = torch.randn(2, 12, 20, 4, generator=g, dtype=torch.float64) * 0.03
    bias = torch.rand(2, 12, 20, generator=g, dtype=torch.float64) * 2 - 0.5
    gg = R.small_ints((2, 12, 20, 4), 3)
    yield "random trilinear, internal stack", tex, uv, gg, da, bias, None, dict(filter_mode="linear-mipmap-linear", boundary_mode="clamp")
    d = torch.randn(1, 16, 16, 3, generator=g, dtype=torch.float64)
    d[0, 0, :8] = torch.tensor([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=torch.float64)
    yield "cube corners", torch.rand(1, 6, 8, 8, 3, generator=g, dtype=torch.float64), d, R.small_ints((1, 16, 16, 3), 4), None, None, None, \
        dict(filter_mode="linear", boundary_mode="cube")
    yy, xx = torch.meshgrid(torch.arange(64.0, dtype=torch.float64), torch.arange(64.0, dtype=torch.float64), indexing="ij")
    uv = torch.stack([(xx + 0.5) / 64 + 0.03 * torch.sin(yy / 23), (yy + 0.5) / 64 + 0.03 * torch.cos(xx / 31)], -1)[None]
    yield "smooth field", torch.rand(1, 24, 32, 4, generator=g, dtype=torch.float64), uv, R.small_ints((1, 64, 64, 4), 5), None, None, None, \
        dict(filter_mode="linear", boundary_mode="wrap")


def test_g_tex_bound_catches_one_dropped_lookup():
    """On each pattern family of the GPU tests, the per-texel bound R.g_tex_bounds is tight enough that a g_tex missing any one
    lookup's contribution breaks it at some texel (checked for every 7th lookup)."""
    for name, tex, uv, g, da, bias, mip, kw in _drop_one_families():
        levels = [tex] + list(mip or [])
        leaves = lambda: [t.clone().requires_grad_(True) for t in levels]

        def g_tex(gg):
            ls = leaves()
            out = R.texture(ls[0], uv, da, bias, mip=ls[1:] if mip else None, **kw)
            return torch.autograd.grad(out, ls, gg, allow_unused=True)

        full = g_tex(g)
        bounds = R.g_tex_bounds(tex, uv, g, da, bias, mip, **kw)
        n = g[..., 0].numel()
        checked = 0
        for i in range(0, n, 7):
            gi = g.reshape(n, -1)
            if float(gi[i].abs().sum()) == 0 or (kw["boundary_mode"] == "cube" and float(uv.reshape(n, 3)[i].abs().sum()) == 0):
                continue
            dropped = gi.clone()
            dropped[i] = 0
            part = g_tex(dropped.reshape(g.shape))
            broke = any(bool(((a - b).abs() > bd).any()) for a, b, bd in zip(full, part, bounds) if a is not None)
            lost = max(float((a - b).abs().max()) for a, b in zip(full, part) if a is not None)
            if lost == 0:  # (a lookup whose taps all fall outside a zero-boundary texture contributes nothing)
                continue
            assert broke, (name, i, lost)
            checked += 1
        assert checked > 10, name
