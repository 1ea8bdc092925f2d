"""The texture backward (csrc/texture.hip: tex_bwd_kernel, tex_mip_fwd_kernel, tex_mip_bwd_kernel) on adversarial lookups, through
ops.texture and the nvdiffrast shim.

Stages of the backward each case below forces:
  - the wave layout: an 8 x 8 block of lookups per wave when W >= 8, full and partial tiles (H, W in 8, 9, 15, 16, 17, 31; B 1 and 3),
    and 64 consecutive lookups when W < 8 (W = 1..7, uv [B, N, 2] with N not a multiple of 64, uv [B, 2], a 5-D uv), where one wave
    spans rows and images;
  - ts_merge (tile_scatter.h), per (level slot, tap slot): every merge distance (1, 8, 2, 16, 4, 32) through magnification (kx, ky)
    for all of 0..3 x 0..3 -- (3, 3) puts a whole wave on one quad; keys equal at distance 2 but not 1; runs of 3 off the power-of-two
    alignment; all keys distinct; keyless lanes (key -1) between equal keys, from zero-boundary taps outside the texture, zero cube
    directions and a level weight of 0;
  - the key numbering keybase[level] + row: neighbouring lanes on different levels that read the same row number, and images of a
    per-image texture (tex_batch == B) that read the same rows, in the W < 8 layout, must not merge; tex_batch == 1 must;
  - collapsed taps: 1 x N, N x 1 and 1 x 1 textures and 1 x 1 top levels, where several tap slots of a lane hit one texel;
  - the filters nearest, linear, linear-mipmap-nearest and linear-mipmap-linear under wrap, clamp and zero; cube maps under linear
    and trilinear, with waves across faces, edge walks and corner thirds;
  - the 16-byte row path and the scalar path (C % 4, and C % 4 == 0 with a level that is contiguous but not 16-byte aligned), C from
    1 to 64;
  - the mip chain's forward and backward on one-axis steps, odd stops, max_mip_level and cube chains;
  - far-out uv (|u| up to 1e12) and Jacobians whose lambda_max overflows or underflows fp32 (|J| up to 1e30, down to 1e-30).

References: the float64 restatement tests/texture_ref.py under autograd.  Where every fp32 operation is exact (power-of-two sizes,
uv = (i + 0.5 + a/8) / size, dyadic texels, small-integer g_out, bias k + {0, 0.25, 0.75}, custom stacks) the comparison is torch.equal
for the output and every gradient, so the order of the float atomics cannot matter.  Everywhere else g_tex is held to the per-texel
bound R.g_tex_bounds (float64 magnitudes times the term count and coordinate scale, times 2^-24), and the per-lookup outputs and
gradients to bounds of the same form; tests/test_texture_cpu.py shows that dropping one lookup's contribution breaks the g_tex bound.
"""
import importlib
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = R.EPS
MODES = ("nearest", "linear", "linear-mipmap-nearest", "linear-mipmap-linear")
BOUNDARIES = ("wrap", "clamp", "zero")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("3danimals_amd.ops")


@pytest.fixture(scope="module")
def dr():
    sys.path.insert(0, os.path.join(ROOT, "3danimals_amd", "shims"))
    return importlib.import_module("nvdiffrast.torch")


def _is_mip(mode):
    return mode in ("linear-mipmap-nearest", "linear-mipmap-linear")


def run(fn, tex, uv, g, uv_da=None, bias=None, mip=None, dtype=torch.float32, device="cpu", **kw):
    """(out, g_tex, [g of each mip level], g_uv, g_uv_da, g_bias) of fn(tex, uv, uv_da, bias, mip=..., **kw) . g, all float64 on the CPU
    (zeros for an input without a gradient)."""
    to = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
    t, u, a, b = to(tex), to(uv), to(uv_da), to(bias)
    ms = None if mip is None else [to(m) for m in mip]
    out = fn(t, u, a, b, mip=ms, **kw)
    out.backward(g.to(device=device, dtype=dtype))
    c = lambda x, ref: torch.zeros(ref.shape, dtype=torch.float64) if x is None or x.grad is None else x.grad.detach().double().cpu()
    return (out.detach().double().cpu(), c(t, tex), [c(m, mm) for m, mm in zip(ms or [], mip or [])], c(u, uv),
            None if a is None else c(a, uv_da), None if b is None else c(b, bias))


def gpu(ops, dev, *args, **kw):
    return run(lambda t, u, a, b, mip=None, **k: ops.texture(t, u, a, b, mip=mip, **k), *args, device=dev, **kw)


def ref(*args, **kw):
    return run(lambda t, u, a, b, mip=None, **k: R.texture(t, u, a, b, mip=mip, **k), *args, dtype=torch.float64, device="cpu", **kw)


NAMES = ("out", "g_tex", "g_mip", "g_uv", "g_uv_da", "g_bias")


def assert_equal(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        if name == "g_mip":
            for l, (x, y) in enumerate(zip(a, b)):
                assert torch.equal(x, y), (what, f"g_mip[{l + 1}]", float((x - y).abs().max()))
        elif b is not None:
            assert a.shape == b.shape and torch.equal(a, b), (what, name, float((a - b).abs().max()))


def assert_within(got, want, bound, what):
    got, want, bound = got.double().cpu(), want.double().cpu(), bound.double().cpu().expand(want.shape)
    err = (got - want).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} elements beyond the bound; first at flat index {i}: got "
                             f"{float(got.reshape(-1)[i])!r}, want {float(want.reshape(-1)[i])!r}, bound {float(bound.reshape(-1)[i]):.3g}")


def lookup_bound(tex, uv, g, cube, levels=1, A=64.0):
    """Per-lookup bound on out / g_bias (and, times the level-0 size, g_uv): the weights carry ~(A + X) EPS absolute error, a dot
    product over C channels C EPS, the internal chain `levels` roundings."""
    X = R.coord_scale(uv.double(), tex, cube).cpu()
    T = float(tex.double().abs().max())
    C = tex.shape[-1]
    gs = g.double().abs().sum(-1).cpu() if g is not None else torch.ones_like(X)
    return 16 * EPS * (A + X + C + levels) * T * gs


def check_bounded(got, want, tex, uv, g, kw, uv_da=None, bias=None, mip=None, level=None, g_bounds=None):
    """out, g_tex (+ custom levels), g_uv, g_bias, g_uv_da within their bounds.  ``level``: the reference's level per lookup (for the
    g_bias / g_uv_da comparison, which is discontinuous where the level crosses an integer: lookups within 1e-5 of one are left out)."""
    cube = kw.get("boundary_mode") == "cube"
    nlev = 1 + (len(mip) if mip is not None else len(R.mip_chain(tex)) - 1)
    lb = lookup_bound(tex, uv, None, cube, nlev)[..., None]
    assert_within(got[0], want[0], lb, "out")
    gb = g_bounds if g_bounds is not None else R.g_tex_bounds(tex, uv, g, uv_da, bias, mip, **kw)
    assert_within(got[1], want[1], gb[0], "g_tex")
    for l, (a, b) in enumerate(zip(got[2], want[2])):
        assert_within(a, b, gb[l + 1], f"g_mip[{l + 1}]")
    lg = lookup_bound(tex, uv, g, cube, nlev)
    size = max(tex.shape[-2], tex.shape[-3])
    assert_within(got[3], want[3], (lg * size)[..., None], "g_uv")
    if bias is not None or uv_da is not None:
        keep = torch.ones_like(lg, dtype=torch.bool)
        if level is not None:  # (the unclamped level; only crossings inside [0, top] matter)
            lev = level.double().cpu()
            keep = ~(((lev - lev.round()).abs() < 1e-5) & (lev > -1e-5) & (lev < nlev - 1 + 1e-5))
            assert float(keep.double().mean()) > 0.99
        if bias is not None:
            assert_within(got[5] * keep, want[5] * keep, lg, "g_bias")
        if uv_da is not None:
            # |d level / d uv_da| per lookup (its largest component: the others may be ~0 by cancellation) from the restatement
            big = want[4].abs().amax(-1, keepdim=True)
            dl = big / want[5].abs().clamp(min=1e-300)[..., None] if bias is not None else big
            assert_within(got[4] * keep[..., None], want[4] * keep[..., None], lg[..., None] * dl + 2 ** -12 * big, "g_uv_da")


def ref_level_2d(uv_da, bias, size, nlev):
    """The restatement's level per lookup (2-D), float64, before the clamp to [0, nlev - 1]."""
    d = uv_da.double()
    lod = R.lod_from_jacobian(d[..., 0] * size[1], d[..., 1] * size[1], d[..., 2] * size[0], d[..., 3] * size[0])
    return lod + (0 if bias is None else bias.double())


def case(ops, dev, f, mode, boundary, what, uv=None):
    kw = dict(filter_mode=mode, boundary_mode=boundary)
    args = (f["tex"], f["uv"] if uv is None else uv, f["g"])
    opt = dict(bias=f["bias"], mip=f["mip"], **kw)
    assert_equal(gpu(ops, dev, *args, **opt), ref(*args, **opt), what)


# ------------------------------------------------------------------------------------------------ exact: merge patterns
SHAPES = [(1, 8, 8), (3, 9, 9), (1, 15, 15), (3, 16, 16), (1, 17, 17), (3, 31, 31), (1, 8, 31), (3, 17, 9), (1, 31, 16), (3, 15, 8)]


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_exact_merge_patterns(pattern, mode, boundary, dev, ops):
    i = R.PATTERNS.index(pattern)
    B, H, W = SHAPES[(i + MODES.index(mode)) % len(SHAPES)]
    C = (1, 2, 3, 4, 5, 8)[i % 6]
    f = R.exact_field(pattern, B, H, W, (16, 32) if i % 2 else (32, 16), C, mode, seed=100 + i, k=i % 3, tex_batch=B if i % 4 == 1 else 1)
    case(ops, dev, f, mode, boundary, (pattern, mode, boundary, B, H, W, C))


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_exact_frame_shapes_w_ge_8(B, H, W, dev, ops):
    for mode in ("linear", "linear-mipmap-linear"):
        f = R.exact_field("mag11", B, H, W, (16, 16), 3, mode, seed=200 + H * W, k=1)
        case(ops, dev, f, mode, "wrap", (B, H, W, mode))


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8, 16, 33, 64])
def test_exact_channels(C, dev, ops):
    for pattern, mode in (("mag33", "linear-mipmap-linear"), ("alt", "linear"), ("run3", "nearest")):
        f = R.exact_field(pattern, 3, 17, 16, (16, 16), C, mode, seed=300 + C, k=1, tex_batch=3 if C % 2 else 1)
        case(ops, dev, f, mode, "clamp", (C, pattern, mode))


@pytest.mark.parametrize("W", [1, 2, 3, 4, 5, 6, 7])
def test_exact_narrow_frames(W, dev, ops):
    """W < 8: 64 consecutive lookups per wave, across rows and images."""
    for mode in MODES:
        for bt in (1, 3):
            f = R.exact_field("mag21", 3, 23, W, (16, 16), 4 if W % 2 else 3, mode, seed=400 + W, k=1, tex_batch=bt)
            case(ops, dev, f, mode, ("wrap", "clamp", "zero")[W % 3], (W, mode, bt))


@pytest.mark.parametrize("tex_batch", [1, 3])
@pytest.mark.parametrize("lead", [(37,), (100,), (), (3, 5, 7)])
def test_exact_image_split_in_the_narrow_layout(lead, tex_batch, dev, ops):
    """uv [B, N, 2], [B, 2] and 5-D: the wrapper sets W = 1.  Every image samples the same uv: with a per-image texture the images'
    lanes (one wave holds several) must not merge; with a shared texture they add into the same texels."""
    B, C = 3, 5
    n = 1
    for s in lead:
        n *= s
    for mode in MODES:
        f = R.exact_field("mag33", 1, 1, n, (8, 16), C, mode, seed=500 + n, k=1, tex_batch=tex_batch)
        uv = f["uv"].reshape(1, *lead, 2).expand(B, *lead, 2).contiguous()
        f["g"] = R.small_ints((B,) + tuple(lead) + (C,), 501 + n)
        if f["bias"] is not None:
            f["bias"] = f["bias"].reshape(1, *lead).expand(B, *lead).contiguous()
        for boundary in ("wrap", "zero"):
            case(ops, dev, f, mode, boundary, (lead, tex_batch, mode, boundary), uv=uv)


@pytest.mark.parametrize("mode", MODES)
def test_exact_holes_from_zero_boundary(mode, dev, ops):
    """Equal keys with every other lane keyless: odd-x lanes sample outside a zero-boundary texture (all four taps key -1)."""
    f = R.exact_field("mag33", 2, 16, 16, (16, 16), 4, mode, seed=600, k=1)
    px, _ = R.frame_xy(2, 16, 16)
    uv = torch.where((px % 2 == 1)[..., None], torch.tensor([-1.5, 2.75], dtype=torch.float64), f["uv"])
    case(ops, dev, f, mode, "zero", mode, uv=uv)


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_exact_holes_from_zero_level_weight(boundary, dev, ops):
    """linear-mipmap-linear with an integer bias on every other lane: its second level slot has weight 0 (key -1) between lanes whose
    slot is live."""
    f = R.exact_field("mag33", 1, 16, 16, (16, 16), 3, "linear-mipmap-linear", seed=610, k=1)
    px, _ = R.frame_xy(1, 16, 16)
    f["bias"] = torch.where(px % 2 == 1, torch.full_like(f["bias"], 1.0), torch.full_like(f["bias"], 1.25))
    case(ops, dev, f, "linear-mipmap-linear", boundary, boundary)


@pytest.mark.parametrize("mode", ["linear-mipmap-nearest", "linear-mipmap-linear"])
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_exact_level_split(mode, boundary, dev, ops):
    """Neighbouring lanes on different levels read the same row numbers (uv near the origin: row 0 of both levels); keybase keeps the
    levels' keys apart."""
    B, H, W, C = 1, 16, 16, 3
    f = R.exact_field("mag33", B, H, W, (16, 16), C, mode, seed=620, k=0)
    px, py = R.frame_xy(B, H, W)
    a = torch.randint(0, 8, (2, B, H, W), generator=R._gen(621))
    f["uv"] = R.exact_uv(torch.zeros_like(px), torch.zeros_like(py), a[0], a[1], 16, 16)
    lane = (px & 7) + 8 * (py & 7)
    off = 0.25 if mode == "linear-mipmap-linear" else 0.0
    f["bias"] = ((lane ^ (lane >> 1) ^ (lane >> 3)) & 1).double() + off  # (neighbours at distance 1 and 8 differ)
    case(ops, dev, f, mode, boundary, (mode, boundary))


@pytest.mark.parametrize("size", [(1, 16), (16, 1), (1, 1), (2, 1), (1, 2)])
def test_exact_collapsed_taps(size, dev, ops):
    """1 x N, N x 1 and 1 x 1 textures (and their 1 x 1 top levels): several tap slots of one lane hit one texel."""
    for mode in MODES:
        f = R.exact_field("mag22", 3, 9, 10, size, 3, mode, seed=700 + size[0] * 10 + size[1], k=2, tex_batch=3)
        for boundary in BOUNDARIES:
            case(ops, dev, f, mode, boundary, (size, mode, boundary))


# ------------------------------------------------------------------------------------------------ exact: cube maps
def exact_cube(B, H, W, S, C, seed, mode, k=0, tex_batch=1):
    """Directions whose major component is +-1 and whose face coordinate is a texel centre + a/8 of level k; one coordinate of a lookup
    may take a tap off the face (an edge walk), never both (no corner tap), on level k and k + 1."""
    levels = len(R.mip_sizes(S, S)) if _is_mip(mode) else 1
    g = R._gen(seed)
    s = S >> k
    N = B * H * W
    face = torch.randint(0, 6, (N,), generator=g)
    lo, hi = (2, s - 2) if _is_mip(mode) else (0, s - 1)  # (mipmap: the coordinate that stays on the face stays off level k + 1's edges)
    ix = torch.randint(lo, hi, (N,), generator=g)
    iy = torch.randint(lo, hi, (N,), generator=g)
    a = torch.randint(0, 8, (2, N), generator=g)
    edge = torch.randint(0, 4, (N,), generator=g)  # 0: inside; 1: x below; 2: x above; 3: y above
    ix = torch.where(edge == 1, -1, torch.where(edge == 2, s - 1, ix))
    a[0] = torch.where(edge == 1, 5 + a[0] % 3, torch.where(edge == 2, a[0] % 4, a[0]))
    iy = torch.where(edge == 3, s - 1, iy)
    a[1] = torch.where(edge == 3, a[1] % 4, a[1])
    st = lambda i, aa: 2 * (i.double() + 0.5 + aa.double() / 8) / s - 1
    d = R.cube_to_dir(face, st(ix, a[0]), st(iy, a[1])).reshape(B, H, W, 3)
    tex = R.dyadic((tex_batch, 6, S, S, C), seed + 1)
    mip = [R.dyadic((tex_batch, 6, S >> l, S >> l, C), seed + 1 + l) for l in range(1, levels)] if _is_mip(mode) else None
    bias = None
    if _is_mip(mode):
        px, py = R.frame_xy(B, H, W)
        bias = k + torch.tensor(R.FRACTIONS, dtype=torch.float64)[(px + 2 * py) % 3]
    return dict(tex=tex, mip=mip, uv=d, bias=bias, g=R.small_ints((B, H, W, C), seed + 2))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tex_batch", [1, 2])
def test_exact_cube_without_corners(mode, tex_batch, dev, ops):
    f = exact_cube(2, 16, 12, 16, 3 + tex_batch, 800 + tex_batch, mode, k=1, tex_batch=tex_batch)
    case(ops, dev, f, mode, "cube", (mode, tex_batch))


# ------------------------------------------------------------------------------------------------ bounded: corners, uv_da, random fields
@pytest.mark.parametrize("mode", ["linear", "linear-mipmap-linear"])
@pytest.mark.parametrize("tex_batch", [1, 2])
def test_cube_corners_and_zero_directions_bounded(mode, tex_batch, dev, ops):
    """Random directions (waves across faces), the eight corner directions (corner thirds) and zero directions on every other lane
    (keyless holes)."""
    B, H, W, S, C = 2, 16, 16, 8, 3
    d = torch.randn(B, H, W, 3, generator=R._gen(900), dtype=torch.float64)
    corners = torch.tensor([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=torch.float64)
    d[:, :2, :8] = corners.reshape(1, 8, 3) * (1 + torch.rand(B, 2, 8, 1, generator=R._gen(901), dtype=torch.float64) * 1e-3)
    px, _ = R.frame_xy(B, H, W)
    d[:, 8:] = torch.where((px[:, 8:] % 2 == 1)[..., None], torch.zeros(3, dtype=torch.float64), d[:, 8:])
    tex = R.dyadic((tex_batch, 6, S, S, C), 902)
    g = R.small_ints((B, H, W, C), 903)
    bias = torch.rand(B, H, W, generator=R._gen(904), dtype=torch.float64) * 3 - 0.25 if mode != "linear" else None
    kw = dict(filter_mode=mode, boundary_mode="cube")
    d32 = d.float().double()
    b32 = None if bias is None else bias.float().double()
    got = gpu(ops, dev, tex, d32, g, bias=b32, **kw)
    want = ref(tex, d32, g, bias=b32, **kw)
    check_bounded(got, want, tex, d32, g, kw, bias=b32, level=b32)
    z = (d32.abs().sum(-1) == 0)
    assert float(got[0][z].abs().max()) == 0 and float(got[3][z].abs().max()) == 0


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("size", [(64, 16), (16, 64), (24, 40), (1, 32), (32, 1)])
def test_trilinear_internal_stack_on_non_square_textures_bounded(size, boundary, dev, ops):
    B, H, W, C = 2, 12, 20, 4
    tex = R.dyadic((1,) + size + (C,), 1000)
    uv = (torch.rand(B, H, W, 2, generator=R._gen(1001), dtype=torch.float64) * 1.4 - 0.2).float().double()
    da = (torch.randn(B, H, W, 4, generator=R._gen(1002), dtype=torch.float64) * 0.03).float().double()
    bias = (torch.rand(B, H, W, generator=R._gen(1003), dtype=torch.float64) * 2 - 0.5).float().double()
    g = R.small_ints((B, H, W, C), 1004)
    kw = dict(filter_mode="linear-mipmap-linear", boundary_mode=boundary)
    got = gpu(ops, dev, tex, uv, g, uv_da=da, bias=bias, **kw)
    want = ref(tex, uv, g, uv_da=da, bias=bias, **kw)
    nlev = len(R.mip_sizes(*size))
    check_bounded(got, want, tex, uv, g, kw, uv_da=da, bias=bias, level=ref_level_2d(da, bias, size, nlev))


@pytest.mark.parametrize("C", [4, 8])
def test_scalar_path_for_an_unaligned_level(C, dev, ops):
    """C % 4 == 0 with a level that is contiguous but not 16-byte aligned takes the scalar path: its forward equals the 16-byte path
    bit for bit, its backward stays within the bound."""
    tex = R.dyadic((1, 16, 16, C), 1100)
    mip = [R.dyadic((1, 16 >> l, 16 >> l, C), 1100 + l) for l in range(1, 5)]
    uv = (torch.rand(2, 16, 16, 2, generator=R._gen(1101), dtype=torch.float64) * 1.2 - 0.1).float().double()
    bias = (torch.rand(2, 16, 16, generator=R._gen(1102), dtype=torch.float64) * 4).float().double()
    g = R.small_ints((2, 16, 16, C), 1103)

    def unaligned(t):
        s = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)[1:].view(t.shape)
        s.copy_(t)
        assert s.is_contiguous() and s.data_ptr() % 16 == 4
        return s

    kw = dict(filter_mode="linear-mipmap-linear", boundary_mode="wrap")
    ms = [m.float().to(dev) for m in mip]
    aligned = ops.texture(tex.float().to(dev), uv.float().to(dev), mip_level_bias=bias.float().to(dev), mip=ms, **kw)
    for which in (0, 2):
        t = unaligned(tex.float().to(dev)) if which == 0 else tex.float().to(dev)
        mm = [unaligned(m) if l + 1 == which else m for l, m in enumerate(ms)]
        got = ops.texture(t, uv.float().to(dev), mip_level_bias=bias.float().to(dev), mip=mm, **kw)
        assert torch.equal(got, aligned), which
    # backward: autograd through a leaf whose storage is offset by one float
    leaf = unaligned(tex.float().to(dev)).requires_grad_(True)
    ml = [m.clone().requires_grad_(True) for m in ms]
    u = uv.float().to(dev).requires_grad_(True)
    b = bias.float().to(dev).requires_grad_(True)
    out = ops.texture(leaf, u, mip_level_bias=b, mip=ml, **kw)
    out.backward(g.float().to(dev))
    got = (out.detach().double().cpu(), leaf.grad.double().cpu(), [m.grad.double().cpu() for m in ml], u.grad.double().cpu(), None,
           b.grad.double().cpu())
    want = ref(tex, uv, g, bias=bias, mip=mip, **kw)
    check_bounded(got, want, tex, uv, g, kw, bias=bias, mip=mip, level=bias)


# ------------------------------------------------------------------------------------------------ at scale (float64 reference on the GPU)
def test_at_scale_trilinear_with_uv_da_against_float64(dev, ops):
    """4 x 128^2 lookups into a 512^2 texture through the internal stack, with uv_da and a bias: every gradient against the float64
    restatement, not only run-to-run reproducibility."""
    B, H, W, T, C = 4, 128, 128, 512, 4
    g0 = torch.Generator(device=dev).manual_seed(1200)
    tex = torch.rand(1, T, T, C, device=dev, generator=g0, dtype=torch.float64).float().double()
    uv = (torch.rand(B, H, W, 2, device=dev, generator=g0, dtype=torch.float64) * 1.5 - 0.25).float().double()
    da = (torch.randn(B, H, W, 4, device=dev, generator=g0, dtype=torch.float64) * 0.01).float().double()
    bias = (torch.rand(B, H, W, device=dev, generator=g0, dtype=torch.float64) * 2 - 1).float().double()
    g = torch.randint(-3, 4, (B, H, W, C), device=dev, generator=g0).double()
    kw = dict(filter_mode="linear-mipmap-linear", boundary_mode="wrap")
    got = gpu(ops, dev, tex, uv, g, uv_da=da, bias=bias, **kw)
    want = run(lambda t, u, a, b, mip=None, **k: R.texture(t, u, a, b, mip=mip, **k), tex, uv, g, uv_da=da, bias=bias,
               dtype=torch.float64, device=dev, **kw)
    bounds = [b.cpu() for b in R.g_tex_bounds(tex, uv, g, da, bias, None, **kw)]
    check_bounded(got, want, tex.cpu(), uv.cpu(), g.cpu(), kw, uv_da=da.cpu(), bias=bias.cpu(),
                  level=ref_level_2d(da, bias, (T, T), 10).cpu(), g_bounds=bounds)


def test_at_scale_smooth_field_merges(dev, ops):
    """16 x 256^2 lookups of a smooth uv field at ~6 lookups per texel (a 128 x 96 texture): merges at scale, bounded."""
    B, H, W, C = 16, 256, 256, 4
    g0 = torch.Generator(device=dev).manual_seed(1300)
    tex = torch.rand(1, 96, 128, C, device=dev, generator=g0, dtype=torch.float64).float().double()
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    ph = torch.arange(B, device=dev, dtype=torch.float64).view(B, 1, 1)
    u = (xx + 0.5) / W + 0.03 * torch.sin(yy / 23 + ph) + 0.1 * ph / B
    v = (yy + 0.5) / H + 0.03 * torch.cos(xx / 31 - ph)
    uv = torch.stack([u, v], -1).float().double()
    g = torch.randint(-3, 4, (B, H, W, C), device=dev, generator=g0).double()
    kw = dict(filter_mode="linear", boundary_mode="wrap")
    got = gpu(ops, dev, tex, uv, g, **kw)
    want = run(lambda t, u_, a, b, mip=None, **k: R.texture(t, u_, a, b, mip=mip, **k), tex, uv, g, dtype=torch.float64, device=dev, **kw)
    bounds = [b.cpu() for b in R.g_tex_bounds(tex, uv, g, **kw)]
    check_bounded(got, want, tex.cpu(), uv.cpu(), g.cpu(), kw, g_bounds=bounds)


# ------------------------------------------------------------------------------------------------ the mip chain
@pytest.mark.parametrize("size", [(64, 16), (16, 64), (1, 32), (32, 1), (24, 40), (6, 1), (1, 1)])
@pytest.mark.parametrize("C", [3, 4])
def test_mip_chain_levels_and_backward_exact(size, C, dev, ops, dr):
    tex = R.dyadic((2,) + size + (C,), 1400 + C)
    chain = R.mip_chain(tex)
    got = dr.texture_construct_mip(tex.float().to(dev))
    assert len(got.levels) == len(chain) - 1
    for l, (a, b) in enumerate(zip(got.levels, chain[1:])):
        assert torch.equal(a.double().cpu(), b), (size, l + 1)
    _exact_mip_backward(ops, dev, tex, False)


def _exact_mip_backward(ops, dev, tex, cube, max_mip_level=None):
    H, W = tex.shape[-3], tex.shape[-2]
    sizes = ops.texture_mip_sizes(H, W, max_mip_level)
    if len(sizes) == 1:
        return
    gl = [torch.randint(-8, 9, tuple(tex.shape[:-3]) + (h, w, tex.shape[-1]), generator=R._gen(1450 + l)).double() / 4
          for l, (h, w) in enumerate(sizes[1:])]
    t = tex.float().to(dev).requires_grad_(True)
    levels = ops._TextureMip.apply(t, sizes, cube)
    levels = levels if isinstance(levels, tuple) else (levels,)
    for a, b in zip(levels, R.mip_chain(tex, max_mip_level)[1:]):
        assert torch.equal(a.detach().double().cpu(), b)
    torch.autograd.backward(levels, [x.float().to(dev) for x in gl])
    leaf = tex.clone().requires_grad_(True)
    want = torch.autograd.grad(R.mip_chain(leaf, max_mip_level)[1:], leaf, gl)[0]
    assert torch.equal(t.grad.double().cpu(), want), (tuple(tex.shape), max_mip_level)


def test_mip_chain_ten_levels_and_cube_batch_exact(dev, ops, dr):
    _exact_mip_backward(ops, dev, R.dyadic((1, 512, 512, 1), 1500), False)  # 10 levels
    _exact_mip_backward(ops, dev, R.dyadic((1, 512, 2, 3), 1501), False)
    cube = R.dyadic((3, 6, 16, 16, 4), 1502)
    got = dr.texture_construct_mip(cube.float().to(dev), cube_mode=True)
    for a, b in zip(got.levels, R.mip_chain(cube)[1:]):
        assert torch.equal(a.double().cpu(), b)
    _exact_mip_backward(ops, dev, cube, True)


@pytest.mark.parametrize("max_mip_level", [0, 1, 2])
@pytest.mark.parametrize("C", [3, 4])
def test_max_mip_level(max_mip_level, C, dev, ops):
    tex = R.dyadic((1, 32, 16, C), 1600 + C)
    _exact_mip_backward(ops, dev, tex, False, max_mip_level)
    # a bias past the top samples level max_mip_level of the internal chain
    f = R.exact_field("mag11", 1, 9, 9, (32, 16), C, "linear-mipmap-linear", seed=1601)
    bias = torch.full((1, 9, 9), 7.0, dtype=torch.float64)
    kw = dict(filter_mode="linear-mipmap-linear", boundary_mode="clamp", max_mip_level=max_mip_level)
    got = gpu(ops, dev, tex, f["uv"], f["g"], bias=bias, **kw)
    want = ref(tex, f["uv"], f["g"], bias=bias, **kw)
    assert_equal(got, want, ("max_mip_level", max_mip_level, C))
    top = R.mip_chain(tex, max_mip_level)[-1]
    assert torch.equal(got[0], R.texture(top, f["uv"], filter_mode="linear", boundary_mode="clamp"))


# ------------------------------------------------------------------------------------------------ known answers: far-out uv
FAR = (1e6, 1e9, 1e12)


def _far_uv(n_in, seed, far, both):
    """[1, N, 2]: u far out (+-far, and +-far plus sixteenths where fp32 holds them); v a dyadic texel coordinate, or far too."""
    us = []
    for f in far:
        for s in (1, -1):
            us += [s * f, s * f + 0.0625, s * f + 0.4375, s * f - 0.25]
    u = torch.tensor(us, dtype=torch.float32).double()
    z = torch.zeros(u.numel(), dtype=torch.long)
    v = R.exact_uv(z, torch.randint(0, n_in, (u.numel(),), generator=R._gen(seed)), z,
                   torch.randint(0, 8, (u.numel(),), generator=R._gen(seed + 1)), 1, n_in)[..., 1]
    if both:
        v = u.flip(0)
    return torch.stack([u, v], -1)[None]


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_far_out_uv(boundary, both, dev, ops):
    """|u| in {1e6, 1e9, 1e12} on a 1024-wide texture: clamp reads the edge column (the corner texel when v is far too), zero reads
    nothing, wrap reads u mod 1; the far-out component of g_uv is 0 under clamp and zero, and g_tex is exact."""
    tex = R.dyadic((1, 8, 1024, 3), 1700)
    uv = _far_uv(8, 1701, FAR, both)
    g = R.small_ints(uv.shape[:-1] + (3,), 1702)
    for mode in ("nearest", "linear"):
        kw = dict(filter_mode=mode, boundary_mode=boundary)
        got = gpu(ops, dev, tex, uv, g, **kw)
        want = ref(tex, uv, g, **kw)
        assert_equal(got, want, ("far", boundary, both, mode))
        if boundary != "wrap":
            assert float(got[3][..., 0].abs().max()) == 0.0
        if boundary == "zero":
            assert float(got[0].abs().max()) == 0.0 and float(got[1].abs().max()) == 0.0
        if boundary == "clamp":  # the edge column (u -> 0 or 1), or the corner texel
            edge = uv.clone()
            edge[..., 0] = (uv[..., 0] > 0).double()
            if both:
                edge[..., 1] = (uv[..., 1] > 0).double()
            assert torch.equal(got[0], R.texture(tex, edge, filter_mode=mode, boundary_mode="clamp"))


def test_far_out_uv_mipmapped_and_near_the_threshold(dev, ops):
    """Far-out uv on every level of a trilinear lookup, and |x| just either side of 2^22 (where the reduction starts)."""
    tex = R.dyadic((1, 16, 1024, 3), 1710)
    mip = [R.dyadic((1,) + s + (3,), 1711 + l) for l, s in enumerate(R.mip_sizes(16, 1024)[1:])]
    uv = _far_uv(16, 1712, FAR + (4096.0, 4096.25, 8192.0), False)
    bias = torch.tensor(R.FRACTIONS, dtype=torch.float64).repeat(uv.shape[1] // 3 + 1)[: uv.shape[1]][None] + 1
    g = R.small_ints(uv.shape[:-1] + (3,), 1713)
    for boundary in BOUNDARIES:
        kw = dict(filter_mode="linear-mipmap-linear", boundary_mode=boundary)
        assert_equal(gpu(ops, dev, tex, uv, g, bias=bias, mip=mip, **kw), ref(tex, uv, g, bias=bias, mip=mip, **kw), ("far mip", boundary))


# ------------------------------------------------------------------------------------------------ known answers: huge and tiny Jacobians
JS = (1e9, 1e10, 1e20, 1e30)


def _aniso_da(J, n, size, seed):
    """uv_da [1, 1, n, 4] whose texel Jacobian has largest singular value ~J (anisotropic: lambda's hd^2 overflows first)."""
    g = R._gen(seed)
    a = torch.rand(n, generator=g, dtype=torch.float64) * 6.28
    r = 0.25 + torch.rand(n, generator=g, dtype=torch.float64) * 0.5
    Jm = torch.stack([J * torch.cos(a), -J * r * torch.sin(a), J * torch.sin(a), J * r * torch.cos(a)], -1)
    return (Jm / torch.tensor([size[1], size[1], size[0], size[0]], dtype=torch.float64)).float().double().view(1, 1, n, 4)


@pytest.mark.parametrize("boundary", ["wrap", "clamp"])
@pytest.mark.parametrize("J", JS)
def test_huge_jacobian_samples_the_top_level(J, boundary, dev, ops):
    n, S = 40, 16
    tex = R.dyadic((1, S, S, 3), 1800)
    z = torch.zeros(n, dtype=torch.long)  # (texel centres: on the 1 x 1 top level every weight times a texel stays exact)
    uv = R.exact_uv(torch.arange(n) % S, (torch.arange(n) * 7) % S, z, z, S, S).view(1, 1, n, 2)
    da = _aniso_da(J, n, (S, S), 1801)
    bias = torch.zeros(1, 1, n, dtype=torch.float64)
    g = R.small_ints((1, 1, n, 3), 1802)
    kw = dict(filter_mode="linear-mipmap-linear", boundary_mode=boundary)
    got = gpu(ops, dev, tex, uv, g, uv_da=da, bias=bias, **kw)
    mean = tex.mean((1, 2))
    assert torch.equal(got[0], mean.view(1, 1, 1, 3).expand(1, 1, n, 3)), ("top level (1x1 mean)", J)
    assert float(got[4].abs().max()) == 0.0 and float(got[5].abs().max()) == 0.0, ("no level gradient at the clamp", J)
    want = ref(tex, uv, g, uv_da=da, bias=bias, **kw)
    check_bounded(got, want, tex, uv, g, kw, uv_da=da, bias=bias)


@pytest.mark.parametrize("J", JS)
def test_huge_jacobian_on_a_cube(J, dev, ops):
    n, S = 40, 16
    tex = R.dyadic((1, 6, S, S, 3), 1810)
    d = torch.randn(1, 1, n, 3, generator=R._gen(1811), dtype=torch.float64).float().double()
    da = (torch.randn(1, 1, n, 6, generator=R._gen(1812), dtype=torch.float64) * (J / (2 * S))).float().double()  # (|J| ~ J texels)
    bias = torch.zeros(1, 1, n, dtype=torch.float64)
    g = R.small_ints((1, 1, n, 3), 1813)
    kw = dict(filter_mode="linear-mipmap-linear", boundary_mode="cube")
    got = gpu(ops, dev, tex, d, g, uv_da=da, bias=bias, **kw)
    want = ref(tex, d, g, uv_da=da, bias=bias, **kw)
    top = R.texture(R.mip_chain(tex)[-1], d, filter_mode="linear", boundary_mode="cube")
    assert_within(got[0], top, lookup_bound(tex, d, None, True, 5)[..., None], f"top level, J={J}")
    assert float(got[4].abs().max()) == 0.0 and float(got[5].abs().max()) == 0.0, ("no level gradient at the clamp", J)
    check_bounded(got, want, tex, d, g, kw, uv_da=da, bias=bias)


@pytest.mark.parametrize("J,b", [(1e10, -30.0), (1e20, -63.0), (1e-30, 0.0), (1e-30, 100.6)])
def test_jacobian_beyond_fp32_with_a_bias_back_into_the_chain(J, b, dev, ops):
    """J = 1e10 and bias -30 give a level of about 3.2: the output, g_bias and g_uv_da follow the restatement there (a fix that only
    maps lambda = inf to the top level fails this).  J = 1e-30 gives level 0; with bias 100.6 the level is back at ~1."""
    n, S = 40, 16
    tex = R.dyadic((1, S, S, 3), 1820)
    uv = (torch.rand(1, 1, n, 2, generator=R._gen(1821), dtype=torch.float64)).float().double()
    da = _aniso_da(J, n, (S, S), 1822)
    bias = torch.full((1, 1, n), b, dtype=torch.float64)
    g = R.small_ints((1, 1, n, 3), 1823)
    kw = dict(filter_mode="linear-mipmap-linear", boundary_mode="wrap")
    got = gpu(ops, dev, tex, uv, g, uv_da=da, bias=bias, **kw)
    want = ref(tex, uv, g, uv_da=da, bias=bias, **kw)
    level = ref_level_2d(da, bias, (S, S), 5)
    check_bounded(got, want, tex, uv, g, kw, uv_da=da, bias=bias, level=level)
    level = level.clamp(0, 4)
    if b == 0.0:
        lin = ops.texture(tex.float().to(dev), uv.float().to(dev), filter_mode="linear", boundary_mode="wrap")
        assert float(level.max()) == 0.0 and torch.equal(got[0], lin.double().cpu())
    else:
        assert 0.5 < float(level.min()) and float(level.max()) < 3.9, level
        assert float(want[5].abs().max()) > 0 and float(got[5].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ uv_da alignment
def test_unaligned_uv_da_is_copied_before_the_kernels(dev, ops, monkeypatch):
    """The kernels read a 2-D uv_da row as a float4: a contiguous uv_da at a 4-byte offset must reach them as an aligned copy."""
    seen = []
    real = ops.call

    def checked(name, *args, **kw):
        if name in ("a3d_texture_fwd", "a3d_texture_bwd"):
            p = args[2] if name == "a3d_texture_fwd" else args[3]
            seen.append(name)
            assert p is None or p % 16 == 0, f"{name}: uv_da pointer {p:#x} is not 16-byte aligned"
            if name == "a3d_texture_bwd":
                assert args[9] is None or args[9] % 16 == 0, f"{name}: g_uv_da pointer {args[9]:#x} is not 16-byte aligned"
        return real(name, *args, **kw)

    tex = torch.rand(1, 32, 32, 3, device=dev)
    uv = torch.rand(2, 8, 8, 2, device=dev)
    da = torch.randn(2, 8, 8, 4, device=dev) * 0.05
    g = torch.randn(2, 8, 8, 3, device=dev)
    mis = torch.empty(da.numel() + 1, device=dev)[1:].view(da.shape)
    mis.copy_(da)
    assert mis.is_contiguous() and mis.data_ptr() % 16 == 4
    outs = []
    monkeypatch.setattr(ops, "call", checked)
    for d in (da, mis):
        dd = d.detach().requires_grad_(True)
        t = tex.clone().requires_grad_(True)
        o = ops.texture(t, uv, uv_da=dd, boundary_mode="wrap")
        o.backward(g)
        outs.append((o.detach(), t.grad, dd.grad))
    assert seen.count("a3d_texture_fwd") == 2 and seen.count("a3d_texture_bwd") == 2
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2])
