"""The fused G-buffer kernels (csrc/gbuffer.hip: gb_fwd_kernel, gb_cover_fwd_kernel, gb_bwd_kernel<512,640> / <1024,768>,
gb_prior_sum_kernel) against float64 on covered-pixel lists fabricated to force every stage of the backward's scatter -- both merge
rounds, no merge, the entry overflow, the slot overflow, probe exhaustion, long lists on one slot, image boundaries between lanes, holes
and partial work-groups -- each under both table sizes (tests/gbuffer_ref.py; tests/test_gbuffer_cpu.py asserts what each pattern forces).
Every call goes through the C ABI (_lib.call) with its outputs poisoned with NaN first.

Exact mode: columns 0..11 of the gradient rows and the forward's interpolated columns are torch.equal to float64; the clip columns 12, 13,
15 are held to rast_bwd_reference's bound with exact (gu, gv).  Normal mode: columns 0..2 (face-normal adjoint included) are held to
gbuffer_ref.vpos_bound, a bound counted from gb_pixel_adjoint's operations.
"""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbuffer_ref as G  # noqa: E402
from test_scatter_backward_gpu import _check_rast, _clip_of  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
H, W = 24, 40
EXACT_FWD_COLS = [0, 1, 2, 6, 7, 8, 9, 10, 11]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("3danimals_amd._lib")


def _case(name, table, B, seed=0):
    """'holes<P>' -> the holes pattern with P entries (P = 1 under the 512-slot instance needs B = 1: 1 >= 0.6 * B * F)."""
    P = None
    if name.startswith("holes"):
        name, P = "holes", int(name[5:])
        if P == 1 and table == "small":
            B = 1
    case = G.finish(G.make_list(name, table, B, seed, P), B, H, W, seed)
    G.assert_forced(case)  # the side of P < 0.6 * B * F this case is meant for, and the stage its pattern forces
    return case


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _d(x, dev):
    return None if x is None else x.to(dev)


def run_bwd(L, dev, case, t, clip, want_prior, clear):
    """a3d_gbuffer_bwd -> gradient rows [B*V,16] on the CPU.  clear = 0: the rows arrive poisoned and the entry point must clear them."""
    B, V, F, P = case["B"], case["V"], case["F"], case["P"]
    d = {k: _d(v, dev) for k, v in t.items()}
    tri = torch.from_numpy(case["tri"]).int().to(dev)
    pix = torch.from_numpy(case["pix"]).to(dev)
    rows = torch.zeros(B, V, G.GB_ROW, device=dev) if clear else _nan(dev, B, V, G.GB_ROW)
    E = 0 if t["extra"] is None else t["extra"].shape[-1]
    clip_d = _d(clip, dev)
    L.call("a3d_gbuffer_bwd", L.ptr(d["g_out"]), L.ptr(d["rast"]), L.ptr(tri), L.ptr(pix), P, L.ptr(d["v_pos"]), L.ptr(d["v_nrm"]),
           L.ptr(d["prior"]), t["prior"].shape[0], L.ptr(clip_d), B, V, F, H, W, L.ptr(rows), int(clear), int(want_prior), L.ptr(d["extra"]), E,
           L.ptr(d["g_extra"]), L.ptr(d["g_tex"]), L.stream())
    torch.cuda.synchronize()
    return rows.cpu().reshape(B * V, G.GB_ROW)


def _assert_rows_equal(got, ref, what):
    bad = (got != ref).any(-1).nonzero().reshape(-1)
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {got.shape[0]} vertex rows differ, e.g. row {int(bad[0])}: "
                              f"{got[bad[0]].tolist()} vs {ref[bad[0]].tolist()}")


# (E, prior_batch 1 or B, g_tex, want_prior, want_clip, g_rows_are_clear)
SWITCHES = [(0, "B", True, 1, True, 0), (1, 1, False, 1, True, 1), (2, "B", True, 0, False, 0), (3, 1, True, 1, True, 1),
            (0, 1, False, 0, False, 1)]
LISTS = ["runs", "period8", "checker", "unique", "collide", "fan", "boundary", "holes1", "holes255", "holes256", "holes257"]
EXACT_CASES = [(name, table, (i + j + 2 * k) % len(SWITCHES), 3 if (i + k) % 3 == 2 else 2)
               for i, name in enumerate(LISTS) for j, table in enumerate(["small", "big"]) for k in range(2)]


@pytest.mark.parametrize("name,table,sw,B", EXACT_CASES, ids=[f"{n}-{t}-s{s}-B{b}" for n, t, s, b in EXACT_CASES])
def test_gbuffer_bwd_exact_on_list_pattern(name, table, sw, B, dev, L):
    """Exact mode, B = 2 or 3 on 24 x 40 (B*H*W <= 2880 <= 2^16, the exactness condition of gbuffer_ref): every pattern under both table
    sizes, each with two of the five switch sets, so every switch value meets at least three patterns.  Measured on an MI355X: the clip
    columns use at most 0.041 of rast_bwd_reference's bound."""
    E, pb, with_tex, want_prior, want_clip, clear = SWITCHES[sw]
    case = _case(name, table, B, seed=sw)
    B = case["B"]
    t = G.exact_tensors(case, E=E, prior_batch=B if pb == "B" else 1, with_tex=with_tex, seed=sw)
    clip = _clip_of(case["xy"], True, B, sw) if want_clip else None
    ref, g_rast, _, _ = G.backward_reference(case, t, want_prior=bool(want_prior))
    got = run_bwd(L, dev, case, t, clip, want_prior, clear)
    assert torch.isfinite(got).all(), "a gradient row left poisoned"
    _assert_rows_equal(got[:, :12], ref[:, :12].float(), "columns 0..11")
    if not want_prior:
        assert torch.equal(got[:, 6:9], torch.zeros_like(got[:, 6:9]))
    if want_clip:
        cref, cbound, feeds = G.clip_reference(case, clip, g_rast)
        _check_rast(got[:, 12:16], cref, cbound, feeds)
        used = ((got[:, 12:16].double() - cref).abs() / cbound.clamp(min=1e-300))[:, [0, 1, 3]][feeds > 0]
        print(f"clip columns: {float(used.max()) if used.numel() else 0.0:.3f} of the bound")
    else:
        assert torch.equal(got[:, 12:16], torch.zeros_like(got[:, 12:16])), "clip = NULL: columns 12..15 stay 0"


def _normal_case(name, table, seed):
    case = _case(name, table, 2, seed)
    tiny = []
    if name == "unique":  # private vertices: a quarter of the triangles a factor >= 4 above resp. below the 1e-20 clamp of d
        tiny = ([(tr, (4e-20 * (4 + tr % 5)) ** 0.25) for tr in range(0, 64, 2)] + [(tr, (1e-20 / (8 + tr % 5)) ** 0.25) for tr in range(1, 64, 2)])
    return case, G.normal_tensors(case, seed, tiny=tiny)


@pytest.mark.parametrize("table", ["small", "big"])
@pytest.mark.parametrize("name", ["runs", "fan", "unique", "period8"])
def test_gbuffer_bwd_face_normal_adjoint_within_counted_bound(name, table, dev, L):
    """Normal mode: columns 0..2 within gbuffer_ref.vpos_bound per element (rounding count in vpos_terms' docstring), columns 3..8
    within attr_bound, the rest exactly 0 (no extra attribute, clip = NULL).  'unique' carries near-degenerate triangles on both sides of
    the clamp, each held to the bound of its own branch.  Measured on an MI355X: at most 0.39 of the bound in columns 0..2 (on 'unique', one term
    per row; 0.02 .. 0.13 on the others), 0.31 in columns 3..8; the same figures under both table sizes."""
    case, t = _normal_case(name, table, seed=5)
    ref, bound, feeds, _, _, _ = G.vpos_bound(case, t)
    full, _, _, _ = G.backward_reference(case, t)
    got = run_bwd(L, dev, case, t, None, 1, 0)
    assert torch.isfinite(got).all()
    err = (got[:, 0:3].double() - ref).abs()
    used = float((err / bound.clamp(min=1e-300))[feeds > 0].max())
    err_a = (got[:, 3:9].double() - full[:, 3:9]).abs()
    bound_a = G.attr_bound(case, t)
    used_a = float((err_a / bound_a.clamp(min=1e-300))[feeds > 0].max())
    print(f"{name} {table}: columns 0..2 use {used:.3f} of the bound, columns 3..8 {used_a:.3f}")
    bad = (err > bound).any(-1).nonzero().reshape(-1)
    assert bad.numel() == 0, (int(bad[0]), got[bad[0], 0:3].tolist(), ref[bad[0]].tolist(), bound[bad[0]].tolist())
    assert not bool((err_a > bound_a).any())
    assert torch.equal(got[feeds == 0], torch.zeros_like(got[feeds == 0])) and torch.equal(got[:, 9:], torch.zeros_like(got[:, 9:]))


# ------------------------------------------------------------------------------------------------ forward entry points
def _with_degenerates(case):
    """Two degenerate triangles among the private ones of 'unique': a repeated vertex index and (see _fwd_tensors) collinear vertices."""
    case["tri"][1] = [case["tri"][1][0], case["tri"][1][0], case["tri"][1][2]]
    return case


def _fwd_tensors(case, E, pb, seed, degenerate):
    t = G.exact_tensors(case, E=E, prior_batch=pb, seed=seed)
    if degenerate:
        i0, i1, i2 = case["tri"][0]
        t["v_pos"][:, i0], t["v_pos"][:, i1], t["v_pos"][:, i2] = torch.zeros(3), torch.tensor([1.0, 2.0, 3.0]), torch.tensor([2.0, 4.0, 6.0])
    return t


def _aux(L, dev, P, pad_to, rows, spare=5):
    """a3d_gb_aux over canary-filled buffers with ``spare`` rows behind the ``rows`` the struct declares."""
    tex = torch.full((rows + spare, 3), 777.0, device=dev)
    img = torch.full((rows + spare,), -7, dtype=torch.int64, device=dev)
    return L.GbAux(size=ctypes.sizeof(L.GbAux), tex_out=L.ptr(tex), img_out=L.ptr(img), rows=rows, pad_to=pad_to), tex, img


def _check_forward(case, t, out, ex, tex, img, pad_to, rows_declared, what):
    P, B = case["P"], case["B"]
    ref, ex_ref, live = G.forward_reference(case, t)
    out, ref32 = out.cpu(), ref.float()
    assert torch.isfinite(out).all(), what
    bad = (out[:, EXACT_FWD_COLS] != ref32[:, EXACT_FWD_COLS]).any(-1).nonzero().reshape(-1)
    assert bad.numel() == 0, (what, int(bad[0]), out[bad[0]].tolist(), ref[bad[0]].tolist())
    fn_err = float((out[:, 3:6].double() - ref[:, 3:6]).abs().max())
    print(f"{what}: worst face-normal error {fn_err / EPS:.2f} x 2^-24")
    assert fn_err <= 4 * EPS, (what, fn_err / EPS)
    assert torch.equal(out[~live], torch.zeros_like(out[~live])), "entries with f < 0 or f >= F are zero rows"
    if ex_ref is not None:
        assert torch.equal(ex.cpu(), ex_ref.float()), what
    if tex is not None:
        tex, img = tex.cpu(), img.cpu()
        assert torch.equal(tex[:P].view(torch.int32), out[:, 9:12].contiguous().view(torch.int32)), "tex_out == columns 9..11, bit for bit"
        assert torch.equal(img[:P], torch.from_numpy(case["b"])), "img_out == image of the pixel"
        end = P if pad_to <= 0 else min(-(-P // pad_to) * pad_to, rows_declared)
        assert torch.equal(tex[P:end], torch.zeros(end - P, 3)) and torch.equal(img[P:end], torch.full((end - P,), B - 1))
        assert torch.equal(tex[end:], torch.full_like(tex[end:], 777.0)) and torch.equal(img[end:], torch.full_like(img[end:], -7)), \
            "rows behind min(round_up(P, pad_to), rows) are untouched"
    return fn_err


FWD_CASES = [("unique", "small", 2, 0, "B", 64, 1), ("runs", "big", 3, 3, 1, 0, 0), ("holes256", "small", 2, 2, "B", 64, 2),
             ("holes257", "big", 2, 1, 1, 100, 3), ("holes1", "big", 2, 0, "B", 8, 0), ("fan", "small", 2, 0, 1, 1000, 1)]


@pytest.mark.parametrize("name,table,B,E,pb,pad_to,seed", FWD_CASES, ids=[f"{c[0]}-pad{c[5]}" for c in FWD_CASES])
def test_gbuffer_fwd_exact_rows_padding_and_row_clear(name, table, B, E, pb, pad_to, seed, dev, L):
    """a3d_gbuffer_fwd in exact mode: interpolated columns torch.equal to float64; the face normal (integer positions: cross product and
    d are exact, leaving sqrt, reciprocal and product) within 4 x 2^-24, degenerate triangles (repeated index, collinear) at the float64
    clamp; zero rows for dead entries; tex_out / img_out and their padding for pad_to = 0, P a multiple of pad_to, P = 1, and a declared
    row count below round_up(P, pad_to) ('fan': 1000 -> rows = P + 3); the gradient rows cleared whole.  Measured on an MI355X: worst
    face-normal error 1.65 x 2^-24 (both forward entry points)."""
    case = _case(name, table, B, seed)
    if name == "unique":
        case = _with_degenerates(case)
    B, V, F, P = case["B"], case["V"], case["F"], case["P"]
    t = _fwd_tensors(case, E, B if pb == "B" else 1, seed, name == "unique")
    d = {k: _d(v, dev) for k, v in t.items()}
    tri, pix = torch.from_numpy(case["tri"]).int().to(dev), torch.from_numpy(case["pix"]).to(dev)
    rows_declared = P + 3 if pad_to == 1000 else (-(-P // pad_to) * pad_to if pad_to else P)
    aux, tex, img = _aux(L, dev, P, pad_to, rows_declared)
    out, ex = _nan(dev, P, 12), (_nan(dev, P, E) if E else None)
    g_rows = _nan(dev, B, V, G.GB_ROW)
    L.call("a3d_gbuffer_fwd", L.ptr(d["rast"]), L.ptr(tri), L.ptr(pix), P, L.ptr(d["v_pos"]), L.ptr(d["v_nrm"]), L.ptr(d["prior"]),
           t["prior"].shape[0], B, V, F, H, W, L.ptr(out), L.ptr(d["extra"]), E, L.ptr(ex), L.ptr(g_rows), ctypes.addressof(aux), L.stream())
    torch.cuda.synchronize()
    _check_forward(case, t, out, ex, tex, img, pad_to, rows_declared, f"a3d_gbuffer_fwd {name}")
    assert torch.equal(g_rows.cpu(), torch.zeros(B, V, G.GB_ROW)), "g_rows_to_clear is cleared whole"
    if name == "unique":
        ref, _, _ = G.forward_reference(case, t)
        p = torch.from_numpy(case["f"])
        for tr in (0, 1):
            sel = (p == tr).nonzero().reshape(-1)
            assert sel.numel() and torch.equal(ref[sel, 3:6], torch.zeros(sel.numel(), 3, dtype=torch.float64))
            assert torch.equal(out.cpu()[sel, 3:6], torch.zeros(sel.numel(), 3)), "degenerate triangle: the clamp gives a zero normal"


def test_gbuffer_fwd_clears_more_rows_than_the_launch_has_threads(dev, L):
    """P = 1 (one work-group of 256 threads) and B*V*4 = 8000 float4 to clear, without aux and without an extra attribute."""
    B = 2
    case = G.make_list("holes", "big", B, 0, 1)
    case["V"] = 1000
    case = G.finish(case, B, H, W)
    t = G.exact_tensors(case)
    d = {k: _d(v, dev) for k, v in t.items()}
    tri, pix = torch.from_numpy(case["tri"]).int().to(dev), torch.from_numpy(case["pix"]).to(dev)
    out, g_rows = _nan(dev, 1, 12), _nan(dev, B, 1000, G.GB_ROW)
    assert B * 1000 * 4 > 256
    L.call("a3d_gbuffer_fwd", L.ptr(d["rast"]), L.ptr(tri), L.ptr(pix), 1, L.ptr(d["v_pos"]), L.ptr(d["v_nrm"]), L.ptr(d["prior"]), B, B, 1000,
           case["F"], H, W, L.ptr(out), None, 0, None, L.ptr(g_rows), None, L.stream())
    torch.cuda.synchronize()
    _check_forward(case, t, out, None, None, None, 0, 1, "P = 1")
    assert torch.equal(g_rows.cpu(), torch.zeros(B, 1000, G.GB_ROW))


COVER_CASES = [("runs", "small", 2, 0, "B", 64), ("holes257", "big", 2, 3, 1, 0), ("unique", "small", 3, 2, "B", 128), ("holes1", "big", 2, 0, 1, 16)]


@pytest.mark.parametrize("name,table,B,E,pb,pad_to", COVER_CASES, ids=[c[0] for c in COVER_CASES])
def test_cover_gbuffer_fwd_builds_the_list_and_the_same_rows(name, table, B, E, pb, pad_to, dev, L):
    """a3d_cover_gbuffer_fwd with scratch from a3d_cover_count on the same fabricated rasters: the list is the covered pixels (id > 0,
    ids out of range included) image-major, inv is its inverse, and the rows obey the checks of a3d_gbuffer_fwd for the list it built."""
    case = _case(name, table, B, 1)
    B, V, F = case["B"], case["V"], case["F"]
    t = G.exact_tensors(case, E=E, prior_batch=B if pb == "B" else 1, seed=1)
    covered = (t["rast"].reshape(-1, 4)[:, 3] > 0).nonzero().reshape(-1)
    P = covered.numel()
    d = {k: _d(v, dev) for k, v in t.items()}
    tri = torch.from_numpy(case["tri"]).int().to(dev)
    lib = L.lib()
    scratch = torch.empty(lib.a3d_cover_scratch_bytes(B, H, W) // 4, dtype=torch.int32, device=dev)
    L.call("a3d_cover_count", L.ptr(d["rast"]), B, H, W, 8, L.ptr(scratch), L.stream())
    nb, stride = lib.a3d_cover_blocks(B, H, W), lib.a3d_cover_group_stride()
    assert int(scratch[nb:nb + lib.a3d_cover_groups(B, H, W) * stride][::stride].sum()) == P
    rows_declared = -(-P // pad_to) * pad_to if pad_to else P
    aux, tex, img = _aux(L, dev, P, pad_to, rows_declared)
    pix = torch.full((P,), -1, dtype=torch.int64, device=dev)
    inv = torch.full((B * H * W,), -9, dtype=torch.int32, device=dev)
    out, ex = _nan(dev, P, 12), (_nan(dev, P, E) if E else None)
    g_rows = _nan(dev, B, V, G.GB_ROW)
    L.call("a3d_cover_gbuffer_fwd", L.ptr(d["rast"]), L.ptr(tri), B, V, F, H, W, L.ptr(scratch), P, L.ptr(pix), L.ptr(inv), L.ptr(d["v_pos"]),
           L.ptr(d["v_nrm"]), L.ptr(d["prior"]), t["prior"].shape[0], L.ptr(out), L.ptr(d["extra"]), E, L.ptr(ex), L.ptr(g_rows),
           ctypes.addressof(aux), L.stream())
    torch.cuda.synchronize()
    pix, inv = pix.cpu(), inv.cpu()
    assert torch.equal(torch.sort(pix)[0], covered), "the list holds every covered pixel once"
    assert torch.equal(pix // (H * W), torch.sort(pix // (H * W))[0]), "image-major"
    want_inv = torch.full((B * H * W,), -1, dtype=torch.int32)
    want_inv[pix] = torch.arange(P, dtype=torch.int32)
    assert torch.equal(inv, want_inv)
    listed = dict(case, pix=pix.numpy(), f=case["ids"].reshape(-1)[pix.numpy()], b=(pix // (H * W)).numpy(), P=P)
    _check_forward(listed, t, out, ex, tex, img, pad_to, rows_declared, f"a3d_cover_gbuffer_fwd {name}")
    assert torch.equal(g_rows.cpu(), torch.zeros(B, V, G.GB_ROW))


@pytest.mark.parametrize("B", [1, 3, 4, 5, 9])
def test_gbuffer_prior_grad_is_the_sum_over_images(B, dev, L):
    """gb_prior_sum_kernel (4-wide loop and its tail) on exact rows: multiples of 1/16 in [-64, 64] in columns 6..8 (every partial sum
    exact), NaN in every column it must not read; torch.equal to the float64 sum."""
    V = 300
    rng = np.random.default_rng(B)
    rows = torch.full((B, V, G.GB_ROW), float("nan"))
    rows[..., 6:9] = torch.from_numpy(rng.integers(-1024, 1025, (B, V, 3)) / 16.0).float()
    ref = rows[..., 6:9].double().sum(0)
    rows_d, got = rows.to(dev), _nan(dev, 1, V, 3)
    L.call("a3d_gbuffer_prior_grad", L.ptr(rows_d), B, V, L.ptr(got), L.stream())
    torch.cuda.synchronize()
    assert torch.equal(got.cpu()[0], ref.float()) and torch.equal(ref.float().double(), ref)
