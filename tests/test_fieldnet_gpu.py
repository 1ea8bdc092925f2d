"""The field networks' oldest kernels on the GPU -- csrc/gemm.hip, csrc/segsum.hip, csrc/embed.hip through their ops wrappers, and the chain
hostnets._stack_backward builds from them -- against the float64 statements of tests/fieldnet_ref.py, on the shapes where such kernels go
wrong: below one tile, ragged tiles, the persistent GEMM's second sweep, every column layout of the segment sums, image boundaries on and
beside block edges, empty images and lists, zeros of both signs, denormals, huge arguments and non-finite rows.  Every quantity's error
statistic stays within 4x of what a plain float32 evaluation reaches on the same inputs (the CPU's mm / index_add_; for the embedding the
torch expression on this GPU), masks are threshold_backward's bit for bit, the GEMM has the same bits on every run, a NaN passes the fused
ReLU as it passes torch.relu, and guard mode finds no canary touched.

Measured on MI355X (largest statistic over all cases | largest ratio to the float32 evaluation's figure for the same row count; the bar is 4):
    gemm, K = 256          2.13 | 2.03 (M = 32)      second sweep, M = 65569: 2.56 | 1.42
    gemm, other K          2.19 | 1.69 (M = 127)
    segsum                 1.15 | 1.00               masked segsum 1.05 | 0.95      add_relu 0.25 | 1.00 (torch's bits)
    embedding fwd          0.54 | 1.00               embedding bwd 0.65 | 1.00      (forward: torch's bits on every input, 1e4 f_k included)
    chain  g_x 0.28 | 2.16   g_in 0.64 | 1.97   g_rows 0.83 | 2.44 (M = 48)   g_first 1.03 | 1.57   g_hidden 1.18 | 1.16
The sums of one term or none (one row per image, P = 1, the empty list) are exact on both sides: statistic 0 against a floor of 0.
Nothing exceeded the bar; the one change the tests forced on a kernel is the NaN-propagating ReLU of ss_add_relu*_kernel.
"""
import functools
import importlib
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fieldnet_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _ops():
    return importlib.import_module("3danimals_amd.ops")


def _L():
    return importlib.import_module("3danimals_amd._lib")


def _hostnets():
    return importlib.import_module("3danimals_amd.hostnets")


def _bits(t):
    return t.view(torch.int32)


def _no_nan(t):
    return torch.where(t.isnan(), torch.full_like(t, 7.0), t)


def _report(quantity, rows, value, floor):
    print(f"FIG {quantity} rows={rows} stat={value:.4f} floor={floor:.4f} ratio={value / floor if floor else 0.0:.3f}")


# ------------------------------------------------------------------------------------------------------------------ GEMM
def _gemm(inp, masked, a=None):
    return _ops().gemm_nn_relumask((inp["a"] if a is None else a).cuda(), inp["b"].cuda(), inp["x"].cuda() if masked else None)


def _gemm_case(m, k, quantity, floor, rows_named=None):
    inp = R.make_gemm_inputs(m, k)
    assert R.has_the_special_values(inp["x"])
    for masked in ((False, True) if k >= 256 else (False,)):
        got = _gemm(inp, masked)
        v = R.check_gemm(got.cpu(), inp, masked, R.MARGIN * floor, f"gemm M={m} K={k} masked={masked}", rows_named)
        _report(quantity, m, v, floor)
        assert torch.equal(_bits(got), _bits(_gemm(inp, masked)))  # the same bits on a second run
        if masked:  # the denormal passes; 0.0, -0.0 and -1.5 do not
            assert got[0, 2] != 0 and got[m - 1, 132] != 0 and not got[0, :2].any() and got[0, 3] == 0 and got[m - 1, 131] == 0


@pytest.mark.parametrize("m", R.GEMM256_ROWS)
def test_persistent_gemm_against_float64(m):
    _gemm_case(m, 256, "gemm256", R.noise_floor()["gemm256", m])


@pytest.mark.parametrize("k", R.GEMM_OTHER_K)
def test_block_tiled_gemm_against_float64(k):
    for m in R.GEMM_OTHER_ROWS:
        _gemm_case(m, k, "gemm_k", R.noise_floor()["gemm_k", m])


def test_persistent_gemm_second_sweep_against_float64():
    """M_wrap: the first M at which a wave takes a second tile (its accumulators, its prefetch registers and its sign words in LDS are used
    again), the second sweep being one full tile and a ragged one of one row.  Checked in full; a failure names the second sweep's rows."""
    n_cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    m = R.m_wrap(n_cu)
    rows = list(R.second_sweep_rows(n_cu, m))
    assert len(rows) == 33 and rows[-1] == m - 1
    _gemm_case(m, 256, "gemm256_wrap", R.gemm_floor(256, m), rows_named=rows)


@pytest.mark.parametrize("k,m", [(256, m) for m in R.GEMM256_ROWS] + [(288, 33), (288, 129), (512, 129), (512, 257)])
def test_gemm_keeps_non_finite_rows_to_themselves(k, m):
    """An infinity in one row of A and a NaN in another (the last: the row the clamped loads of a ragged tile repeat): their masked entries are
    still +0.0 (a select, not a product with 0), their unmasked ones non-finite, and every other row has the bits it has without them."""
    inp = R.make_gemm_inputs(m, k)
    dirty = R.with_nonfinite_rows(inp["a"])
    bad = [r for r in R.nonfinite_rows(m) if r is not None]
    keep = torch.ones(m, dtype=torch.bool)
    keep[bad] = False
    for masked in (True, False):
        clean, got = _gemm(inp, masked).cpu(), _gemm(inp, masked, dirty).cpu()
        assert torch.equal(_bits(got[keep]), _bits(clean[keep])), (k, m, masked)
        passes = inp["x"][bad] > 0 if masked else torch.ones(len(bad), R.N, dtype=torch.bool)
        assert not bool(torch.isfinite(got[bad][passes]).any()) and bool((_bits(got[bad])[~passes] == 0).all()), (k, m, masked)


def test_wrappers_refuse_a_cpu_mask_and_a_cpu_index_beside_gpu_operands(monkeypatch):
    """A host pointer that reaches a kernel is a GPU fault, not a wrong number: ops.call is replaced by a recorder here, so a wrapper that
    loses its device check fails this test instead of launching."""
    ops, A3DError = _ops(), _L().A3DError
    calls = []
    monkeypatch.setattr(ops, "call", lambda *a, **k: calls.append(a[0]))
    inp = R.make_gemm_inputs(33, 256)
    s = R.make_seg_inputs("one image, 129 rows", 64)
    for fn, args in ((ops.gemm_nn_relumask, (inp["a"].cuda(), inp["b"].cuda(), inp["x"])), (ops.gemm_nn_relumask, (inp["a"].cuda(), inp["b"], None)),
                     (ops.rows_segsum_raw, (s["g"].cuda(), s["img"], 1)), (ops.rows_add_relu_raw_, (s["y"].cuda(), s["rows"].cuda(), s["img"])),
                     (ops.rows_add_relu_raw_, (s["y"].cuda(), s["rows"], s["img"].cuda())), (ops.rows_add_relu_, (s["y"].cuda(), s["rows"].cuda(), s["img"])),
                     (ops.harmonic_embed, (torch.zeros(5, 3).cuda(), R.embed_freq(4)))):
        with pytest.raises(A3DError, match="no CPU fallback"):
            fn(*args)
    assert calls == []


# ------------------------------------------------------------------------------------------------------------------ segment sums
def _masked_segsum(g, y, img, b):
    """a3d_rows_add_relu_bwd on a y of its own (through autograd it only ever sees a ReLU's output); buffers from ops' allocator, so that
    guard mode wraps them."""
    ops, L = _ops(), _L()
    g_pre = ops.torch.empty_like(g)
    g_rows = ops.torch.empty((b, g.shape[1]), dtype=torch.float32, device=g.device)
    L.call("a3d_rows_add_relu_bwd", L.ptr(g), L.ptr(y), L.ptr(img), g.shape[0], g.shape[1], b, L.ptr(g_pre), L.ptr(g_rows), L.stream())
    return g_pre, g_rows


def _seg_case(layout, c, floor=None):
    ops = _ops()
    inp = R.make_seg_inputs(layout, c)
    p, b = inp["g"].shape[0], inp["b"]
    g, y, rows, img = (inp[k].cuda() for k in ("g", "y", "rows", "img"))
    bar = lambda q: float("inf") if floor is None else R.MARGIN * floor[q, p]
    what = f"{layout}, C={c}"
    res = dict(segsum=R.check_segsum(ops.rows_segsum_raw(g, img, b), inp, bar("segsum"), "segsum " + what))
    g_pre, g_rows = _masked_segsum(g, y, img, b)
    assert torch.equal(_bits(g_pre), _bits(torch.ops.aten.threshold_backward(g, y, 0)))
    res["masked_segsum"] = R.check_masked_segsum(g_pre, g_rows, inp, bar("masked_segsum"), "masked segsum " + what)
    out = ops.rows_add_relu_raw_(y.clone(), rows, img)
    assert torch.equal(out, torch.relu(y + rows[img])), what
    res["add_relu"] = R.within(R.statistic(out.cpu(), *R.rows_add_relu_ref(inp["y"], inp["rows"], inp["img"])), bar("add_relu"), "add_relu " + what)
    if floor is not None:
        for q, v in res.items():
            _report(q, p, v, floor[q, p])
    return res


@pytest.mark.parametrize("c", R.SEG_CHANNELS)
def test_segment_sums_and_rows_add_relu_against_float64(c):
    """Every layout of fieldnet_ref.SEG_LAYOUTS at this width: the plain sums, the masked sums with their g_pre (bitwise
    threshold_backward), and relu(y + rows[img]) (exactly torch's).  An image without points gets +0.0, an empty list all zeros."""
    floor = R.noise_floor()
    for layout in R.SEG_LAYOUTS:
        _seg_case(layout, c, floor)


@pytest.mark.parametrize("c", (52, 260))  # the scalar and the float4 kernel
def test_rows_add_relu_propagates_nan_like_torch_relu(c):
    """fmaxf(NaN, 0) is 0: a diverged field would read as a dead one a layer later.  -0.0 and a negative sum become +0.0, as torch.relu's."""
    ops = _ops()
    inp = R.make_seg_inputs("boundaries beside block edges", c)
    y, rows, img = inp["y"].clone(), inp["rows"].clone(), inp["img"]
    y[3, 1] = y[130, c - 1] = y[383, 7] = float("nan")
    rows[2, 9] = float("nan")  # a NaN in a per-image row reaches every point of that image
    y[200, 5], rows[1, 5] = float("-inf"), 1.0
    y[201, 5] = float("inf")
    yd, rd, im = y.cuda(), rows.cuda(), img.cuda()
    want = torch.relu(yd + rd[im])
    for fn in (ops.rows_add_relu_raw_, ops.rows_add_relu_):
        out = fn(yd.clone(), rd, im)
        assert torch.equal(out.isnan(), want.isnan()) and int(out.isnan().sum()) == 3 + 127
        assert torch.equal(_no_nan(out), _no_nan(want))
        assert out[200, 5] == 0 and out[201, 5] == float("inf") and bool((_bits(out)[out == 0] == 0).all())


def test_rows_add_relu_autograd_path_matches_the_statements():
    ops = _ops()
    inp = R.make_seg_inputs("boundaries beside block edges", 256)
    y0 = inp["y"].cuda().requires_grad_(True)
    rows = inp["rows"].cuda().requires_grad_(True)
    img, g = inp["img"].cuda(), inp["g"].cuda()
    out = ops.rows_add_relu_(y0 * 1.0, rows, img)
    g_y, g_r = torch.autograd.grad(out, (y0, rows), g)
    assert torch.equal(out.detach(), torch.relu(y0 + rows[img]).detach())
    assert torch.equal(_bits(g_y), _bits(torch.ops.aten.threshold_backward(g, out.detach(), 0)))
    relu_out = dict(inp, y=out.detach().cpu())
    R.check_masked_segsum(g_y, g_r, relu_out, R.MARGIN * R.noise_floor()["masked_segsum", 384])


# ------------------------------------------------------------------------------------------------------------------ embedding
def _emb(n):
    return _hostnets().HarmonicEmbedding(n, R.EMBED_SCALAR)


@functools.lru_cache(maxsize=None)
def _embed_floor():
    floor = R.embed_floor(torch.device("cuda"), _emb)
    print({k: round(v, 4) for k, v in floor.items()})
    return floor


@pytest.mark.parametrize("n,symmetrize,ones", R.EMBED_CONFIGS)
def test_embedding_against_float64_on_the_new_inputs(n, symmetrize, ones):
    ops, floor = _ops(), _embed_floor()
    emb, f = _emb(n), R.embed_freq(n)
    fd = emb._frequencies(torch.device("cuda", torch.cuda.current_device()))
    assert torch.equal(fd.cpu(), f)
    for p in R.EMBED_ROWS:
        x, gen = R.make_embed_inputs(n, p)
        w = R.embed_weights(x, n, ones, gen)
        xa = x.cuda().requires_grad_(True)
        got = ops.harmonic_embed(xa, fd, symmetrize=symmetrize, ones=ones)
        (g_x,) = torch.autograd.grad((got * w.cuda()).sum(), xa)
        want, _ = R.embed_float32(x.cuda(), emb, symmetrize, ones)
        differ = int((_bits(got.detach()) != _bits(want)).sum())
        print(f"n={n} symmetrize={symmetrize} ones={ones} P={p}: {differ} entries differ from the torch expression on the bits")
        v = R.check_embed_fwd(got.detach(), x, f, symmetrize, ones, R.MARGIN * floor["embed_fwd", p], f"embed fwd n={n} P={p}")
        _report("embed_fwd", p, v, floor["embed_fwd", p])
        v = R.check_embed_bwd(g_x, w, x, f, symmetrize, ones, R.MARGIN * floor["embed_bwd", p], f"embed bwd n={n} P={p}")
        _report("embed_bwd", p, v, floor["embed_bwd", p])
        if symmetrize:
            assert bool((g_x[:, 0][xa[:, 0] == 0] == 0).all()) and (p == 1 or int((x[:, 0] == 0).sum()) >= 2)
        if (n, symmetrize, ones) in R.EMBED_CONFIGS[:3]:  # where the parity test demands it of |x| <= 3.5
            assert torch.equal(got.detach(), want), (n, p, differ)
        # an infinity and a NaN stay in their own rows, and are what the torch expression makes of them
        xn, _ = R.make_embed_inputs(n, p, nonfinite=True)
        with torch.no_grad():
            gn = ops.harmonic_embed(xn.cuda(), fd, symmetrize=symmetrize, ones=ones)
        wn, _ = R.embed_float32(xn.cuda(), emb, symmetrize, ones)
        assert torch.equal(_bits(gn[:p]), _bits(got.detach())) and bool(torch.isfinite(gn[:p]).all())
        assert torch.equal(gn.isnan(), wn.isnan())
        if (n, symmetrize, ones) in R.EMBED_CONFIGS[:3]:
            assert torch.allclose(gn, wn, rtol=0, atol=0, equal_nan=True)
        s = slice(3, 3 + 6 * n)
        nan_cols = lambda c: torch.tensor([(j % (3 * n)) // n == c for j in range(6 * n)])
        assert torch.equal(gn[p, s].isnan().cpu(), nan_cols(1)) and gn[p, 1] == float("inf")  # sin / cos of an infinity
        assert torch.equal(gn[p + 1, s].isnan().cpu(), nan_cols(0)) and bool(gn[p + 1, 0].isnan())
        assert not ones or bool((gn[:, -1] == 1).all())


# ------------------------------------------------------------------------------------------------------------------ the stack's backward chain
def _chain_on_gpu(inp):
    hostnets = _hostnets()
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}
    hidden = [w.cuda() for w in inp["hidden"]]
    ys = hostnets._stack_forward(dev["x_emb"], dev["w_in"], dev["per_image"], dev["index"], dev["w_first"], hidden)
    g = torch.ops.aten.threshold_backward(dev["g_out"], ys[-1], 0)
    out = hostnets._stack_backward(g, dev["x_emb"], dev["w_in"], dev["index"], dev["w_first"], hidden, ys, inp["n_images"], True)
    return g, ys, dict(zip(R.CHAIN_QUANTITIES, out))


@pytest.mark.parametrize("m", R.CHAIN_ROWS)
def test_stack_backward_chain_against_float64(m):
    """_stack_backward's five outputs against the float64 chain over the SAME g, weights and float32 ys (from _stack_forward itself, so the
    masks are the ones the GPU saw); the per-image gradient of the empty image is exactly 0."""
    floor = R.noise_floor()
    for n_hidden, with_feat in R.CHAIN_CASES:
        inp = R.make_chain_inputs(m, n_hidden, with_feat)
        g, ys, got = _chain_on_gpu(inp)
        assert len(ys) == 1 + int(with_feat) + n_hidden and len(got["g_hidden"]) == n_hidden
        cpu = {k: (None if v is None else [t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in got.items()}
        stats = R.chain_statistics(cpu, g.cpu(), inp, [y.cpu() for y in ys])
        assert set(stats) == set(R.CHAIN_QUANTITIES) - (set() if with_feat else {"g_rows", "g_first"})
        for name, v in stats.items():
            _report(name, m, v, floor[name, m])
        for name, v in stats.items():
            R.within(v, R.MARGIN * floor[name, m], f"{name} M={m} hidden={n_hidden} feat={with_feat}")
        if with_feat:
            assert bool((_bits(got["g_rows"][1]) == 0).all()) and bool(got["g_rows"][0].any()) and bool(got["g_rows"][2].any())


# ------------------------------------------------------------------------------------------------------------------ guard mode
def test_guard_mode_finds_no_canary_touched_on_the_ragged_cases():
    L, ops = _L(), _ops()
    prev = L.set_guard(1)
    try:
        before = dict(L.guard_stats)
        for m, k in ((1, 256), (33, 256), (4099, 256), (1, 32), (129, 288), (257, 512)):
            inp = R.make_gemm_inputs(m, k)
            assert _gemm(inp, k >= 256).shape == (m, R.N)
            L.guard_check("test_fieldnet_gpu gemm")
        for layout, c in itertools.product(("one image, 1 row", "one image, 129 rows", "boundaries beside block edges", "one row per image", "empty list"),
                                           (1, 17, 260, 1028)):
            _seg_case(layout, c)
            L.guard_check("test_fieldnet_gpu segsum")
        for (n, symmetrize, ones), p in itertools.product(R.EMBED_CONFIGS, (1, 257)):
            x, gen = R.make_embed_inputs(n, p)
            xa = x.cuda().requires_grad_(True)
            got = ops.harmonic_embed(xa, R.embed_freq(n).cuda(), symmetrize=symmetrize, ones=ones)
            torch.autograd.grad((got * R.embed_weights(x, n, ones, gen).cuda()).sum(), xa)
            L.guard_check("test_fieldnet_gpu embed")
        assert L.guard_stats["checks"] >= before["checks"] + 6 + 20 * 3 + 8 * 2 and L.guard_stats["allocations"] >= before["allocations"] + 6 + 16 * 3 + 8 * 2
    finally:
        L.set_guard(prev)
