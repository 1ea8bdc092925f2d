"""The field networks' GEMM, segment-sum and embedding kernels without a GPU: the six entry points and their five Python wrappers refuse what
they would misread before anything is launched, the float64 statements of tests/fieldnet_ref.py are what float64 autograd gives, the inputs
hold their special values, the noise floor the GPU test is held to is finite (and printed), and the assertion helpers the GPU test uses
reject nine wrong results built here on purpose."""
import importlib
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fieldnet_ref as R  # noqa: E402

FAKE = 0x1000  # non-NULL, 16-byte aligned, never dereferenced


def _L():
    return importlib.import_module("3danimals_amd._lib")


def _ops():
    return importlib.import_module("3danimals_amd.ops")


# ------------------------------------------------------------------------------------------------------------------ entry points
def test_entry_points_refuse_invalid_arguments_before_anything_is_launched():
    """None of the pointers below is ever dereferenced and nothing is launched (this runs without a GPU)."""
    lib = _L().lib()

    def refused(fn, good, **bad):
        assert getattr(lib, fn)(*dict(good, **bad).values(), None) == -1, (fn, bad)
        msg = lib.a3d_last_error().decode()
        assert "invalid argument" in msg and fn in msg, (fn, bad, msg)

    gemm = dict(A=FAKE, B=FAKE, X=FAKE, M=100, N=256, K=256, C=FAKE)
    for bad in (dict(N=128), dict(N=0), dict(K=0), dict(K=48), dict(K=-32), dict(K=64), dict(M=-1), dict(M=(1 << 31) - 1), dict(M=1 << 31),
                dict(A=None), dict(B=None), dict(C=None), dict(A=FAKE + 4), dict(B=FAKE + 8), dict(X=FAKE + 4)):
        refused("a3d_gemm_nn_relumask", gemm, **bad)  # (K = 64 with X: the mask is gathered over the first 8 chunks)
    refused("a3d_gemm_nn_relumask", gemm, K=512, X=FAKE + 12)
    refused("a3d_gemm_nn_relumask", gemm, K=64, X=None, A=FAKE + 4)

    seg = dict(g=FAKE, img=FAKE, P=100, C=64, B=3, out=FAKE)
    for bad in (dict(B=0), dict(B=-1), dict(C=0), dict(C=-4), dict(P=-1), dict(g=None), dict(img=None), dict(out=None), dict(g=FAKE + 4),
                dict(g=FAKE + 8, C=1028)):
        refused("a3d_rows_segsum", seg, **bad)
    fwd = dict(y=FAKE, rows=FAKE, img=FAKE, P=100, C=64, B=3)
    for bad in (dict(B=0), dict(C=0), dict(P=-1), dict(y=None), dict(rows=None), dict(img=None), dict(y=FAKE + 4), dict(rows=FAKE + 8),
                dict(y=FAKE + 4, C=4)):
        refused("a3d_rows_add_relu_fwd", fwd, **bad)
    bwd = dict(g=FAKE, y=FAKE, img=FAKE, P=100, C=64, B=3, g_pre=FAKE, g_rows=FAKE)
    for bad in (dict(B=0), dict(C=0), dict(P=-1), dict(g=None), dict(y=None), dict(img=None), dict(g_pre=None), dict(g_rows=None),
                dict(g=FAKE + 4), dict(y=FAKE + 8), dict(g_pre=FAKE + 4)):
        refused("a3d_rows_add_relu_bwd", bwd, **bad)
    efwd = dict(x=FAKE, freq=FAKE, n=10, symmetrize=1, ones=1, P=100, out=FAKE)
    ebwd = dict(g_out=FAKE, x=FAKE, freq=FAKE, n=10, symmetrize=1, ones=1, P=100, g_x=FAKE)
    for fn, good, ptrs in (("a3d_harmonic_embed_fwd", efwd, ("x", "freq", "out")), ("a3d_harmonic_embed_bwd", ebwd, ("g_out", "x", "freq", "g_x"))):
        for bad in [dict(n=0), dict(n=-1), dict(ones=2), dict(ones=-1), dict(P=-1)] + [{k: None} for k in ptrs]:
            refused(fn, good, **bad)


def test_entry_points_accept_an_empty_list_without_a_launch():
    lib = _L().lib()
    assert lib.a3d_gemm_nn_relumask(None, None, None, 0, 256, 256, None, None) == 0
    assert lib.a3d_rows_add_relu_fwd(None, None, None, 0, 64, 3, None) == 0
    assert lib.a3d_harmonic_embed_fwd(None, None, 10, 1, 1, 0, None, None) == 0
    assert lib.a3d_harmonic_embed_bwd(None, None, None, 10, 1, 1, 0, None, None) == 0


# ------------------------------------------------------------------------------------------------------------------ wrappers
@pytest.fixture
def recorder(monkeypatch):
    """ops.call replaced by a recorder: no wrapper below may reach it."""
    ops, calls = _ops(), []
    monkeypatch.setattr(ops, "call", lambda *a, **k: calls.append(a[0]))
    yield ops, calls
    assert calls == []


def test_wrappers_raise_value_errors_on_shapes_and_types_before_the_device_check(recorder):
    ops, _ = recorder
    z = torch.zeros
    img = z(5, dtype=torch.int64)
    for a, b, x in ((z(5, 256), z(256, 128), None), (z(5, 256), z(128, 256), None), (z(5, 48), z(48, 256), None), (z(5, 0), z(0, 256), None),
                    (z(5, 256), z(256), None), (z(256), z(256, 256), None), (z(5, 256), z(256, 256), z(4, 256)), (z(5, 256), z(256, 256), z(5, 128)),
                    (z(5, 256), z(256, 256), z(5, 256, dtype=torch.float64)), (z(5, 256), z(256, 256), z(5, 512)[:, ::2]),
                    (z(5, 64), z(64, 256), z(5, 256))):
        with pytest.raises(ValueError, match="gemm_nn_relumask"):
            ops.gemm_nn_relumask(a, b, x)
    bad_img = (z(5, dtype=torch.int32), z(10, dtype=torch.int64)[::2], z(4, dtype=torch.int64), z(5, 1, dtype=torch.int64), z(5))
    for fn in (ops.rows_add_relu_raw_, ops.rows_add_relu_):
        for y, rows, i in [(z(5, 64), z(3, 64), i) for i in bad_img] + [(z(5, 64), z(3, 32), img), (z(5, 64), z(64), img), (z(5, 64), z(0, 64), img),
                                                                         (z(5, 128)[:, ::2], z(3, 64), img), (z(5, 64, dtype=torch.float64), z(3, 64), img),
                                                                         (z(5, 64, dtype=torch.float16), z(3, 64), img), (z(64), z(3, 64), img)]:
            with pytest.raises(ValueError, match="rows_add_relu"):
                fn(y, rows, i)
    for g, i, b in [(z(5, 64), i, 3) for i in bad_img] + [(z(5, 64), img, 0), (z(5, 64), img, -1), (z(64), img, 3), (z(5, 0), img, 3)]:
        with pytest.raises(ValueError, match="rows_segsum_raw"):
            ops.rows_segsum_raw(g, i, b)
    for x, f in ((z(5, 2), z(4)), (z(5), z(4)), (z(5, 3), z(4, 1)), (z(5, 3), z(0)), (z(5, 3, dtype=torch.int64), z(4)), (z(5, 3), z(4, dtype=torch.int32))):
        with pytest.raises(ValueError, match="harmonic_embed"):
            ops.harmonic_embed(x, f)


def test_wrappers_raise_on_any_cpu_operand(recorder):
    """On the CPU every operand is one; the device check names the wrapper and is the last refusal before the entry point."""
    ops, _ = recorder
    A3DError = _L().A3DError
    z = torch.zeros
    img = z(5, dtype=torch.int64)
    with pytest.raises(A3DError, match="gemm_nn_relumask.*no CPU fallback"):
        ops.gemm_nn_relumask(z(5, 256), z(256, 256))
    with pytest.raises(A3DError, match="gemm_nn_relumask.*no CPU fallback"):
        ops.gemm_nn_relumask(z(5, 256), z(256, 256), z(5, 256))
    with pytest.raises(A3DError, match="rows_add_relu_raw_.*no CPU fallback"):
        ops.rows_add_relu_raw_(z(5, 64), z(3, 64), img)
    with pytest.raises(A3DError, match="rows_add_relu_.*no CPU fallback"):
        ops.rows_add_relu_(z(5, 64), z(3, 64), img)
    with pytest.raises(A3DError, match="rows_segsum_raw.*no CPU fallback"):
        ops.rows_segsum_raw(z(5, 64), img, 3)
    with pytest.raises(A3DError, match="harmonic_embed.*no CPU fallback"):
        ops.harmonic_embed(z(5, 3), z(4))


def test_device_check_covers_every_operand_the_mask_and_the_index_included(recorder, monkeypatch):
    """(Without a GPU no operand can pass the check and another fail it: look at what each wrapper hands to it.)"""
    ops, _ = recorder
    A3DError = _L().A3DError
    seen = []

    def spy(*tensors, what="op"):
        seen.append(tensors)
        raise A3DError(what)

    monkeypatch.setattr(ops, "require_device", spy)
    z = torch.zeros
    a, b, x, y, rows, img = z(5, 256), z(256, 256), z(5, 256), z(5, 64), z(3, 64), z(5, dtype=torch.int64)
    for fn, args, checked in ((ops.gemm_nn_relumask, (a, b, x), (a, b, x)), (ops.rows_add_relu_raw_, (y, rows, img), (y, rows, img)),
                              (ops.rows_add_relu_, (y, rows, img), (y, rows, img)), (ops.rows_segsum_raw, (y, img, 3), (y, img)),
                              (ops.harmonic_embed, (z(5, 3), z(4)), ())):
        del seen[:]
        with pytest.raises(A3DError):
            fn(*args)
        assert len(seen) == 1 and all(any(t is c for t in seen[0]) for c in checked), fn.__name__
        assert fn is not ops.harmonic_embed or sum(t is not None for t in seen[0]) == 2


def test_sorted_index_contract_is_stated_and_checked():
    """The segment sums take a NON-DECREASING index.  A list of at most 128 rows that starts and ends in image 0 with other images in between
    is outside the contract (the kernel sums it into image 0 whole: first == last reads as one image); CHECK_SORTED_INDEX reports it."""
    ops = _ops()
    bad = torch.tensor([0] * 40 + [1] * 30 + [2] * 30 + [0] * 20)
    assert bad.shape[0] <= 128 and bad[0] == bad[-1] == 0 and not R.is_sorted_index(bad)
    for layout in R.SEG_LAYOUTS:
        assert R.is_sorted_index(R.make_seg_inputs(layout, 3)["img"]), layout
    assert "non-decreasing" in ops._assert_sorted.__doc__.lower() and "NON-DECREASING" in ops.rows_per_point.__doc__
    assert ops.CHECK_SORTED_INDEX is False
    ops._assert_sorted(bad)  # off: no check, no cost
    ops.CHECK_SORTED_INDEX = True
    try:
        ops._assert_sorted(R.make_seg_inputs("padded tail", 3)["img"])
        ops._assert_sorted(torch.zeros(0, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="non-decreasing"):
            ops._assert_sorted(bad)
    finally:
        ops.CHECK_SORTED_INDEX = False


# ------------------------------------------------------------------------------------------------------------------ statements
def _close(a, b, rtol=1e-12):
    return torch.allclose(a, b, rtol=rtol, atol=rtol * float(b.abs().max()) * 1e-2 + 1e-300)


def test_gemm_and_segment_sum_statements_are_what_autograd_gives():
    inp = R.make_gemm_inputs(37, 256, seed=1)
    z = torch.randn(37, 256, generator=torch.Generator().manual_seed(2)).double().requires_grad_(True)
    b = inp["b"].double()
    g = inp["a"].double()
    (g_z,) = torch.autograd.grad(torch.relu(z) @ b.t(), z, g)  # the adjoint of x = relu(z), out = x B^T (a Linear with weight B) is (g . B) * (z > 0)
    x = torch.relu(z).detach().float()
    ref, terms = R.gemm_ref(inp["a"], inp["b"], x)
    assert _close(ref, g_z) and torch.equal(ref != 0, (z > 0).detach())
    assert _close(R.gemm_ref(inp["a"], inp["b"])[0], g @ b) and bool((terms >= ref.abs()).all())
    # per-image rows: out = relu(y + rows[img]); its adjoints are g_pre = g * (out > 0) and the segment sums of g_pre
    s = R.make_seg_inputs("boundaries beside block edges", 17, seed=1)
    y, rows = s["y"].double().requires_grad_(True), s["rows"].double().requires_grad_(True)
    out = torch.relu(y + rows[s["img"]])
    g_y, g_r = torch.autograd.grad(out, (y, rows), s["g"].double())
    assert _close(R.rows_add_relu_ref(s["y"], s["rows"], s["img"])[0], out.detach())
    g_pre, g_rows, _ = R.masked_segsum_ref(s["g"], out.detach().float(), s["img"], s["b"])
    assert torch.equal(g_pre, g_y) and _close(g_rows, g_r)
    assert _close(R.segsum_ref(s["g"], s["img"], s["b"])[0], torch.stack([s["g"].double()[s["img"] == i].sum(0) for i in range(s["b"])]))


@pytest.mark.parametrize("n,symmetrize,ones", R.EMBED_CONFIGS)
def test_embedding_statements_are_what_autograd_gives(n, symmetrize, ones):
    """With the float32 product taken as given: away from where it rounds differently, d fl32(x f) / dx is f (f is a power of two times one
    constant, so the product's rounding error is that of the constant's mantissa and does not depend on x's exponent)."""
    x, gen = R.make_embed_inputs(n, 257, seed=1)
    w = R.embed_weights(x, n, ones, gen)
    f = R.embed_freq(n)
    xs, ang = R._embed_angles(x, f, symmetrize)
    xd = x.double().requires_grad_(True)
    xa = torch.cat([xd[:, :1].abs(), xd[:, 1:]], -1) if symmetrize else xd
    delta = ang - (xs.double()[:, :, None] * f.double()).reshape(x.shape[0], -1)  # what rounding the product to float32 moved
    a = (xa[:, :, None] * f.double()).reshape(x.shape[0], -1) + delta
    out = torch.cat([xa, a.sin(), a.cos()] + ([torch.ones(x.shape[0], 1, dtype=torch.float64)] if ones else []), -1)
    (g_x,) = torch.autograd.grad((out * w.double()).sum(), xd)
    assert _close(R.embed_ref(x, f, symmetrize, ones), out.detach())
    ref, terms = R.embed_grad_ref(w, x, f, symmetrize, ones)
    assert _close(ref, g_x) and bool((terms >= ref.abs() * (1 - 1e-12)).all())
    if symmetrize:
        assert bool((ref[:, 0][x[:, 0] == 0] == 0).all()) and int((x[:, 0] == 0).sum()) >= 4


@pytest.mark.parametrize("n_hidden,with_feat", R.CHAIN_CASES)
def test_chain_statement_is_what_autograd_gives(n_hidden, with_feat):
    inp = R.make_chain_inputs(48, n_hidden, with_feat, seed=1)
    leaves = {k: inp[k].double().requires_grad_(True) for k in ("x_emb", "w_in", "per_image", "w_first") if inp[k] is not None}
    hidden = [w.double().requires_grad_(True) for w in inp["hidden"]]
    ys = R.chain_forward(dict(inp, hidden=hidden, **leaves), torch.float64)
    names = list(leaves)
    grads = torch.autograd.grad(ys[-1], [leaves[k] for k in names] + hidden, inp["g_out"].double())
    by = dict(zip(names, grads[:len(names)]))
    ys = [y.detach() for y in ys]
    g = inp["g_out"].double() * (ys[-1] > 0)
    val, trm = R.chain_backward(g, inp, ys)
    assert _close(val["g_x"], by["x_emb"]) and _close(val["g_in"], by["w_in"])
    for a, b in zip(val["g_hidden"], grads[len(names):]):
        assert _close(a, b)
    if with_feat:
        assert _close(val["g_rows"], by["per_image"]) and _close(val["g_first"], by["w_first"])
        assert bool((val["g_rows"][1] == 0).all()) and not bool((inp["index"] == 1).any())  # image 1 is empty
    else:
        assert val["g_rows"] is None and val["g_first"] is None
    for name in ("g_x", "g_in"):
        assert bool((trm[name] >= val[name].abs() * (1 - 1e-12)).all())
    # the masks are those of the ys GIVEN: flip one entry of ys[0] and the statement follows it, whatever a forward would say
    ys2 = [y.clone() for y in ys]
    col = int((ys2[0][5] > 0).nonzero()[0])
    ys2[0][5, col] = 0.0
    val2, _ = R.chain_backward(g, inp, ys2)
    assert not torch.equal(val2["g_in"], val["g_in"])


def test_inputs_hold_their_special_values_and_the_mask_rule_is_threshold_backward():
    for m, k in [(m, 256) for m in R.GEMM256_ROWS] + [(m, k) for k in R.GEMM_OTHER_K for m in R.GEMM_OTHER_ROWS]:
        x = R.make_gemm_inputs(m, k)["x"]
        assert R.has_the_special_values(x), (m, k)
        want = torch.ops.aten.threshold_backward(torch.ones_like(x), x, 0) != 0
        assert torch.equal(want, x > 0) and torch.equal(want, x.view(torch.int32) > 0)  # strictly positive; on the bits: a denormal counts
        assert want[0, 2] and want[m - 1, 132] and not want[0, 0] and not want[0, 1] and not want[0, 3] and not want[m - 1, 131]
        assert 0.3 < float((x == 0).float().mean()) < 0.7
    a = R.with_nonfinite_rows(R.make_gemm_inputs(33, 256)["a"])
    assert bool(torch.isinf(a[11]).any()) and bool(torch.isnan(a[32]).any()) and int((~torch.isfinite(a)).sum()) == 2
    for layout, c in (("one image, 129 rows", 260), ("boundaries on block edges", 1028), ("mostly empty images", 17)):
        s = R.make_seg_inputs(layout, c)
        y = s["y"]
        assert y[0].view(torch.int32)[1] == -(1 << 31) and 0 < float(y[0, 2]) < 1e-38 and float(y[-1, 3]) == -1.5 and not bool(torch.isnan(y).any())
        assert c < 135 or float(y[-1, 133]) == -1.5
    counts = {k: torch.bincount(R.make_seg_inputs(k, 1)["img"], minlength=v[1]).tolist() for k, v in R.SEG_LAYOUTS.items()}
    assert counts["boundaries on block edges"] == [128, 128, 128] and counts["boundaries beside block edges"] == [127, 130, 127]
    assert counts["mostly empty images"] == [0, 60, 0, 0, 40, 0] and counts["one row per image"] == [1] * 300 and counts["empty list"] == [0, 0]
    for n in (4, 8, 10):
        x, _ = R.make_embed_inputs(n, 257)
        bits, f = x.view(torch.int32), R.embed_freq(n)
        assert x.shape == (257, 3) and bool((bits == 0).any()) and bool((bits == -(1 << 31)).any()) and bool((x[:, 0] < 0).any())
        assert bool(((x.abs() > 0) & (x.abs() < 1e-38)).any()) and bool((x == 1e4).any()) and bool((x == -1e4).any())
        assert abs(float(x[5, 1]) * float(f[n - 1]) - math.pi) < 1e-6 and R.make_embed_inputs(n, 7)[0].shape == (7, 3)
        xn, _ = R.make_embed_inputs(n, 7, nonfinite=True)
        assert xn.shape == (9, 3) and bool(torch.isinf(xn[7]).any()) and bool(torch.isnan(xn[8]).any()) and bool(torch.isfinite(xn[:7]).all())
    assert R.m_wrap(256) == 65569 and list(R.second_sweep_rows(256, 65569)) == list(range(65536, 65569))


def _cpu_embed_floor():
    hostnets = importlib.import_module("3danimals_amd.hostnets")
    return R.embed_floor("cpu", lambda n: hostnets.HarmonicEmbedding(n, R.EMBED_SCALAR))


def test_noise_floor_of_the_float32_evaluation():
    floor = dict(R.noise_floor())
    print({k: round(v, 4) for k, v in floor.items()})
    efloor = _cpu_embed_floor()
    print("embedding, with the CPU's libm (the GPU test takes the GPU's):", {k: round(v, 4) for k, v in efloor.items()})
    rows = dict(gemm256=R.GEMM256_ROWS, gemm_k=R.GEMM_OTHER_ROWS, **{q: R.CHAIN_ROWS for q in R.CHAIN_QUANTITIES})
    seg_rows = {R.make_seg_inputs(k, 1)["g"].shape[0] for k in R.SEG_LAYOUTS}
    want = {(q, m) for q, ms in rows.items() for m in ms} | {(q, p) for q in ("segsum", "masked_segsum", "add_relu") for p in seg_rows}
    assert set(floor) == want
    exact = {("segsum", 0), ("masked_segsum", 0), ("add_relu", 0), ("segsum", 1), ("masked_segsum", 1), ("segsum", 300), ("masked_segsum", 300)}  # sums of one term, or of none
    for key, v in floor.items():
        # a float32 evaluation is off by a fraction of eps32 (sum |terms| + |value|) per rounding and, with at most 4112 terms, by far less than their count
        assert math.isfinite(v) and v < 64.0 and ((v == 0.0) if key in exact else v > 0.01), (key, v)
    for key, v in efloor.items():
        assert math.isfinite(v) and 0.0 < v < 64.0, (key, v)
    assert set(efloor) == {(q, p) for q in ("embed_fwd", "embed_bwd") for p in R.EMBED_ROWS}
    assert math.isfinite(R.gemm_floor(256, 4099)) and 0.5 < R.gemm_floor(256, 4099) < 4.0  # (float32 products summed one k at a time reach 2.2 there)


# ------------------------------------------------------------------------------------------------------------------ planted errors
def _rejected(check, bar, *args, **kw):
    """The GPU test's own helper, given a wrong result: it fails a pattern check, or exceeds the bar by at least 10x."""
    try:
        v = check(*args, bar=float("inf"), **kw)
    except R.PatternError:
        return "pattern"
    assert not v <= 10 * bar, (v, bar)
    with pytest.raises(AssertionError):
        check(*args, bar=bar, **kw)
    return v


def test_the_helpers_accept_the_float32_cpu_results_and_reject_planted_errors():
    floor = R.noise_floor()
    seen = {}
    # ---- GEMM, K = 256, M = 33: one full tile and a ragged one of one row
    inp = R.make_gemm_inputs(33, 256)
    a, b, x = inp["a"], inp["b"], inp["x"]
    bar = R.MARGIN * floor["gemm256", 33]
    good = R.gemm_float32_cpu(a, b, x)
    R.check_gemm(good, inp, True, bar)
    R.check_gemm(R.gemm_float32_cpu(a, b), inp, False, bar)
    x_up = x.clone()
    x_up[32] = x[31]
    seen["mask of the ragged tile from the row above"] = _rejected(R.check_gemm, bar, R.gemm_float32_cpu(a, b, x_up), inp, True)
    short = torch.ops.aten.threshold_backward(a[:, :-32].mm(b[:-32]), x, 0)
    seen["last 32 of K dropped"] = _rejected(R.check_gemm, bar, short, inp, True)
    seen["last 32 of K dropped, plain"] = _rejected(R.check_gemm, bar, a[:, :-32].mm(b[:-32]), inp, False)
    seen["denormal masked out"] = _rejected(R.check_gemm, bar, a.mm(b) * (x > 1e-38), inp, True)
    assert int(((x > 0) != (x > 1e-38)).sum()) == 4  # the four denormals alone
    stale = good.clone()
    stale[17] = R.gemm_float32_cpu(*[R.make_gemm_inputs(33, 256, seed=1)[k] for k in "abx"])[17]  # what an earlier call left in the buffer
    seen["one output row left stale"] = _rejected(R.check_gemm, bar, stale, inp, True)
    stale_plain = a.mm(b)
    stale_plain[32] = 0.0
    seen["last row never stored, plain"] = _rejected(R.check_gemm, bar, stale_plain, inp, False)
    neg_zero = good.clone()
    neg_zero[0, 0] = -0.0
    assert _rejected(R.check_gemm, bar, neg_zero, inp, True) == "pattern"
    # ---- segment sums: three images with boundaries beside the 128-row block edges
    s = R.make_seg_inputs("boundaries beside block edges", 64)
    p = s["g"].shape[0]
    bar = R.MARGIN * floor["segsum", p]
    sums = lambda img, g=s["g"]: torch.zeros(s["b"], 64).index_add_(0, img, g)
    R.check_segsum(sums(s["img"]), s, bar)
    moved = s["img"].clone()
    moved[127] = 0  # the first row of image 1 (the last row of block 0) summed into image 0
    seen["boundary row summed into the neighbouring image"] = _rejected(R.check_segsum, bar, sums(moved), s)
    twice = sums(s["img"])
    twice[1] += s["g"][128:256].sum(0)  # block 1 (rows 128..255, all image 1) added twice
    seen["one block's partial sum added twice"] = _rejected(R.check_segsum, bar, twice, s)
    e = R.make_seg_inputs("mostly empty images", 64)
    leak = torch.zeros(6, 64).index_add_(0, e["img"], e["g"])
    R.check_segsum(leak, e, R.MARGIN * floor["segsum", 100])
    leak[2, 5] = -0.0
    assert _rejected(R.check_segsum, bar, leak, e) == "pattern"
    bar = R.MARGIN * floor["masked_segsum", p]
    g_pre = torch.ops.aten.threshold_backward(s["g"], s["y"], 0)
    R.check_masked_segsum(g_pre, sums(s["img"], g_pre), s, bar)
    g_den = s["g"] * (s["y"] > 1e-38)
    assert _rejected(R.check_masked_segsum, bar, g_den, sums(s["img"], g_den), s) == "pattern"
    seen["masked sum, boundary row moved"] = _rejected(R.check_masked_segsum, bar, g_pre, sums(moved, g_pre), s)
    # ---- embedding (the bar from the CPU's float32 torch expression here)
    efloor = _cpu_embed_floor()
    hostnets = importlib.import_module("3danimals_amd.hostnets")
    n, symmetrize, ones = 10, True, True
    x, gen = R.make_embed_inputs(n, 257)
    w = R.embed_weights(x, n, ones, gen)
    f = R.embed_freq(n)
    out, g_x = R.embed_float32(x, hostnets.HarmonicEmbedding(n, R.EMBED_SCALAR), symmetrize, ones, w)
    bar_f, bar_b = R.MARGIN * efloor["embed_fwd", 257], R.MARGIN * efloor["embed_bwd", 257]
    R.check_embed_fwd(out, x, f, symmetrize, ones, bar_f)
    R.check_embed_bwd(g_x, w, x, f, symmetrize, ones, bar_b)
    swapped = out.clone()
    c, k = 1, 3
    swapped[:, 3 + c * n + k], swapped[:, 3 + 3 * n + c * n + k] = out[:, 3 + 3 * n + c * n + k], out[:, 3 + c * n + k]
    seen["sin and cos columns of one (c, k) swapped"] = _rejected(R.check_embed_fwd, bar_f, swapped, x, f, symmetrize, ones)
    f_off = torch.cat((f[1:], f[-1:] * 2))
    shifted = R.embed_ref(x, f_off, symmetrize, ones).float()  # every (c, k) evaluated with f_(k+1)
    seen["frequency index off by one"] = _rejected(R.check_embed_fwd, bar_f, shifted, x, f, symmetrize, ones)
    unsigned = g_x.clone()
    unsigned[:, 0] = g_x[:, 0] * torch.sign(x[:, 0])  # undo the sign: what remains is the derivative with respect to |x_0|
    seen["sign of d|x_0|/dx_0 dropped"] = _rejected(R.check_embed_bwd, bar_b, unsigned, w, x, f, symmetrize, ones)
    raw_copy = out.clone()
    raw_copy[:, 0] = x[:, 0]
    assert _rejected(R.check_embed_fwd, bar_f, raw_copy, x, f, symmetrize, ones) == "pattern"
    print({k: (v if isinstance(v, str) else f"{v:.3g}") for k, v in seen.items()})
    assert len(seen) >= 9
