"""Float64 statements of what csrc/gemm.hip, csrc/segsum.hip and csrc/embed.hip compute and of the chain hostnets._stack_backward builds
from them, the seeded inputs tests/test_fieldnet_gpu.py runs them on, the error statistic both test files use, its noise floor (what a
plain float32 evaluation of the same inputs reaches) and the assertion helpers the GPU test applies to the kernels' results and the CPU
test applies to wrong results planted on purpose.

The statistic is tests/fieldhead_ref.py's, per quantity: max over the entries of |got - ref64| / (eps32 (sum |terms| + |ref64|)), the terms
being the summands behind the entry; 0 / 0 counts as 0.  The embedding's forward values lie in [-1, 1] and are divided by eps32 alone.

The mask rule is threshold_backward's: strictly > 0, on the float32 the kernel sees, so -0.0 is masked and a positive denormal is not.
No input below puts a NaN into a mask operand X or y: threshold_backward(g, NaN) passes g through (its test is `x <= 0 ? 0 : g`) while the
kernels' `x > 0 ? g : 0` gives 0, and no caller relies on either."""
import functools
import itertools
import math

import torch

EPS32 = float(torch.finfo(torch.float32).eps)
MARGIN = 4.0  # a different summation order may cost this much over the plain float32 evaluation (as in fieldhead_ref)
DENORMAL = 1e-40
SPECIAL = (0.0, -0.0, DENORMAL, -1.5, 0.0)  # at columns 0..4 and 130..134 of the first and the last row of a mask operand
SPECIAL_COLS = (0, 130)
N = 256

GEMM256_ROWS = (1, 31, 32, 33, 63, 257, 4099)  # K = 256: the persistent kernel, 32-row tiles
GEMM_OTHER_K = (32, 64, 288, 512)  # the block-tiled kernel, 128-row tiles; one chunk, two, a ninth that re-reads mask byte 0, sixteen
GEMM_OTHER_ROWS = (1, 33, 127, 128, 129, 257)
SEG_CHANNELS = (1, 3, 17, 52, 64, 256, 260, 1028)  # scalar path with CP = 1, 4, 32, 64; vector path with CP = 16, 64, 128 (> CV = 65), 256 (< CV = 257)
EMBED_CONFIGS = ((10, True, True), (8, False, True), (4, True, False), (10, False, False))  # (n, symmetrize, ones)
EMBED_ROWS = (1, 7, 257)
EMBED_SCALAR = 2 * math.pi / 7 * 0.9
CHAIN_ROWS = (16, 48, 4112)  # multiples of hostnets.SPLITK_PARTS; one tile of either GEMM, a ragged one, 129 tiles
CHAIN_CASES = tuple(itertools.product((1, 3), (False, True)))  # (hidden layers, with the per-image layer)
CHAIN_IMAGES = 3  # image 1 is empty
CHAIN_QUANTITIES = ("g_x", "g_in", "g_rows", "g_first", "g_hidden")


class PatternError(AssertionError):
    """A result that is wrong on its bits -- a zero pattern, a copied column -- whatever its size."""


def m_wrap(n_cu):
    """The first M at which a wave of gm_nn3_kernel (n_cu // 2 work-groups per column half, 16 waves each) takes a second 32-row tile, with
    that sweep's second tile ragged: one full sweep, one full tile, one row."""
    return 32 * 16 * (n_cu // 2) + 33


def second_sweep_rows(n_cu, m):
    return range(min(m, 32 * 16 * (n_cu // 2)), m)


# ------------------------------------------------------------------------------------------------------------------ the statistic
def statistic(got, ref, terms=None):
    """max |got - ref| / (eps32 (terms + |ref|)); ``terms`` None: / eps32.  An exact entry counts as 0 whatever its denominator; a NaN or
    an infinity in ``got`` where ``ref`` is finite makes the result NaN or inf, which no bar admits."""
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32 and ref.dtype == torch.float64, (got.shape, ref.shape, got.dtype)
    if ref.numel() == 0:
        return 0.0
    err = (got.double().cpu() - ref).abs()
    den = EPS32 if terms is None else EPS32 * (terms + ref.abs())
    r = torch.where(err == 0, err, err / den)
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def within(value, bar, what):
    assert value <= bar, f"{what}: statistic {value:.4g} above the bar {bar:.4g}"  # (a NaN fails too)
    return value


# ------------------------------------------------------------------------------------------------------------------ GEMM
def gemm_ref(a, b, x=None):
    """(A . B) * (X > 0) in float64 (a masked entry is 0 whatever the product is, an infinity or a NaN included) and the sum of |terms|."""
    prod = a.double() @ b.double()
    terms = a.double().abs() @ b.double().abs()
    if x is not None:
        prod = torch.where(x > 0, prod, torch.zeros_like(prod))
    return prod, terms


def put_special_values(t):
    """SPECIAL into the first and the last row of a [M,256] mask operand, in both 128-column halves."""
    for row in {0, t.shape[0] - 1}:
        for col in SPECIAL_COLS:
            t[row, col:col + len(SPECIAL)] = torch.tensor(SPECIAL)
    return t


def has_the_special_values(t):
    bits = t.view(torch.int32)
    ok = True
    for row in (0, t.shape[0] - 1):
        for col in SPECIAL_COLS:
            ok = ok and bits[row, col] == 0 and bits[row, col + 1] == -(1 << 31) and 0 < float(t[row, col + 2]) < 1e-38 and float(t[row, col + 3]) == -1.5
    return bool(ok)


def make_gemm_inputs(m, k, seed=0):
    """float32 CPU tensors: A randn, B randn * 0.05 without a zero, X = relu(randn) (half exact zeros) with the special values."""
    g = torch.Generator().manual_seed(100003 * k + 7 * m + seed)
    a = torch.randn(m, k, generator=g)
    b = torch.randn(k, N, generator=g) * 0.05
    assert bool((b != 0).all())
    x = put_special_values(torch.relu(torch.randn(m, N, generator=g)))
    return dict(a=a, b=b, x=x)


def nonfinite_rows(m):
    """(row of the +inf, row of the NaN or None): the NaN sits in the last row -- inside a ragged last tile, and the row the kernels'
    clamped loads repeat for the rows past M."""
    return m // 3, (m - 1 if m > 1 else None)


def with_nonfinite_rows(a):
    a = a.clone()
    r_inf, r_nan = nonfinite_rows(a.shape[0])
    a[r_inf, 3] = float("inf")
    if r_nan is not None:
        a[r_nan, a.shape[1] - 2] = float("nan")
    return a


def gemm_float32_cpu(a, b, x=None):
    c = a.mm(b)
    return c if x is None else torch.ops.aten.threshold_backward(c, x, 0)


def check_mask_bits(got, x, what):
    """C != 0 exactly where X > 0, and +0.0 on the bits elsewhere (no product of these inputs is zero or underflows: B has no zero and A is
    randn, so an unmasked entry is a sum of 32 or more products of size 1e-2)."""
    got, passes = got.cpu(), (x > 0)
    if not torch.equal(got != 0, passes):
        bad = (got != 0) != passes
        rows = sorted(set(bad.nonzero()[:, 0].tolist()))
        raise PatternError(f"{what}: zero pattern differs from X > 0 at {int(bad.sum())} entries, rows {rows[:8]}{'...' if len(rows) > 8 else ''}")
    if not bool((got.view(torch.int32)[~passes] == 0).all()):
        raise PatternError(f"{what}: a masked entry is not +0.0 on the bits")


def check_gemm(got, inp, masked, bar, what="gemm", rows_named=None):
    """-> the statistic, after the mask's bit pattern (PatternError) and the bar (AssertionError)."""
    x = inp["x"] if masked else None
    if masked:
        check_mask_bits(got, x, what)
    ref, terms = gemm_ref(inp["a"], inp["b"], x)
    v = statistic(got, ref, terms)
    if not v <= bar and rows_named is not None:
        per_row = torch.tensor([statistic(got[r:r + 1], ref[r:r + 1], terms[r:r + 1]) for r in rows_named])
        what += f" [rows {rows_named[0]}..{rows_named[-1]}: largest statistic {float(per_row.nan_to_num(float('inf')).max()):.4g} at row {rows_named[int(per_row.nan_to_num(float('inf')).argmax())]}]"
    return within(v, bar, what)


# ------------------------------------------------------------------------------------------------------------------ segment sums
def segsum_ref(g, img, b):
    """out[i] = sum of the rows p with img[p] == i, in float64, and the sums of |g|."""
    out = torch.zeros(b, g.shape[1], dtype=torch.float64).index_add_(0, img, g.double())
    terms = torch.zeros(b, g.shape[1], dtype=torch.float64).index_add_(0, img, g.double().abs())
    return out, terms


def masked_segsum_ref(g, y, img, b):
    """a3d_rows_add_relu_bwd: g_pre = g * (y > 0) (exact: bitwise threshold_backward(g, y, 0) where y is no NaN) and its segment sums."""
    g_pre = torch.where(y > 0, g.double(), torch.zeros_like(g, dtype=torch.float64))
    return (g_pre,) + segsum_ref(g_pre, img, b)


def rows_add_relu_ref(y, rows, img):
    """relu(y + rows[img]) in float64, and |y| + |rows[img]|."""
    return torch.relu(y.double() + rows.double()[img]), y.double().abs() + rows.double()[img].abs()


def _runs(counts):
    return torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))


SEG_LAYOUTS = {  # name -> (img as a list of per-image row counts, B)
    "one image, 1 row": ((1,), 1),
    "one image, 127 rows": ((127,), 1),
    "one image, 128 rows": ((128,), 1),
    "one image, 129 rows": ((129,), 1),
    "one image, 513 rows": ((513,), 1),
    "boundaries on block edges": ((128, 128, 128), 3),
    "boundaries beside block edges": ((127, 130, 127), 3),  # edges at 127 and 257
    "one row per image": ((1,) * 300, 300),
    "mostly empty images": ((0, 60, 0, 0, 40, 0), 6),  # only images 1 and 4, inside one block
    "padded tail": ((90, 0, 110 + 56), 3),  # the render path's list: 200 points, then 56 padding rows that repeat the last image
    "empty list": ((0, 0), 2),
}


def make_seg_inputs(layout, c, seed=0):
    """float32 g, y (the special values in its first and last row, as far as C reaches), rows, and the sorted int64 img."""
    counts, b = SEG_LAYOUTS[layout]
    img = _runs(counts)
    p = int(img.shape[0])
    gen = torch.Generator().manual_seed(1009 * c + 13 * p + b + seed)
    g = torch.randn(p, c, generator=gen)
    y = torch.randn(p, c, generator=gen)
    if p:
        for row in {0, p - 1}:
            for col in SPECIAL_COLS:
                n = max(0, min(len(SPECIAL), c - col))
                y[row, col:col + n] = torch.tensor(SPECIAL[:n])
    rows = torch.randn(b, c, generator=gen)
    assert bool((img[1:] >= img[:-1]).all())
    return dict(g=g, y=y, rows=rows, img=img, b=b)


def is_sorted_index(img):
    return bool((img[1:] >= img[:-1]).all())


def check_segsum(got, inp, bar, what="segsum", g=None):
    ref, terms = segsum_ref(inp["g"] if g is None else g, inp["img"], inp["b"])
    present = torch.zeros(inp["b"], dtype=torch.bool).index_fill_(0, inp["img"], True)
    if not bool((got.cpu()[~present].view(torch.int32) == 0).all()):
        raise PatternError(f"{what}: the row of an image without points is not +0.0")
    return within(statistic(got, ref, terms), bar, what)


def check_masked_segsum(g_pre, g_rows, inp, bar, what="masked segsum"):
    want = torch.ops.aten.threshold_backward(inp["g"], inp["y"], 0)
    if not torch.equal(g_pre.cpu().view(torch.int32), want.view(torch.int32)):
        raise PatternError(f"{what}: g_pre is not threshold_backward(g, y, 0) on the bits")
    return check_segsum(g_rows, inp, bar, what, g=want)


# ------------------------------------------------------------------------------------------------------------------ embedding
def embed_freq(n):
    return EMBED_SCALAR * (2.0 ** torch.arange(n))  # hostnets.HarmonicEmbedding(n, EMBED_SCALAR).frequencies, float32


def _embed_angles(x, freq, symmetrize):
    xs = x.clone()
    if symmetrize:
        xs[:, 0] = xs[:, 0].abs()
    ang32 = (xs[:, :, None] * freq).reshape(x.shape[0], -1)  # the float32 product is part of the definition: the kernel rounds it too
    return xs, ang32.double()


def embed_ref(x, freq, symmetrize, ones):
    """[x (|x_0|), sin(a), cos(a), (1)] with a = float64(fl32(x_c f_k)), (c, k) c-major."""
    xs, ang = _embed_angles(x, freq, symmetrize)
    parts = [xs.double(), ang.sin(), ang.cos()] + ([torch.ones(x.shape[0], 1, dtype=torch.float64)] if ones else [])
    return torch.cat(parts, -1)


def embed_grad_ref(g, x, freq, symmetrize, ones):
    """d sum(g * embed(x)) / dx in float64 (the derivative of a is f_k, that of |x_0| is sign(x_0): 0 at +-0 as torch.abs has it), and the
    sum of |terms|."""
    n = freq.shape[0]
    _, ang = _embed_angles(x, freq, symmetrize)
    g, f = g.double(), freq.double()
    gs, gc = g[:, 3:3 + 3 * n].reshape(-1, 3, n), g[:, 3 + 3 * n:3 + 6 * n].reshape(-1, 3, n)
    sn, cs = ang.sin().reshape(-1, 3, n), ang.cos().reshape(-1, 3, n)
    g_x = g[:, :3] + (f * (gs * cs - gc * sn)).sum(-1)
    terms = g[:, :3].abs() + (f * ((gs * cs).abs() + (gc * sn).abs())).sum(-1)
    if symmetrize:
        g_x[:, 0] = g_x[:, 0] * torch.sign(x[:, 0].double())
    return g_x, terms


def make_embed_inputs(n, p, nonfinite=False, seed=0):
    """x [P,3] float32 and the weights g of the output columns.  The seven special rows hold 0.0, -0.0 and +-1e-40 (an x_0 of +-0 included),
    negative x_0, +-1e4 and pi / f_k rounded to float32 (where sin crosses 0 and cos is -1); P = 7 is those rows, P = 257 has them first and
    again last around uniform(-3.5, 3.5) rows, P = 1 is one row with a negative denormal x_0, -1e4 and pi / f_(n-1).  ``nonfinite`` appends
    a row with an infinity and a row with a NaN (forward only)."""
    f = embed_freq(n)
    pi_over = lambda k: float((torch.tensor(math.pi, dtype=torch.float64) / f[k].double()).float())
    special = torch.tensor([[0.0, -0.0, DENORMAL], [-0.0, -DENORMAL, 0.0], [-0.7, 0.3, -1.2], [1e4, -1e4, 0.5], [-1e4, 1e4, -1e4],
                            [pi_over(0), pi_over(n - 1), pi_over(n // 2)], [-pi_over(1), -pi_over(n - 1), pi_over(0)]])
    gen = torch.Generator().manual_seed(101 * n + p + seed)
    if p == 1:
        x = torch.tensor([[-DENORMAL, -1e4, pi_over(n - 1)]])
    elif p == 7:
        x = special
    else:
        x = torch.cat((special, torch.rand(p - 14, 3, generator=gen) * 7 - 3.5, special.flip(0)))
    if nonfinite:
        x = torch.cat((x, torch.tensor([[0.3, float("inf"), -0.2], [float("nan"), 0.1, 0.2]])))
    return x.contiguous(), gen


def embed_weights(x, n, ones, gen):
    return torch.rand(x.shape[0], 3 + 6 * n + int(ones), generator=gen) * 2 - 1


def embed_float32(x, emb, symmetrize, ones, w=None):
    """The torch expression of the existing parity test (HarmonicEmbedding + abs / cat), in float32 on x's device -> (out, g_x or None)."""
    xb = x.clone().requires_grad_(w is not None)
    xs = torch.cat([xb[..., :1].abs(), xb[..., 1:]], -1) if symmetrize else xb
    out = torch.cat([xs, emb(xs)] + ([torch.ones(x.shape[0], 1, device=x.device)] if ones else []), -1)
    g_x = torch.autograd.grad((out * w).sum(), xb)[0] if w is not None else None
    return out.detach(), g_x


def check_embed_fwd(got, x, freq, symmetrize, ones, bar, what="embed fwd"):
    """x must be finite.  The copied columns and the ones column are exact; sin and cos are within the bar of float64."""
    n = freq.shape[0]
    ref = embed_ref(x, freq, symmetrize, ones)
    got = got.cpu()
    if not torch.equal(got[:, :3].view(torch.int32), ref[:, :3].float().view(torch.int32)) or (ones and not bool((got[:, -1] == 1).all())):
        raise PatternError(f"{what}: the copied x columns or the ones column differ")
    return within(statistic(got[:, 3:3 + 6 * n].contiguous(), ref[:, 3:3 + 6 * n].contiguous()), bar, what)


def check_embed_bwd(got, g, x, freq, symmetrize, ones, bar, what="embed bwd"):
    ref, terms = embed_grad_ref(g, x, freq, symmetrize, ones)
    got = got.cpu()
    if symmetrize and not bool((got[:, 0][x[:, 0] == 0] == 0).all()):
        raise PatternError(f"{what}: the gradient at x_0 = +-0 under symmetrize is not 0")
    return within(statistic(got, ref, terms), bar, what)


# ------------------------------------------------------------------------------------------------------------------ the stack's backward chain
def make_chain_inputs(m, n_hidden, with_feat, seed=0):
    """float32: x_emb [M,64] (the n = 10 embedding with the ones column), w_in [256,64], per_image [3,256] / index (images 0 and 2 only) /
    w_first [256,256] or None, n_hidden weights [256,256], and g_out [M,256], the gradient of ys[-1] BEFORE that layer's ReLU adjoint."""
    gen = torch.Generator().manual_seed(31 * m + 5 * n_hidden + int(with_feat) + seed)
    x_emb = embed_ref(torch.rand(m, 3, generator=gen) * 2 - 1, embed_freq(10), True, True).float()
    he = lambda o, i: torch.randn(o, i, generator=gen) * math.sqrt(2.0 / i)
    inp = dict(x_emb=x_emb, w_in=he(N, 64), per_image=None, index=None, w_first=None, n_images=0)
    if with_feat:
        inp.update(per_image=torch.randn(CHAIN_IMAGES, N, generator=gen) * 0.5, w_first=he(N, N), n_images=CHAIN_IMAGES,
                   index=_runs((m // 3, 0, m - m // 3)))
    inp["hidden"] = [he(N, N) for _ in range(n_hidden)]
    inp["g_out"] = torch.randn(m, N, generator=gen)
    return inp


def chain_forward(inp, dtype=torch.float32):
    """[y0, (y1,) .. y_n] of hostnets._stack_forward, plainly, in ``dtype`` on the CPU."""
    c = lambda t: t.to(dtype)
    ys = [torch.relu(c(inp["x_emb"]) @ c(inp["w_in"]).t())]
    if inp["w_first"] is not None:
        ys.append(torch.relu(ys[0] @ c(inp["w_first"]).t() + c(inp["per_image"])[inp["index"]]))
    for w in inp["hidden"]:
        ys.append(torch.relu(ys[-1] @ c(w).t()))
    return ys


def chain_backward(g, inp, ys, dtype=torch.float64):
    """hostnets._stack_backward, statement by statement, in ``dtype``: g is the gradient of ys[-1] with that layer's ReLU adjoint applied;
    every mask is ys[i] > 0 of the ys GIVEN (what the GPU saw), not of a forward of this function's own.  -> (values, sums of |terms|),
    dicts over CHAIN_QUANTITIES (g_hidden: lists)."""
    c = lambda t: t.to(dtype)
    ys = [c(y) for y in ys]
    n_hidden = len(inp["hidden"])
    g = c(g)
    ga = g.abs()  # the same chain over absolute values: an entry's terms are all the products behind it, back to g (what bounds the
    # rounding of the float32 intermediates the chain hands from layer to layer, for the kernels and for the CPU alike)
    val, trm = dict(g_rows=None, g_first=None, g_hidden=[]), dict(g_rows=None, g_first=None, g_hidden=[])

    def step(g, ga, w, y_prev):
        keep = y_prev > 0
        z = torch.zeros((), dtype=dtype)
        return torch.where(keep, g @ c(w), z), torch.where(keep, ga @ c(w).abs(), z)

    for i in range(n_hidden - 1, -1, -1):
        y_prev = ys[len(ys) - n_hidden - 1 + i]
        val["g_hidden"].insert(0, g.t() @ y_prev)
        trm["g_hidden"].insert(0, ga.t() @ y_prev.abs())
        g, ga = step(g, ga, inp["hidden"][i], y_prev)
    if inp["w_first"] is not None:
        b = inp["n_images"]
        val["g_rows"] = torch.zeros(b, N, dtype=dtype).index_add_(0, inp["index"], g)
        trm["g_rows"] = torch.zeros(b, N, dtype=dtype).index_add_(0, inp["index"], ga)
        val["g_first"], trm["g_first"] = g.t() @ ys[0], ga.t() @ ys[0].abs()
        g, ga = step(g, ga, inp["w_first"], ys[0])
    val["g_in"], trm["g_in"] = g.t() @ c(inp["x_emb"]), ga.t() @ c(inp["x_emb"]).abs()
    val["g_x"], trm["g_x"] = g @ c(inp["w_in"]), ga @ c(inp["w_in"]).abs()
    return val, trm


def chain_statistics(got, g, inp, ys):
    """got: dict over CHAIN_QUANTITIES of float32 results (g_hidden a list; None entries skipped) -> {quantity: statistic}."""
    ref, terms = chain_backward(g, inp, ys)
    res = {}
    for name in CHAIN_QUANTITIES:
        if got.get(name) is None:
            assert ref[name] is None
            continue
        if name == "g_hidden":
            assert len(got[name]) == len(ref[name])
            res[name] = max([statistic(a, r, t) for a, r, t in zip(got[name], ref[name], terms[name])], key=lambda v: float("inf") if v != v else v)
        else:
            res[name] = statistic(got[name], ref[name], terms[name])
    return res


def chain_float32_cpu(inp):
    """(g, ys, results) of a plain float32 evaluation on the CPU: forward, threshold_backward, mm, index_add_."""
    ys = chain_forward(inp)
    g = torch.ops.aten.threshold_backward(inp["g_out"], ys[-1], 0)
    n_hidden = len(inp["hidden"])
    out = dict(g_rows=None, g_first=None, g_hidden=[])
    gg = g
    for i in range(n_hidden - 1, -1, -1):
        y_prev = ys[len(ys) - n_hidden - 1 + i]
        out["g_hidden"].insert(0, gg.t().mm(y_prev))
        gg = torch.ops.aten.threshold_backward(gg.mm(inp["hidden"][i]), y_prev, 0)
    if inp["w_first"] is not None:
        out["g_rows"] = torch.zeros(inp["n_images"], N).index_add_(0, inp["index"], gg)
        out["g_first"] = gg.t().mm(ys[0])
        gg = torch.ops.aten.threshold_backward(gg.mm(inp["w_first"]), ys[0], 0)
    out["g_in"] = gg.t().mm(inp["x_emb"])
    out["g_x"] = gg.mm(inp["w_in"])
    return g, ys, out


# ------------------------------------------------------------------------------------------------------------------ the noise floor
@functools.lru_cache(maxsize=None)
def gemm_floor(k, m):
    """The statistic of torch's float32 CPU mm (+ threshold_backward) on the inputs of (M, K), the larger of plain and masked."""
    inp = make_gemm_inputs(m, k)
    v = statistic(gemm_float32_cpu(inp["a"], inp["b"]), *gemm_ref(inp["a"], inp["b"]))
    if k >= 256:
        v = max(v, statistic(gemm_float32_cpu(inp["a"], inp["b"], inp["x"]), *gemm_ref(inp["a"], inp["b"], inp["x"])))
    return v


@functools.lru_cache(maxsize=None)
def noise_floor():
    """(quantity, rows) -> the largest statistic of the plain float32 CPU evaluation (mm + threshold_backward, index_add_, relu, the chain
    of them) over the GPU test's inputs with that many rows.  One figure per row count and not one per case, as in fieldhead_ref: the
    statistic is a maximum over entries, and over the few entries of a narrow case it is a draw, not a tail.  Quantities: gemm256,
    gemm_k (the other K together), segsum, masked_segsum, add_relu, and CHAIN_QUANTITIES."""
    floor = {}

    def note(name, rows, v):
        floor[name, rows] = max(floor.get((name, rows), 0.0), v)

    for m in GEMM256_ROWS:
        note("gemm256", m, gemm_floor(256, m))
    for k, m in itertools.product(GEMM_OTHER_K, GEMM_OTHER_ROWS):
        note("gemm_k", m, gemm_floor(k, m))
    for layout, c in itertools.product(SEG_LAYOUTS, SEG_CHANNELS):
        inp = make_seg_inputs(layout, c)
        p, b = inp["g"].shape[0], inp["b"]
        note("segsum", p, statistic(torch.zeros(b, c).index_add_(0, inp["img"], inp["g"]), *segsum_ref(inp["g"], inp["img"], b)))
        g_pre = torch.ops.aten.threshold_backward(inp["g"], inp["y"], 0)
        note("masked_segsum", p, statistic(torch.zeros(b, c).index_add_(0, inp["img"], g_pre), *segsum_ref(g_pre, inp["img"], b)))
        note("add_relu", p, statistic(torch.relu(inp["y"] + inp["rows"][inp["img"]]), *rows_add_relu_ref(inp["y"], inp["rows"], inp["img"])))
    for m, (n_hidden, with_feat) in itertools.product(CHAIN_ROWS, CHAIN_CASES):
        inp = make_chain_inputs(m, n_hidden, with_feat)
        g, ys, out = chain_float32_cpu(inp)
        for name, v in chain_statistics(out, g, inp, ys).items():
            note(name, m, v)
    return floor


def embed_floor(device, emb_of):
    """(quantity, rows) -> the statistic of the float32 torch expression evaluated on ``device`` (the GPU test: the same device as the kernel,
    so the device's libm is on both sides) over every configuration; ``emb_of(n)`` builds the HarmonicEmbedding."""
    floor = {}
    for (n, symmetrize, ones), p in itertools.product(EMBED_CONFIGS, EMBED_ROWS):
        x, gen = make_embed_inputs(n, p)
        w = embed_weights(x, n, ones, gen)
        out, g_x = embed_float32(x.to(device), emb_of(n), symmetrize, ones, w.to(device))
        f = embed_freq(n)
        ref = embed_ref(x, f, symmetrize, ones)
        floor["embed_fwd", p] = max(floor.get(("embed_fwd", p), 0.0), statistic(out.cpu()[:, 3:3 + 6 * n].contiguous(), ref[:, 3:3 + 6 * n].contiguous()))
        floor["embed_bwd", p] = max(floor.get(("embed_bwd", p), 0.0), statistic(g_x.cpu(), *embed_grad_ref(w, x, f, symmetrize, ones)))
    return floor
