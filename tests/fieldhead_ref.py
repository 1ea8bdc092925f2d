"""Float64 statements of the two entry points of include/a3d_fields.h, the inputs tests/test_fieldhead_gpu.py runs them on, the error
statistic both test files use and its noise floor: what a plain float32 evaluation on the CPU reaches on those same inputs."""
import functools
import itertools

import torch
import torch.nn.functional as F

EPS32 = float(torch.finfo(torch.float32).eps)
WG_ROWS = 512  # A3D_FIELD_HEAD_WG_ROWS (tests/test_fieldhead_cpu.py compares it with the header)
ROWS = (1, 31, 33, 257, 2 * WG_ROWS + 1, 4099)
CHANNELS = (1, 3, 9, 16)
MODES = tuple(itertools.product((0, 1), (False, True)))  # (act, with min_max)
QUANTITIES = ("s", "out", "g_h", "g_w")
DENORMAL = 1e-40
MARGIN = 4.0  # a different summation order may cost this much over the float32 CPU evaluation


def head_fwd_ref(h, w, lo, scale, act):
    """-> (s, out) in float64."""
    s = h.double() @ w.double().t()
    if act:
        s = torch.sigmoid(s)
    out = s if scale is None else s * scale.double() + lo.double()
    return s, out


def head_adjoint_ref(g_out, s, scale, act):
    ga = g_out.double() if scale is None else g_out.double() * scale.double()
    return ga * (s.double() * (1 - s.double())) if act else ga


def head_bwd_ref(g_out, s, h, w, scale, act):
    """-> (g_h, g_w) in float64; the mask is h > 0, strictly."""
    ga = head_adjoint_ref(g_out, s, scale, act)
    return (ga @ w.double()) * (h > 0), ga.t() @ h.double()


def make_inputs(m, c, with_map, seed=0):
    """float32 CPU tensors.  h is a ReLU output with exact zeros plus, in the first and the last row, a -0.0, a positive denormal and a
    negative value (which a ReLU never leaves, and which the mask must still treat as threshold_backward does)."""
    g = torch.Generator().manual_seed(1000 * m + 10 * c + seed)
    h = torch.relu(torch.randn(m, 256, generator=g))
    for row, col in ((0, 0), (m - 1, 130)):
        h[row, col:col + 5] = torch.tensor([0.0, -0.0, DENORMAL, -1.5, 0.0])
    w = torch.randn(c, 256, generator=g) * 0.1
    g_out = torch.randn(m, c, generator=g)
    lo = scale = None
    if with_map:
        lo = torch.randn(c, generator=g)
        scale = torch.rand(c, generator=g) + 0.5
    return dict(h=h, w=w, g_out=g_out, lo=lo, scale=scale)


def has_the_special_values(h):
    bits = h.view(torch.int32)
    return bool((bits == 0).any() and (bits == -(1 << 31)).any() and ((h > 0) & (h < 1e-38)).any() and (h < 0).any())


def statistics(got, inp, act):
    """max over the entries of |x - ref64| / (eps32 (sum_k |term_k| + |ref64|)) for s, out, g_h and g_w of ``got`` (a dict; a missing or
    None entry is skipped); term_k are the summands of the dot product behind the entry."""
    h, w, g_out, lo, scale = (inp[k] for k in ("h", "w", "g_out", "lo", "scale"))
    s, out = head_fwd_ref(h, w, lo, scale, act)
    g_h, g_w = head_bwd_ref(g_out, s, h, w, scale, act)
    ga = head_adjoint_ref(g_out, s, scale, act).abs()
    fwd_terms = h.double().abs() @ w.double().abs().t()
    terms = dict(s=fwd_terms, out=fwd_terms, g_h=ga @ w.double().abs(), g_w=ga.t() @ h.double().abs())
    ref = dict(s=s, out=out, g_h=g_h, g_w=g_w)
    res = {}
    for name in QUANTITIES:
        x = got.get(name)
        if x is not None:
            assert x.shape == ref[name].shape and x.dtype == torch.float32, (name, x.shape, x.dtype)
            err = (x.double().cpu() - ref[name]).abs()  # (an entry all of whose terms are zero must be exact: 0 / 0 counts as 0, e / 0 as inf)
            res[name] = float(torch.where(err == 0, err, err / (EPS32 * (terms[name] + ref[name].abs()))).max())
    return res


def float32_cpu(inp, act):
    """linear -> sigmoid -> affine and its autograd in float32 on the CPU, the ReLU adjoint by threshold_backward."""
    h = inp["h"].clone().requires_grad_(True)
    w = inp["w"].clone().requires_grad_(True)
    s = F.linear(h, w)
    if act:
        s = torch.sigmoid(s)
    out = s if inp["scale"] is None else s * inp["scale"] + inp["lo"]
    g_h, g_w = torch.autograd.grad(out, (h, w), inp["g_out"])
    return dict(s=s.detach(), out=out.detach(), g_h=torch.ops.aten.threshold_backward(g_h, inp["h"], 0), g_w=g_w)


@functools.lru_cache(maxsize=None)
def noise_floor():
    """(quantity, rows) -> the largest statistic of the float32 CPU evaluation over the inputs of the GPU test with that many rows.
    One figure per row count and not one per case: the statistic is a maximum over the entries, and over the single entry of the
    one-row, one-channel case it is a draw that says nothing about the tail of its distribution (it can be 0).  With one row every
    g_w entry is a single product, and the one with the denormal h is itself denormal: its rounding error, a fraction of 2^-149, is
    thousands of eps32 of it -- for the CPU and for any other correctly rounded float32 evaluation alike."""
    floor = {}
    for m, c, (act, with_map) in itertools.product(ROWS, CHANNELS, MODES):
        inp = make_inputs(m, c, with_map)
        for name, v in statistics(float32_cpu(inp, act), inp, act).items():
            floor[name, m] = max(floor.get((name, m), 0.0), v)
    return floor
