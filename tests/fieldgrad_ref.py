"""Float64 statements of the scalar field's value, input gradient and the adjoint of that gradient (hostnets._FieldValue / _FieldInputGrad,
3danimals_amd/csrc/fieldgrad.h), of the embedding's tangent (csrc/embed.hip, he_jvp_kernel) and of the head kernels (csrc/fieldhead.hip), with the
seeded inputs tests/test_fieldgrad_gpu.py runs them on and the float32 CPU evaluations its bars come from.

    value      y_0 = relu(e W_in^T), y_l = relu(y_(l-1) W_l^T), out = y_L w_h^T                    D_l := (y_l > 0)
    gradient   b_L = (s w_h) * D_L, b_(l-1) = (b_l W_l) * D_(l-1), v = b_0 W_in, g_x = J_e(x)^T v
               first order: dW_l = b_l^T y_(l-1), dw_h = s^T y_L, dW_in = b_0^T e
    adjoint    dv = J_e(x) lam, dW_in = b_0^T dv, t_0 = (dv W_in^T) * D_0, t_l = (t_(l-1) W_l^T) * D_l, dW_l = b_l^T t_(l-1),
               dw_h = sum_m s[m] t_L[m,:], ds = t_L w_h^T

e = [x (|x_0|), sin(x_c f_k), cos(x_c f_k), 1], (c, k) c-major; W_in [256, 4 + 6n] carries the in_layer's bias as its last column.  Every
function takes the masks D_l as arguments: a float64 forward flips the mask of an entry at rounding distance from 0, and that would compare
two different piecewise-linear functions.  ``angle32``: the angles are float64(fl32(x_c f_k)), as the kernels round them (fieldnet_ref);
without it everything is float64, which is what torch's own double backward in float64 computes.

Statistic and bars are tests/fieldnet_ref.py's: |got - ref64| / (eps32 (sum |terms| + |ref64|)), at most 4 x what the float32 CPU
evaluation of the same inputs reaches."""
import functools
import math

import torch

import fieldnet_ref as F

N = 256
MARGIN = F.MARGIN
GEMM_ROWS = (1, 31, 33, 129, 1000)
GEMM_K = (52, 64, 256)  # the in_layer's K for 8 and 10 frequencies, a hidden layer's
JVP_N = (4, 8, 10)
CHAIN_ROWS = (33, 1000)
CHAIN_LAYERS = (1, 4)


# ------------------------------------------------------------------------------------------------------------------ embedding
def _angles(x, freq, symmetrize, angle32):
    xs = x.clone()
    if symmetrize:
        xs[:, 0] = xs[:, 0].abs()
    if angle32:
        ang = (xs.float()[:, :, None] * freq.float()).double()
    else:
        ang = xs.double()[:, :, None] * freq.double()
    sgn = torch.ones_like(x, dtype=torch.float64)
    if symmetrize:
        sgn[:, 0] = torch.sign(x[:, 0].double())  # 0 at +-0, as torch.abs has it
    return xs.double(), ang, sgn  # ang [M,3,n]


def embed(x, freq, symmetrize, angle32=False):
    xs, ang, _ = _angles(x, freq, symmetrize, angle32)
    m = x.shape[0]
    return torch.cat([xs, ang.sin().reshape(m, -1), ang.cos().reshape(m, -1), torch.ones(m, 1, dtype=torch.float64)], -1)


def embed_vjp(v, x, freq, symmetrize, angle32=False):
    """J_e(x)^T v and the sum of |terms| (fieldnet_ref.embed_grad_ref with the ones column)."""
    n = freq.shape[0]
    _, ang, sgn = _angles(x, freq, symmetrize, angle32)
    v, f = v.double(), freq.double()
    vs, vc = v[:, 3:3 + 3 * n].reshape(-1, 3, n), v[:, 3 + 3 * n:3 + 6 * n].reshape(-1, 3, n)
    g = v[:, :3] + (f * (vs * ang.cos() - vc * ang.sin())).sum(-1)
    terms = v[:, :3].abs() + (f * ((vs * ang.cos()).abs() + (vc * ang.sin()).abs())).sum(-1)
    return g * sgn, terms


def embed_jvp(lam, x, freq, symmetrize, angle32=False):
    """J_e(x) lam [M, 4 + 6n]; every entry is one product (the ones column's is 0)."""
    m = x.shape[0]
    _, ang, sgn = _angles(x, freq, symmetrize, angle32)
    l, f = lam.double() * sgn, freq.double()
    return torch.cat([l, (l[:, :, None] * f * ang.cos()).reshape(m, -1), (-l[:, :, None] * f * ang.sin()).reshape(m, -1),
                      torch.zeros(m, 1, dtype=torch.float64)], -1)


# ------------------------------------------------------------------------------------------------------------------ the three blocks
def value(e, w_in, hidden, w_h):
    """[y_0 .. y_L], out -- in the dtype of ``e``."""
    c = lambda t: t.to(e.dtype)
    ys = [torch.relu(e @ c(w_in).t())]
    for w in hidden:
        ys.append(torch.relu(ys[-1] @ c(w).t()))
    return ys, ys[-1] @ c(w_h).t()


def masks_of(ys):
    return [y > 0 for y in ys]


def gradient(s, e, ys, masks, w_in, hidden, w_h, dtype=torch.float64):
    """-> dict(b=[b_0 .. b_L], v, g_in, g_head, g_hidden) and the same over absolute values (the sums of |terms|); ys and masks as GIVEN."""
    c = lambda t: t.to(dtype)
    z = torch.zeros((), dtype=dtype)
    L = len(hidden)
    b, ba = [None] * (L + 1), [None] * (L + 1)
    b[L] = torch.where(masks[L], c(s) * c(w_h), z)
    ba[L] = b[L].abs()
    for l in range(L, 0, -1):
        b[l - 1] = torch.where(masks[l - 1], b[l] @ c(hidden[l - 1]), z)
        ba[l - 1] = torch.where(masks[l - 1], ba[l] @ c(hidden[l - 1]).abs(), z)
    val = dict(b=b, v=b[0] @ c(w_in), g_in=b[0].t() @ c(e), g_head=c(s).t() @ c(ys[L]), g_hidden=[b[l + 1].t() @ c(ys[l]) for l in range(L)])
    trm = dict(b=ba, v=ba[0] @ c(w_in).abs(), g_in=ba[0].t() @ c(e).abs(), g_head=c(s).abs().t() @ c(ys[L]).abs(),
               g_hidden=[ba[l + 1].t() @ c(ys[l]).abs() for l in range(L)])
    return val, trm


def adjoint(dv, s, b, masks, w_in, hidden, w_h, dtype=torch.float64):
    """-> dict(t=[t_0 .. t_L], g_in, g_hidden, g_head, g_s) and the sums of |terms|; b as GIVEN (the gradient pass's chain)."""
    c = lambda t: t.to(dtype)
    z = torch.zeros((), dtype=dtype)
    L = len(hidden)
    dv = c(dv)
    t = [torch.where(masks[0], dv @ c(w_in).t(), z)]
    ta = [torch.where(masks[0], dv.abs() @ c(w_in).abs().t(), z)]
    for l in range(1, L + 1):
        t.append(torch.where(masks[l], t[-1] @ c(hidden[l - 1]).t(), z))
        ta.append(torch.where(masks[l], ta[-1] @ c(hidden[l - 1]).abs().t(), z))
    b = [c(x) for x in b]
    val = dict(t=t, g_in=b[0].t() @ dv, g_hidden=[b[l + 1].t() @ t[l] for l in range(L)], g_head=c(s).t() @ t[L], g_s=t[L] @ c(w_h).t())
    trm = dict(t=ta, g_in=b[0].abs().t() @ dv.abs(), g_hidden=[b[l + 1].abs().t() @ ta[l] for l in range(L)], g_head=c(s).abs().t() @ ta[L],
               g_s=ta[L] @ c(w_h).abs().t())
    return val, trm


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_net(n_hidden, n_freq, seed=0, dtype=torch.float32):
    """He-initialised weights of the standard field: w_in [256, 4 + 6n] (bias column last), n_hidden x [256,256], w_h [1,256]."""
    gen = torch.Generator().manual_seed(977 * n_hidden + 31 * n_freq + seed)
    he = lambda o, i: (torch.randn(o, i, generator=gen) * math.sqrt(2.0 / i)).to(dtype)
    return dict(w_in=he(N, 4 + 6 * n_freq), hidden=[he(N, N) for _ in range(n_hidden)], w_h=he(1, N), freq=F.embed_freq(n_freq))


def make_points(m, seed=0):
    """x [M,3] in (-3.5, 3.5) with x_0 = 0 in the first row and -0.0 in the last, s [M,1] and lam [M,3]."""
    gen = torch.Generator().manual_seed(7919 * m + seed)
    x = torch.rand(m, 3, generator=gen) * 7 - 3.5
    x[0, 0] = 0.0
    x[m - 1, 0] = -0.0 if m > 1 else 0.0
    return x, torch.randn(m, 1, generator=gen), torch.randn(m, 3, generator=gen)


def make_nt_inputs(m, k, seed=0):
    """a [M,K] randn, w [256,K] randn * 0.05 without a zero, x = relu(randn) with fieldnet_ref's special values."""
    gen = torch.Generator().manual_seed(100003 * k + 7 * m + 11 + seed)
    a = torch.randn(m, k, generator=gen)
    w = torch.randn(N, k, generator=gen) * 0.05
    assert bool((w != 0).all())
    return dict(a=a, w=w, b=w.t().contiguous(), x=F.put_special_values(torch.relu(torch.randn(m, N, generator=gen))))


def make_head_inputs(m, seed=0):
    gen = torch.Generator().manual_seed(104729 * m + seed)
    s = torch.randn(m, 1, generator=gen)
    w = torch.randn(1, N, generator=gen) * 0.1
    assert bool((w != 0).all()) and bool((s != 0).all())
    y = F.put_special_values(torch.relu(torch.randn(m, N, generator=gen)))
    return dict(s=s, w=w, y=y, t=torch.randn(m, N, generator=gen))


def head_fwd_ref(inp):
    """(s w) * (y > 0): one product per entry, so the float32 result is the correctly rounded one."""
    return torch.where(inp["y"] > 0, inp["s"].double() * inp["w"].double(), torch.zeros((), dtype=torch.float64))


def head_bwd_ref(inp):
    s, t, w = inp["s"].double(), inp["t"].double(), inp["w"].double()
    return (s.t() @ t, s.abs().t() @ t.abs()), (t @ w.t(), t.abs() @ w.abs().t())


# ------------------------------------------------------------------------------------------------------------------ noise floors
@functools.lru_cache(maxsize=None)
def nt_floor(m):
    """The statistic of torch's float32 CPU mm (+ threshold_backward) over every K, on the inputs of M rows."""
    v = 0.0
    for k in GEMM_K:
        inp = make_nt_inputs(m, k)
        for x in (None, inp["x"]):
            v = max(v, F.statistic(F.gemm_float32_cpu(inp["a"], inp["b"], x), *F.gemm_ref(inp["a"], inp["b"], x)))
    return v


@functools.lru_cache(maxsize=None)
def head_floor(m):
    inp = make_head_inputs(m)
    (gw, gwt), (gs, gst) = head_bwd_ref(inp)
    return dict(g_w=F.statistic(inp["s"].t().mm(inp["t"]), gw, gwt), g_s=F.statistic(inp["t"].mm(inp["w"].t()), gs, gst))


TN_CASES = ((1, 1, 256), (31, 1, 52), (33, 4, 256), (129, 2, 64), (1000, 4, 256), (1000, 1, 52), (10000, 4, 256))  # (M, batch, C)


def make_tn_inputs(m, batch, c, seed=0):
    gen = torch.Generator().manual_seed(15485863 * batch + 611 * c + m + seed)
    return torch.randn(batch, m, N, generator=gen), torch.randn(batch, m, c, generator=gen)


def tn_ref(p, q):
    return p.double().transpose(1, 2) @ q.double(), p.double().abs().transpose(1, 2) @ q.double().abs()


@functools.lru_cache(maxsize=None)
def tn_floor(m):
    """The statistic of torch's float32 CPU bmm over the cases of M rows."""
    v = 0.0
    for mm, batch, c in TN_CASES:
        if mm == m:
            p, q = make_tn_inputs(mm, batch, c)
            v = max(v, F.statistic(torch.bmm(p.transpose(1, 2), q), *tn_ref(p, q)))
    return v


def _worst(values):
    return max(values, key=lambda v: float("inf") if v != v else v)


def chain_statistics(got, ref, terms):
    """{quantity: statistic} over the keys of ``got`` (lists: the largest over the layers)."""
    res = {}
    for name, g in got.items():
        if isinstance(g, (list, tuple)):
            res[name] = _worst([F.statistic(a.cpu(), r, t) for a, r, t in zip(g, ref[name], terms[name])])
        else:
            res[name] = F.statistic(g.cpu(), ref[name], terms[name])
    return res


@functools.lru_cache(maxsize=None)
def chain_floor(m, n_hidden, n_freq=8, symmetrize=True):
    """{quantity: statistic} of the plain float32 CPU evaluation of the whole chain (forward, the three blocks with mm / threshold-style
    selects) against float64 with the float32 run's own masks, intermediates handed on in float32 as on the GPU."""
    net, (x, s, lam) = make_net(n_hidden, n_freq), make_points(m)
    return chain_float32_statistics(net, x, s, lam, symmetrize)


def chain_float32_statistics(net, x, s, lam, symmetrize, device="cpu"):
    """The float32 formulation on ``device`` against the float64 blocks, quantity by quantity."""
    f32 = torch.float32
    freq = net["freq"]
    to = lambda t: t.to(device)
    e64 = embed(x, freq, symmetrize, angle32=True)
    e = to(e64.float())
    w_in, hidden, w_h = to(net["w_in"]), [to(w) for w in net["hidden"]], to(net["w_h"])
    ys, out = value(e, w_in, hidden, w_h)
    ys_c = [y.cpu() for y in ys]
    masks = masks_of(ys_c)
    masks_d = [m.to(device) for m in masks]
    gval, _ = gradient(to(s), e, ys, masks_d, w_in, hidden, w_h, dtype=f32)
    g_x = embed_vjp(gval["v"].cpu(), x, freq, symmetrize, angle32=True)[0].float()
    dv = embed_jvp(lam, x, freq, symmetrize, angle32=True).float()
    aval, _ = adjoint(to(dv), to(s), gval["b"], masks_d, w_in, hidden, w_h, dtype=f32)
    got = dict(g_x=g_x, g_in=gval["g_in"], g_head=gval["g_head"], g_hidden=gval["g_hidden"], a_in=aval["g_in"], a_hidden=aval["g_hidden"],
               a_head=aval["g_head"], a_s=aval["g_s"])
    res = chain_reference_statistics(got, x, s, lam, net, ys_c, [b.cpu() for b in gval["b"]], gval["v"].cpu(), dv, symmetrize)
    res.update(forward_statistics(ys_c, out.cpu(), x, net, symmetrize))
    return res


def forward_statistics(ys, out, x, net, symmetrize):
    """{y, out}: a run's activations and values against the float64 forward from the same points (the condition under which the masks of the
    run may stand in for the float64 ones: entries at rounding distance from 0 apart, the two forwards agree).  An activation's terms are
    the products behind it back to the embedding: the forward over absolute values."""
    e64 = embed(x, net["freq"], symmetrize, angle32=True)
    ys64, out64 = value(e64, net["w_in"], net["hidden"], net["w_h"])
    ya, _ = value(e64.abs(), net["w_in"].abs(), [w.abs() for w in net["hidden"]], net["w_h"].abs())
    return dict(y=_worst([F.statistic(y, r, t) for y, r, t in zip(ys, ys64, ya)]), out=F.statistic(out, out64, ya[-1] @ net["w_h"].double().abs().t()))


def chain_reference_statistics(got, x, s, lam, net, ys, b, v, dv, symmetrize):
    """The statistics of one run's results against the float64 blocks evaluated from the inputs with that run's masks (ys: the run's
    activations).  An entry's terms are all the products behind it, back to s and lam: the chains over absolute values.
    ``got``: g_x, g_in, g_head, g_hidden (gradient pass) and a_in, a_hidden, a_head, a_s (adjoint); b, v, dv: the run's intermediates."""
    freq = net["freq"]
    masks = masks_of(ys)
    e64 = embed(x, freq, symmetrize, angle32=True)
    gval, gtrm = gradient(s, e64, ys, masks, net["w_in"], net["hidden"], net["w_h"])
    gx_ref = embed_vjp(gval["v"], x, freq, symmetrize, angle32=True)[0]
    gx_terms = embed_vjp_abs(gtrm["v"], x, freq, symmetrize)  # the embedding's adjoint over the chain's absolute sums
    aval, atrm = adjoint(embed_jvp(lam, x, freq, symmetrize, angle32=True), s, gval["b"], masks, net["w_in"], net["hidden"], net["w_h"])
    ref = dict(g_x=gx_ref, g_in=gval["g_in"], g_head=gval["g_head"], g_hidden=gval["g_hidden"], a_in=aval["g_in"], a_hidden=aval["g_hidden"],
               a_head=aval["g_head"], a_s=aval["g_s"], b=gval["b"], v=gval["v"], dv=embed_jvp(lam, x, freq, symmetrize, angle32=True))
    # the adjoint's weight-gradient products contract b with t: their terms carry both chains' absolute sums
    L = len(net["hidden"])
    trm = dict(g_x=gx_terms, g_in=gtrm["g_in"], g_head=gtrm["g_head"], g_hidden=gtrm["g_hidden"],
               a_in=gtrm["b"][0].t() @ ref["dv"].abs(), a_hidden=[gtrm["b"][l + 1].t() @ atrm["t"][l] for l in range(L)], a_head=atrm["g_head"],
               a_s=atrm["g_s"], b=gtrm["b"], v=gtrm["v"], dv=None)
    res = chain_statistics({k: got[k] for k in got}, ref, trm)
    res["b"] = _worst([F.statistic(a, r, t) for a, r, t in zip(b, ref["b"], trm["b"])])
    if v is not None:
        res["v"] = F.statistic(v, ref["v"], trm["v"])
    if dv is not None:
        res["dv"] = F.statistic(dv, ref["dv"], ref["dv"].abs())
    return res


def embed_vjp_abs(va, x, freq, symmetrize):
    """sum of |terms| of J_e^T v for a v given by its own sums of |terms| va >= 0."""
    n = freq.shape[0]
    _, ang, _ = _angles(x, freq, symmetrize, True)
    f = freq.double()
    vs, vc = va[:, 3:3 + 3 * n].reshape(-1, 3, n), va[:, 3 + 3 * n:3 + 6 * n].reshape(-1, 3, n)
    return va[:, :3] + (f * (vs * ang.cos().abs() + vc * ang.sin().abs())).sum(-1)
