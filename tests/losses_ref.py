"""Float64 restatement of the reconstruction and flow losses (csrc/losses.hip; compute_reconstruction_losses, background mode 'none'),
written from their definition.  N = B x F frames of H x W pixels, m = the alpha channel of ``shaded``:

    mask        = sum((m valid - mask_gt)^2) / HW
    mask_inv_dt = sum((1 - m) dt0) / HW                      mask_dt = sum(m dt1) / HW   (0 without dt1)
    q           = [m valid > 0] mask_gt                       (no gradient)
    both        = [box3x3(q) / 9 > 0.99]                      the 3 x 3 sum takes zeros outside the frame
    rgb         = sum(|rgb - image_gt| both) / (3 HW)         d|x|/dx = sign(x), sign(0) = 0
    dino        = sum((feat - feat_gt)^2 both) / (D HW)
    flow[b,f]   = sum((flow - flow_gt)^2 both[b,f]) / max(2 count(both[b,f]), 1),  f < F - 1; 0 if |flow_gt| > 0.5 anywhere on both[b,f]

Plain torch, no import from the package; every function takes a dtype: float64 is the reference, float32 the yardstick.  Gradients come
from autograd of  sum(loss * w_loss) + sum(flow * w_flow).

The four discrete decisions -- m valid > 0, box / 9 > 0.99, |flow_gt| > 0.5, sign(rgb - image_gt) -- belong to the definition and must
come out the same in every precision: ``check_knife_edges`` (called by ``build``) refuses a case in which a rounding could move one.

Beside each value stands its MAGNITUDE (as in tests/skin_ref.py): for a loss the same expression with every summand replaced by its
absolute value, for a gradient element the sum of the absolute values of its terms (three for alpha: mask, mask_inv_dt, mask_dt -- the
first with |m valid| + |mask_gt| for its inner difference, see ``alpha_terms``; one for everything else).  Errors are measured in units of 2^-24 x magnitude.  MEASURED holds, per case and quantity, what the float32
evaluation of this restatement reaches against the float64 one (tests/test_losses_cpu.py measures it afresh and compares); a kernel's
bound is 4 x that figure in these units plus 4 ulp of the float64 value, and nothing else.
"""
import numpy as np
import torch
import torch.nn.functional as F

from deriv_ref import EPS, units, violations  # noqa: F401  (the same unit and the same bound as the derivative suite)

F64 = torch.float64
FACTOR = 4.0
KEYS = ("loss", "g_rgb", "g_alpha", "g_feat", "flow", "g_flow")
WRONG = ("no_pad", "flow_count", "large_whole_frame", "rgb_hw", "pair_frame", "sign0")  # the deliberately wrong pieces of test_losses_cpu
NORMAL_MIN = 2.0 ** -126
TINY = 2.0 ** -102  # 2^-126 / 2^-24: an alpha gradient below the float32 normal range (alpha = 2^-126 is a case value) may lose its last bits
HALF_UP = float(np.nextafter(np.float32(0.5), np.float32(1.0)))


# ---------------------------------------------------------------------------------------------------------------- restatement
def box_sums(alpha, valid, mask_gt, pad_zero=True):
    """[N,H,W] sums of q = [alpha valid > 0] mask_gt over the 3 x 3 neighbourhood (dtype of ``mask_gt``), zeros outside the frame."""
    q = (alpha * valid > 0).to(mask_gt.dtype) * mask_gt
    H, W = q.shape[1:]
    qp = F.pad(q, (1, 1, 1, 1)) if pad_zero else F.pad(q[:, None], (1, 1, 1, 1), mode="replicate")[:, 0]
    s = torch.zeros_like(q)
    for dy in range(3):
        for dx in range(3):
            s = s + qp[:, dy:dy + H, dx:dx + W]
    return s


def eroded_mask(alpha, valid, mask_gt, pad_zero=True):
    """bool [N,H,W]"""
    return box_sums(alpha.detach(), valid, mask_gt, pad_zero) / 9 > 0.99


def recon_losses(c, shaded, feat, dtype=F64, wrong=None, mag=False):
    """-> (loss [N,5] = (mask, mask_inv_dt, rgb, dino, mask_dt), both bool [N,H,W]).  ``mag``: every summand by its absolute value."""
    t = lambda k: c[k].to(dtype)
    H, W, D = c["H"], c["W"], c["D"]
    HW = H * W
    a = (lambda x: x.abs()) if mag else (lambda x: x)
    m, valid, mask_gt, dt = shaded[..., 3], t("valid"), t("mask_gt"), t("mask_dt")
    total = lambda x: x.flatten(1).sum(1)
    both = eroded_mask(m, valid, mask_gt, pad_zero=wrong != "no_pad")
    bf = both.to(dtype)[..., None]
    diff = shaded[..., :3] - t("image_gt").permute(0, 2, 3, 1)
    absd = torch.where(diff >= 0, diff, -diff) if wrong == "sign0" else diff.abs()  # (where: the derivative at 0 is +1)
    cols = [total((m * valid - mask_gt) ** 2) / HW, total(a((1 - m) * dt[:, 0])) / HW, total(absd * bf) / (HW if wrong == "rgb_hw" else 3 * HW)]
    cols.append(total((feat - t("feat_gt").permute(0, 2, 3, 1)) ** 2 * bf) / (D * HW) if D else torch.zeros_like(cols[0]))
    cols.append(total(a(m * dt[:, 1])) / HW if c["dt1"] else torch.zeros_like(cols[0]))
    return torch.stack(cols, 1), both


def flow_losses(c, flow, both, dtype=F64, wrong=None):
    """flow [N,H,W,2], both bool [N,H,W] -> (loss [B,F-1], dropped bool [B,F-1]).  Every summand is a square: its own magnitude."""
    B, Fr, H, W = c["B"], c["F"], c["H"], c["W"]
    P = B * (Fr - 1)
    if wrong == "pair_frame":  # pair number p reads frame p
        pred, bm = flow[:P].view(B, Fr - 1, H, W, 2), both[:P].view(B, Fr - 1, H, W)
    else:
        pred, bm = flow.view(B, Fr, H, W, 2)[:, :-1], both.view(B, Fr, H, W)[:, :-1]
    gt = c["flow_gt"].to(dtype).permute(0, 1, 3, 4, 2)
    big = gt.abs() > 0.5
    dropped = (big if wrong == "large_whole_frame" else big & bm[..., None]).flatten(2).any(2)
    count = bm.flatten(2).sum(2).to(dtype)
    den = (count if wrong == "flow_count" else 2 * count).clamp_min(1)
    err = ((pred - gt) ** 2 * bm[..., None].to(dtype)).flatten(2).sum(2)
    return err * (~dropped).to(dtype) / den, dropped


def evaluate(c, dtype=F64, wrong=None):
    """Everything case ``c`` produces, evaluated in ``dtype``: loss [N,5], mask uint8 [N,H,W], g_rgb [N,H,W,3], g_alpha [N,H,W],
    g_feat [N,H,W,D] (D > 0), and with F > 1: flow [B,F-1], dropped bool [B,F-1], g_flow [N,H,W,2]."""
    shaded = c["shaded"].to(dtype).requires_grad_(True)
    feat = c["feat"].to(dtype).requires_grad_(True) if c["D"] else None
    loss, both = recon_losses(c, shaded, feat, dtype, wrong)
    total = (loss * c["w_loss"].to(dtype)).sum()
    leaves = [shaded] + ([feat] if c["D"] else [])
    res = dict(loss=loss.detach(), mask=both.to(torch.uint8))
    if c["F"] > 1:
        flow = c["flow"].to(dtype).requires_grad_(True)
        fl, dropped = flow_losses(c, flow, both, dtype, wrong)
        total = total + (fl * c["w_flow"].to(dtype)).sum()
        leaves.append(flow)
        res.update(flow=fl.detach(), dropped=dropped)
    g = torch.autograd.grad(total, leaves)
    res.update(g_rgb=g[0][..., :3], g_alpha=g[0][..., 3])
    if c["D"]:
        res["g_feat"] = g[1]
    if c["F"] > 1:
        res["g_flow"] = g[-1]
    return res


def alpha_terms(c, mag=False):
    """The three terms of the alpha gradient, float64 [3,N,H,W]: mask, mask_inv_dt, mask_dt.  ``mag``: their magnitudes -- absolute
    values, and |m valid| + |mask_gt| for the difference inside the first (a rounding of m valid moves the term by that much however
    small the difference is: the subtraction becomes an addition, as in tests/deriv_ref.py)."""
    t = lambda k: c[k].double()
    HW = c["H"] * c["W"]
    m, valid, w = t("shaded")[..., 3], t("valid"), t("w_loss")[:, :, None, None] / HW
    t3 = w[:, 4] * t("mask_dt")[:, 1] if c["dt1"] else torch.zeros_like(m)
    if mag:
        return torch.stack([w[:, 0].abs() * 2 * ((m * valid).abs() + t("mask_gt").abs()) * valid.abs(), (w[:, 1] * t("mask_dt")[:, 0]).abs(), t3.abs()])
    return torch.stack([w[:, 0] * 2 * (m * valid - t("mask_gt")) * valid, -w[:, 1] * t("mask_dt")[:, 0], t3])


def reference(c):
    """key -> (float64 value, magnitude) over keys_of(c), plus 'mask' (uint8) and 'dropped' (bool) as plain tensors."""
    ev = evaluate(c)
    with torch.no_grad():
        lmag = recon_losses(c, c["shaded"].double(), c["feat"].double() if c["D"] else None, mag=True)[0]
    res = dict(mask=ev["mask"], loss=(ev["loss"], lmag), g_rgb=(ev["g_rgb"], ev["g_rgb"].abs()), g_alpha=(ev["g_alpha"], alpha_terms(c, mag=True).sum(0) + TINY))
    if c["D"]:
        res["g_feat"] = (ev["g_feat"], ev["g_feat"].abs())
    if c["F"] > 1:
        res.update(dropped=ev["dropped"], flow=(ev["flow"], ev["flow"].abs()), g_flow=(ev["g_flow"], ev["g_flow"].abs()))
    return res


def keys_of(c):
    """The float quantities a case is compared on."""
    return tuple(k for k in KEYS if (k != "g_feat" or c["D"]) and (k not in ("flow", "g_flow") or c["F"] > 1))


def figure(name, key):
    """What the float32 evaluation reaches on quantity ``key`` of case ``name`` (units of 2^-24 x magnitude)."""
    return MEASURED[name][key]


def allowed_units(name, key):
    return FACTOR * figure(name, key)


def bad_elements(got, ref, mag, name, key):
    """Indices where |got - ref| > 2^-24 (4 x figure(name, key) x magnitude + 4 |ref|); non-finite values violate."""
    return violations(got, ref, mag, figure(name, key), factor=FACTOR, floor_ulp=4.0)


# ---------------------------------------------------------------------------------------------------------------- knife edges
def check_knife_edges(c):
    """Asserts, in float64, that no discrete decision of case ``c`` can be moved by a rounding."""
    alpha, valid = c["shaded"][..., 3].double(), c["valid"].double()
    for x in (alpha, valid):
        assert bool(((x == 0) | (x.abs() >= NORMAL_MIN)).all()), "a denormal input"
    tiny = (alpha != 0) & (alpha.abs() < 0.2)
    assert bool(((valid[tiny] == 0) | (valid[tiny] == 1)).all()), "a fractional valid beside a tiny alpha"
    prod = alpha * valid
    assert bool(((prod == 0) | (prod.abs() >= NORMAL_MIN)).all()) and bool((prod.float().double() == prod)[tiny | (alpha == 0)].all()), \
        "alpha * valid is not exact where it decides"
    s = box_sums(alpha, valid, c["mask_gt"].double())
    assert bool(((s == s.round()) | ((s - 8.91).abs() >= 1e-3)).all()), "a 3 x 3 sum within 1e-3 of 0.99 x 9"
    if c["F"] > 1:
        g = c["flow_gt"].double().abs()
        assert bool(((g <= 0.45) | (g == 0.5) | (g == HALF_UP) | (g >= 0.6)).all()), "a |flow_gt| near 0.5 that is neither 0.5 nor the next float"
    return c


# ---------------------------------------------------------------------------------------------------------------- cases
# name -> dict(B, F, H, W, D, layout, alpha, mask, rgb, dt1, up, pairs, fstride[, hole]).  N = B x F frames; F = 1: no flow.
#   layout  contig | wide17 (the first 16 channels of a 17-channel image) | offset1 (contiguous, one float into its storage: misaligned)
#   alpha   render (0 / 1 / soft >= 0.2, a solid patch of ones) | special (render + {0, -0.0, -0.25, 2^-126, 1, 1.5} at 40% of the
#           pixels) | positive ({2^-126, 1, 1.5, soft}, valid = 1: the mask is mask_gt's alone)
#   mask    binary | ones | 0.98 | 0.995 | hole (ones and one zero per frame at ``hole`` [(y, x), ...], cycled over the frames)
#   rgb     random | ties (one channel equal to the target bit for bit, the others one ulp above / below) | wide (1e-3 .. 1e3)
#   up      random (normal weights, zeros and negative ones among them) | sum (loss.sum()) | cols4 (column 4 unused)
#   pairs   flow specials cycled over the B (F - 1) pairs: plain | empty | one | half | over0 | over1 | offmask
def _c(B, Fr, H, W, D, layout="contig", alpha="render", mask="binary", rgb="random", dt1=True, up="random", pairs=("plain",), fstride=2, **kw):
    return dict(B=B, F=Fr, H=H, W=W, D=D, layout=layout, alpha=alpha, mask=mask, rgb=rgb, dt1=dt1, up=up, pairs=tuple(pairs), fstride=fstride, **kw)


ALL_PAIRS = ("plain", "empty", "one", "half", "over0", "over1", "offmask")
CASES = {
    # ---- frame shapes, each with one frame and with B = 3 sequences of two frames (flow on every shape)
    "hw_1x1_n1": _c(1, 1, 1, 1, 4, alpha="positive", mask="ones"),
    "hw_1x1_b3": _c(3, 2, 1, 1, 5, alpha="special"),
    "hw_1x7_n1": _c(1, 1, 1, 7, 8, alpha="positive", mask="ones", up="sum"),
    "hw_1x7_b3": _c(3, 2, 1, 7, 3, alpha="special", fstride=3),
    "hw_9x1_n1": _c(1, 1, 9, 1, 1, alpha="positive", mask="0.995"),
    "hw_9x1_b3": _c(3, 2, 9, 1, 4, alpha="special", up="cols4"),
    "hw_3x85_n1": _c(1, 1, 3, 85, 12, alpha="positive", mask="hole", hole=[(1, 84)]),
    "hw_3x85_b3": _c(3, 2, 3, 85, 4, pairs=("plain", "half", "over0"), fstride=3),
    "hw_16x16_n1": _c(1, 1, 16, 16, 16, alpha="positive", mask="hole", hole=[(5, 15)], rgb="ties"),
    "hw_16x16_b3": _c(3, 2, 16, 16, 8, pairs=("offmask", "one", "over1")),
    "hw_257x1_n1": _c(1, 1, 257, 1, 5, alpha="positive", mask="ones"),
    "hw_257x1_b3": _c(3, 2, 257, 1, 4, alpha="special", fstride=3),
    "hw_1x257_n1": _c(1, 1, 1, 257, 4, alpha="positive", mask="0.995"),
    "hw_1x257_b3": _c(3, 2, 1, 257, 3, alpha="special"),
    "hw_2x300_n1": _c(1, 1, 2, 300, 8, alpha="positive", mask="hole", hole=[(0, 256)]),
    "hw_2x300_b3": _c(3, 2, 2, 300, 0, alpha="special", up="sum"),
    "hw_4x300_n3": _c(3, 1, 4, 300, 4, alpha="positive", mask="hole", hole=[(1, 212), (2, 255), (1, 299)]),  # (W > 256 with an interior; pixel 512)
    "hw_200x3_n1": _c(1, 1, 200, 3, 20, alpha="positive", mask="hole", hole=[(85, 1)]),
    "hw_200x3_b3": _c(3, 2, 200, 3, 4, pairs=("half", "plain", "empty"), fstride=3),
    "hw_130x130_n1": _c(1, 1, 130, 130, 8, alpha="positive", mask="hole", hole=[(1, 126)]),
    "hw_130x130_b3": _c(3, 2, 130, 130, 4, alpha="special", pairs=("plain", "offmask", "half"), up="cols4"),
    "hw_17x33_n1": _c(1, 1, 17, 33, 16, alpha="special", rgb="ties"),
    "hw_17x33_b3": _c(3, 2, 17, 33, 5, pairs=("over1", "plain", "one"), fstride=3),
    # ---- feature widths on 17 x 33 (three work-groups, the last wave ragged)
    "d_none": _c(3, 1, 17, 33, 0),
    "d1": _c(3, 1, 17, 33, 1, alpha="special"),
    "d3": _c(3, 1, 17, 33, 3, up="sum"),
    "d5": _c(3, 1, 17, 33, 5, rgb="wide"),
    "d4": _c(3, 1, 17, 33, 4, alpha="special"),
    "d8": _c(3, 1, 17, 33, 8, up="cols4"),
    "d12": _c(3, 1, 17, 33, 12),
    "d20": _c(3, 1, 17, 33, 20, alpha="special", up="sum"),
    "d16_contig": _c(3, 1, 17, 33, 16),
    "d16_wide17": _c(3, 1, 17, 33, 16, layout="wide17", alpha="special"),
    "d16_offset1": _c(3, 1, 17, 33, 16, layout="offset1"),
    "d12_offset1": _c(1, 1, 16, 16, 12, layout="offset1", up="sum"),
    "d260": _c(1, 1, 17, 33, 260),
    # ---- targets
    "mask_ones": _c(3, 1, 17, 33, 4, alpha="positive", mask="ones"),
    "mask_098": _c(3, 1, 17, 33, 4, alpha="positive", mask="0.98"),
    "mask_0995": _c(3, 1, 17, 33, 4, alpha="positive", mask="0.995"),
    "mask_hole_group_edge": _c(3, 1, 17, 33, 4, alpha="positive", mask="hole", hole=[(7, 25), (7, 24), (15, 17)]),  # pixels 256, 255, 512
    "mask_hole_row_end": _c(3, 1, 17, 33, 4, alpha="positive", mask="hole", hole=[(8, 32), (8, 0), (0, 0)]),
    "rgb_ties": _c(3, 1, 17, 33, 0, rgb="ties"),
    "rgb_wide": _c(3, 1, 17, 33, 0, rgb="wide", up="sum"),
    "no_dt1": _c(3, 1, 17, 33, 16, alpha="special", dt1=False),
    "no_dt1_sum": _c(1, 1, 16, 16, 5, dt1=False, up="sum"),
    # ---- flow
    "flow_b1_f2": _c(1, 2, 17, 33, 0, pairs=("half",)),
    "flow_b1_f4_stride3": _c(1, 4, 17, 33, 4, pairs=("offmask", "over0", "one"), fstride=3),
    "flow_b3_f2_stride3": _c(3, 2, 17, 33, 0, pairs=("over1", "empty", "offmask"), fstride=3, up="sum"),
    "flow_b3_f4": _c(3, 4, 17, 33, 16, layout="wide17", pairs=ALL_PAIRS + ("plain", "offmask")),
    "flow_b3_f4_sum": _c(3, 4, 16, 16, 0, pairs=("plain", "over0", "plain", "half", "plain", "empty", "over1", "plain", "one"), up="sum"),
}


def _patch(n):
    """The solid patch's extent along an axis of n pixels."""
    lo = n // 4
    return lo, min(n, lo + max(5, n // 2))


def build(name, check=True):
    """The tensors of a case (float32, CPU; feat NHWC, targets NCHW as the dataset holds them) and the spec's fields."""
    s = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 9000)
    B, Fr, H, W, D = s["B"], s["F"], s["H"], s["W"], s["D"]
    N = B * Fr
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    u = lambda *sh: rng.uniform(0.0, 1.0, sh).astype(np.float32)
    (y0, y1), (x0, x1) = _patch(H), _patch(W)
    # alpha and valid
    soft = np.clip(u(N, H, W), 0.2, 1.0)
    if s["alpha"] == "positive":
        alpha = np.choose(rng.integers(0, 4, (N, H, W)), [np.full((N, H, W), NORMAL_MIN, np.float32), np.ones((N, H, W), np.float32),
                                                          np.full((N, H, W), 1.5, np.float32), soft])
        valid = np.ones((N, H, W), np.float32)
    else:
        alpha = (u(N, H, W) > 0.4) * soft
        alpha[:, y0:y1, x0:x1] = 1.0
        if s["alpha"] == "special":
            vals = np.float32([0.0, -0.0, -0.25, NORMAL_MIN, 1.0, 1.5])
            alpha = np.where(u(N, H, W) < 0.4, vals[rng.integers(0, 6, (N, H, W))], alpha)
        valid = (u(N, H, W) > 0.1).astype(np.float32)
        frac = (u(N, H, W) < 0.15) & ((alpha == 0) | (alpha >= 0.2))
        valid = np.where(frac, 0.3 + 0.6 * u(N, H, W), valid)
        valid[:, y0:y1, x0:x1] = np.where(u(N, y1 - y0, x1 - x0) < 0.9, 1.0, valid[:, y0:y1, x0:x1])
    # mask_gt
    if s["mask"] == "binary":
        mask = (u(N, H, W) > 0.3).astype(np.float32)
        mask[:, y0:y1, x0:x1] = 1.0
    else:
        mask = np.full((N, H, W), {"ones": 1.0, "hole": 1.0, "0.98": 0.98, "0.995": 0.995}[s["mask"]], np.float32)
        if s["mask"] == "hole":
            for n in range(N):
                mask[(n,) + tuple(s["hole"][n % len(s["hole"])])] = 0.0
    # flow specials that shape a frame's mask
    kinds = [s["pairs"][p % len(s["pairs"])] for p in range(B * (Fr - 1))]
    frame_of = lambda p: (p // (Fr - 1)) * Fr + p % (Fr - 1)
    for p, kind in enumerate(kinds):
        n = frame_of(p)
        if kind == "empty":
            mask[n] = 0.0
        elif kind == "offmask":  # a strip of the solid patch leaves this frame's mask and stays on the next frame's
            mask[n, :, min(x0 + 1, W - 1)] = 0.0
        elif kind == "one" and H >= 3 and W >= 3:
            cy, cx = 1 + (p * 5) % (H - 2), 1 + (p * 7) % (W - 2)
            mask[n] = 0.0
            mask[n, cy - 1:cy + 2, cx - 1:cx + 2] = 1.0
            alpha[n, cy - 1:cy + 2, cx - 1:cx + 2] = 1.0
            valid[n, cy - 1:cy + 2, cx - 1:cx + 2] = 1.0
    # colours, features, distance transforms, upstream weights
    if s["rgb"] == "wide":
        rgb, image_gt = 10.0 ** rng.uniform(-3, 3, (N, H, W, 3)), 10.0 ** rng.uniform(-3, 3, (N, 3, H, W))
    else:
        rgb, image_gt = u(N, H, W, 3), u(N, 3, H, W)
    rgb, image_gt = rgb.astype(np.float32), image_gt.astype(np.float32)
    if s["rgb"] == "ties":
        gt = image_gt.transpose(0, 2, 3, 1)
        k = np.arange(N * H * W).reshape(N, H, W) % 3
        up_, dn = np.nextafter(gt, np.float32(2.0)), np.nextafter(gt, np.float32(-1.0))
        for ch in range(3):
            rgb[..., ch] = np.where(k == ch, gt[..., ch], np.where((k + 1) % 3 == ch, up_[..., ch], dn[..., ch]))
    c = dict(s, name=name, N=N)
    c["shaded"] = f32(np.concatenate([rgb, alpha[..., None]], -1))
    c["valid"], c["mask_gt"], c["image_gt"] = f32(valid), f32(mask), f32(image_gt)
    c["mask_dt"] = f32(5.0 * u(N, 2, H, W))
    c["feat"], c["feat_gt"] = (f32(u(N, H, W, D)), f32(u(N, D, H, W))) if D else (None, None)
    w = rng.normal(size=(N, 5))
    if s["up"] == "random":
        for n in range(N):
            w[n, n % 5] = 0.0
    elif s["up"] == "sum":
        w[:] = 1.0
    else:
        assert s["up"] == "cols4", s["up"]
        w[:, 4] = 0.0
    c["w_loss"] = f32(w)
    # flow
    if Fr > 1:
        both = eroded_mask(c["shaded"][..., 3].double(), c["valid"].double(), c["mask_gt"].double()).numpy()
        gtf = ((u(B * (Fr - 1), 2, H, W) - 0.5) * 0.8).astype(np.float32)
        for p, kind in enumerate(kinds):
            on = both[frame_of(p)]
            ys, xs = np.nonzero(on)
            if kind == "half" and len(ys):
                sel = np.arange(len(ys))
                gtf[p, 0, ys[sel % 3 == 0], xs[sel % 3 == 0]] = 0.5
                gtf[p, 1, ys[sel % 3 == 1], xs[sel % 3 == 1]] = -0.5
            elif kind in ("over0", "over1") and len(ys):
                i = 0 if kind == "over0" else len(ys) - 1
                gtf[p, int(kind[-1]), ys[i], xs[i]] = HALF_UP if kind == "over0" else -HALF_UP
            elif kind == "offmask":
                off = ~on & ((u(H, W) < 0.1) | both[frame_of(p) + 1])
                gtf[p, 0][off] = 0.9
                gtf[p, 1][off] = -0.7
        c["flow"] = f32((u(N, H, W, 2) - 0.5) * 0.4)
        c["flow_gt"] = f32(gtf).view(B, Fr - 1, 2, H, W)
        c["w_flow"] = torch.ones(B, Fr - 1) if s["up"] == "sum" else f32(rng.normal(size=(B, Fr - 1)))
    c["kinds"] = kinds
    return check_knife_edges(c) if check else c


# what the float32 evaluation of the restatement reaches against the float64 one, in units of 2^-24 x magnitude (maximum over the
# elements; CPU, one thread; third decimal rounded up): written by tests/test_losses_cpu.py::measure_all, asserted by
# test_measured_table_is_current
MEASURED = {
    "hw_1x1_n1": {"loss": 0.0, "g_rgb": 0.0, "g_alpha": 0.119, "g_feat": 0.0},
    "hw_1x1_b3": {"loss": 0.0, "g_rgb": 0.0, "g_alpha": 0.905, "g_feat": 0.0, "flow": 0.0, "g_flow": 0.0},
    "hw_1x7_n1": {"loss": 0.67, "g_rgb": 0.0, "g_alpha": 1.103, "g_feat": 0.0},
    "hw_1x7_b3": {"loss": 1.54, "g_rgb": 0.0, "g_alpha": 1.853, "g_feat": 0.0, "flow": 0.0, "g_flow": 0.0},
    "hw_9x1_n1": {"loss": 1.232, "g_rgb": 0.0, "g_alpha": 0.828, "g_feat": 0.0},
    "hw_9x1_b3": {"loss": 1.121, "g_rgb": 0.0, "g_alpha": 1.059, "g_feat": 0.0, "flow": 0.0, "g_flow": 0.0},
    "hw_3x85_n1": {"loss": 1.44, "g_rgb": 0.103, "g_alpha": 1.768, "g_feat": 2.146},
    "hw_3x85_b3": {"loss": 2.07, "g_rgb": 0.521, "g_alpha": 1.978, "g_feat": 2.063, "flow": 0.345, "g_flow": 2.096},
    "hw_16x16_n1": {"loss": 0.768, "g_rgb": 0.49, "g_alpha": 1.315, "g_feat": 1.736},
    "hw_16x16_b3": {"loss": 2.414, "g_rgb": 0.499, "g_alpha": 1.596, "g_feat": 1.658, "flow": 1.066, "g_flow": 1.567},
    "hw_257x1_n1": {"loss": 0.414, "g_rgb": 0.0, "g_alpha": 1.482, "g_feat": 0.0},
    "hw_257x1_b3": {"loss": 1.605, "g_rgb": 0.0, "g_alpha": 2.079, "g_feat": 0.0, "flow": 0.0, "g_flow": 0.0},
    "hw_1x257_n1": {"loss": 0.808, "g_rgb": 0.0, "g_alpha": 1.237, "g_feat": 0.0},
    "hw_1x257_b3": {"loss": 1.305, "g_rgb": 0.0, "g_alpha": 1.696, "g_feat": 0.0, "flow": 0.0, "g_flow": 0.0},
    "hw_2x300_n1": {"loss": 0.513, "g_rgb": 0.0, "g_alpha": 2.266, "g_feat": 0.0},
    "hw_2x300_b3": {"loss": 2.157, "g_rgb": 0.0, "g_alpha": 2.193, "flow": 0.0, "g_flow": 0.0},
    "hw_4x300_n3": {"loss": 1.976, "g_rgb": 0.291, "g_alpha": 2.018, "g_feat": 2.573},
    "hw_200x3_n1": {"loss": 1.723, "g_rgb": 0.897, "g_alpha": 1.726, "g_feat": 2.238},
    "hw_200x3_b3": {"loss": 2.111, "g_rgb": 0.441, "g_alpha": 2.438, "g_feat": 2.639, "flow": 0.744, "g_flow": 1.795},
    "hw_130x130_n1": {"loss": 1.715, "g_rgb": 0.253, "g_alpha": 2.077, "g_feat": 2.08},
    "hw_130x130_b3": {"loss": 2.833, "g_rgb": 0.655, "g_alpha": 2.261, "g_feat": 2.691, "flow": 1.113, "g_flow": 2.333},
    "hw_17x33_n1": {"loss": 1.508, "g_rgb": 0.08, "g_alpha": 1.874, "g_feat": 1.732},
    "hw_17x33_b3": {"loss": 1.855, "g_rgb": 0.686, "g_alpha": 2.28, "g_feat": 2.316, "flow": 0.526, "g_flow": 1.998},
    "d_none": {"loss": 1.674, "g_rgb": 0.664, "g_alpha": 1.859},
    "d1": {"loss": 2.14, "g_rgb": 0.155, "g_alpha": 1.987, "g_feat": 1.588},
    "d3": {"loss": 2.761, "g_rgb": 0.403, "g_alpha": 1.825, "g_feat": 2.113},
    "d5": {"loss": 1.578, "g_rgb": 0.468, "g_alpha": 1.695, "g_feat": 1.762},
    "d4": {"loss": 1.97, "g_rgb": 0.361, "g_alpha": 1.921, "g_feat": 1.394},
    "d8": {"loss": 2.316, "g_rgb": 0.688, "g_alpha": 1.983, "g_feat": 2.265},
    "d12": {"loss": 1.777, "g_rgb": 0.862, "g_alpha": 1.802, "g_feat": 2.219},
    "d20": {"loss": 1.514, "g_rgb": 0.403, "g_alpha": 1.896, "g_feat": 1.808},
    "d16_contig": {"loss": 1.649, "g_rgb": 0.407, "g_alpha": 1.876, "g_feat": 2.114},
    "d16_wide17": {"loss": 2.355, "g_rgb": 0.463, "g_alpha": 2.654, "g_feat": 2.558},
    "d16_offset1": {"loss": 2.133, "g_rgb": 0.449, "g_alpha": 1.94, "g_feat": 2.318},
    "d12_offset1": {"loss": 0.52, "g_rgb": 0.501, "g_alpha": 0.836, "g_feat": 1.887},
    "d260": {"loss": 0.517, "g_rgb": 0.288, "g_alpha": 1.303, "g_feat": 2.051},
    "mask_ones": {"loss": 1.662, "g_rgb": 0.377, "g_alpha": 1.701, "g_feat": 2.717},
    "mask_098": {"loss": 1.631, "g_rgb": 0.0, "g_alpha": 1.944, "g_feat": 0.0},
    "mask_0995": {"loss": 1.899, "g_rgb": 0.49, "g_alpha": 1.634, "g_feat": 2.238},
    "mask_hole_group_edge": {"loss": 2.022, "g_rgb": 0.316, "g_alpha": 1.927, "g_feat": 1.943},
    "mask_hole_row_end": {"loss": 1.66, "g_rgb": 0.672, "g_alpha": 2.259, "g_feat": 2.269},
    "rgb_ties": {"loss": 1.834, "g_rgb": 0.933, "g_alpha": 1.872},
    "rgb_wide": {"loss": 1.938, "g_rgb": 0.403, "g_alpha": 1.749},
    "no_dt1": {"loss": 1.936, "g_rgb": 0.389, "g_alpha": 1.702, "g_feat": 1.936},
    "no_dt1_sum": {"loss": 1.552, "g_rgb": 0.501, "g_alpha": 1.019, "g_feat": 1.842},
    "flow_b1_f2": {"loss": 2.17, "g_rgb": 0.077, "g_alpha": 2.028, "flow": 0.132, "g_flow": 1.466},
    "flow_b1_f4_stride3": {"loss": 1.656, "g_rgb": 0.691, "g_alpha": 1.956, "g_feat": 2.048, "flow": 0.742, "g_flow": 1.538},
    "flow_b3_f2_stride3": {"loss": 2.428, "g_rgb": 0.403, "g_alpha": 2.339, "flow": 1.055, "g_flow": 1.875},
    "flow_b3_f4": {"loss": 2.569, "g_rgb": 0.787, "g_alpha": 2.673, "g_feat": 2.552, "flow": 1.686, "g_flow": 1.956},
    "flow_b3_f4_sum": {"loss": 2.572, "g_rgb": 0.501, "g_alpha": 1.403, "flow": 1.282, "g_flow": 1.542},
}
