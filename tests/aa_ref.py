"""Restatement of the silhouette antialiasing (csrc/antialias.hip) in two separable halves, written from oracle/raster_ref.py::antialias
statement by statement, in plain torch, every function taking a dtype:

  decide(rast, clip, tri, opp, dtype)    the DISCRETE half: which adjacent pixel pairs become crossing records, as the kernel stores them
                                         in ``struct AaRec`` -- (pix0, tri, flags, alpha), flags bit 0 the direction (0 right, 1 lower
                                         neighbour), bits 1-2 the crossing edge, bit 3 the triangle belongs to the pair's second pixel,
                                         bit 4 the crossing distance was clamped -- rows sorted lexicographically so that two lists
                                         compare as sets; and, per candidate pair (a pair whose triangle ids differ), the float64 MARGIN
                                         of every discrete decision, each in its own scale (see ``margins``);
  evaluate(case, rec, alpha, buffers)    the CONTINUOUS half: takes the decisions as given and evaluates alpha (from the record's pixel,
                                         triangle, edge and direction alone, as the backward kernels do), the blends and everything
                                         downstream in the requested dtype, differentiable by autograd: the dense antialias, the rows
                                         compositor (index_copy of [vals, 1] over a background that is none, shared, per image or short
                                         of channels, the blend, the cut to ``keep`` channels), the mask compositor (ones where the raster
                                         is covered), and the depth and supersampled chains (tests/depth_ref.py, tests/msaa_ref.py with
                                         this antialias as their ``antialias`` callable).

Beside each float64 value stands its MAGNITUDE (tests/deriv_ref.py, tests/meshgeom_ref.py): the same chain over absolute inputs with an
addition for every subtraction; a gradient's magnitude is the gradient of the magnitude expression under |upstream gradient|.  Two
parts are not a plain absolute-value restatement: alpha enters at the first-order scale of its error (``alpha_scales``), and the
magnitude of g_clip is that of the edge adjoint written out term by term (``gradient_scale``), fed with every record's d(loss) /
d(alpha) and with the sum of the absolute values of that sum's terms; the depth chain carries the conditioning of its range
(``Buffer.depth_magnitude``).
Atomically summed outputs (g_clip, g_vals, g_null, blended pixels) are thereby judged against what their terms can round to, not
against a cancelled result.  Errors are in units of 2^-24 x magnitude (``units``); the kernels' bound for a run and quantity is
4 x MEASURED[run][quantity] units plus 4 ulp of the float64 value (``bad_elements``), MEASURED being what the float32 evaluation of
this same restatement reaches against its float64 evaluation (measured and asserted by tests/test_aa_cpu.py).  Nothing else enters
the bound and no element is left out.
"""
import numpy as np
import torch

from deriv_ref import EPS, units, violations  # noqa: F401  (the same unit and the same bound as the derivative suite)

import depth_ref
import msaa_ref

F64, F32 = torch.float64, torch.float32
FACTOR = 4.0
MARGINAL = 1e-4  # a candidate pair is marginal when any of its decision margins is below this, in the margin's own scale
INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------- the discrete half
def candidates(rast):
    """The adjacent pixel pairs whose triangle ids differ, right pairs (d = 0) first, then lower pairs, each in (b, y, x) order."""
    ids = rast[..., 3].long() - 1
    zw = rast[..., 2]
    parts = []
    for d in (0, 1):
        if d == 0:
            id0, id1, z0, z1 = ids[:, :, :-1], ids[:, :, 1:], zw[:, :, :-1], zw[:, :, 1:]
        else:
            id0, id1, z0, z1 = ids[:, :-1, :], ids[:, 1:, :], zw[:, :-1, :], zw[:, 1:, :]
        b, y, x = (id0 != id1).nonzero().unbind(1)
        parts.append(dict(b=b, y=y, x=x, d=torch.full_like(b, d), t0=id0[b, y, x], t1=id1[b, y, x], z0=z0[b, y, x], z1=z1[b, y, x]))
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def _same_sign(a, b):
    return torch.signbit(a) == torch.signbit(b)


def _cross(ax, ay, bx, by, cx, cy):
    """(a - c) x (b - c), the oracle's operation order: (ax - cx) * (by - cy) - (bx - cx) * (ay - cy)."""
    return (ax - cx) * (by - cy) - (bx - cx) * (ay - cy)


def _cross_scale(ax, ay, bx, by, cx, cy, sax, say, sbx, sby, scx, scy):
    """What the roundings of the six coordinates (scales s**) can move that cross product by, to first order."""
    return ((sax + scx) * (by - cy).abs() + (ax - cx).abs() * (sby + scy) + (sbx + scx) * (ay - cy).abs() + (bx - cx).abs() * (say + scy))


def geometry(c, clip, tri, opp, H, W, dtype):
    """oracle.raster_ref.antialias up to ``ok`` and ``alpha`` for the candidate pairs ``c``, both directions at once, in ``dtype``;
    every intermediate a margin needs is returned too."""
    pos = clip.to(dtype)
    tri_l, opp_l = tri.long(), torch.as_tensor(opp).long()
    b, y, x, d, t0, t1 = c["b"], c["y"], c["x"], c["d"], c["t0"], c["t1"]
    t = torch.where(t0 >= 0, t0, t1)
    both = (t0 >= 0) & (t1 >= 0)
    t = torch.where(both, torch.where(c["z0"] < c["z1"], t0, t1), t)
    use1 = t == t1
    px = x + torch.where(use1, 1 - d, torch.zeros_like(d))
    py = y + torch.where(use1, d, torch.zeros_like(d))
    ds = torch.where(use1, -1.0, 1.0).to(dtype)
    vi = tri_l[t]
    oi = opp_l[t]
    oi = torch.where(oi >= 0, oi, vi)  # no neighbour -> own vertex -> always silhouette
    pb = b if pos.shape[0] > 1 else torch.zeros_like(b)
    P, O = pos[pb[:, None], vi], pos[pb[:, None], oi]
    xh, yh = W * 0.5, H * 0.5
    fx = (px.to(dtype) + 0.5 - xh)[:, None]
    fy = (py.to(dtype) + 0.5 - yh)[:, None]
    SX, SY = P[..., 0] / P[..., 3] * xh, P[..., 1] / P[..., 3] * yh
    SOX, SOY = O[..., 0] / O[..., 3] * xh, O[..., 1] / O[..., 3] * yh
    X, Y, OX, OY = SX - fx, SY - fy, SOX - fx, SOY - fy
    mX, mY, mOX, mOY = SX.abs() + fx.abs(), SY.abs() + fy.abs(), SOX.abs() + fx.abs(), SOY.abs() + fy.abs()  # rounding scales
    x0, x1, x2 = X.unbind(-1)
    y0, y1, y2 = Y.unbind(-1)
    bb = _cross(x1, y1, x2, y2, x0, y0)
    w = torch.stack([_cross(x1, y1, x2, y2, OX[:, 0], OY[:, 0]), _cross(x2, y2, x0, y0, OX[:, 1], OY[:, 1]), _cross(x0, y0, x1, y1, OX[:, 2], OY[:, 2])], -1)
    sil = _same_sign(w, bb[:, None])
    s_bb = _cross_scale(x1, y1, x2, y2, x0, y0, mX[:, 1], mY[:, 1], mX[:, 2], mY[:, 2], mX[:, 0], mY[:, 0])
    s_w = torch.stack([_cross_scale(X[:, (k + 1) % 3], Y[:, (k + 1) % 3], X[:, (k + 2) % 3], Y[:, (k + 2) % 3], OX[:, k], OY[:, k], mX[:, (k + 1) % 3],
                                    mY[:, (k + 1) % 3], mX[:, (k + 2) % 3], mY[:, (k + 2) % 3], mOX[:, k], mOY[:, k]) for k in range(3)], -1)
    d1 = (d == 1)[:, None]  # pair direction becomes the first coordinate
    X, Y, mX, mY = torch.where(d1, Y, X), torch.where(d1, X, Y), torch.where(d1, mY, mX), torch.where(d1, mX, mY)
    nxt, nn = [1, 2, 0], [2, 0, 1]  # edge i joins vertices (i+1, i+2)
    xa, ya, xb, yb = X[:, nxt], Y[:, nxt], X[:, nn], Y[:, nn]
    dxe, dye = xb - xa, yb - ya
    num = ds[:, None] * (xa * dye - ya * dxe)
    straddle = ~_same_sign(ya, yb)
    ratio = torch.where(straddle, num / torch.where(straddle, dye, torch.ones_like(dye)), torch.full_like(num, -INF))
    di = torch.zeros_like(t)  # argmax, ties to the lowest index
    best = ratio[:, 0]
    for k in (1, 2):
        better = ratio[:, k] > best
        di = torch.where(better, torch.full_like(di, k), di)
        best = torch.where(better, ratio[:, k], best)
    pick = lambda v: v.gather(1, di[:, None])[:, 0]
    dc = best
    ok = pick(sil) & pick(straddle) & (pick(dye).abs() >= pick(dxe).abs()) & (dc > -0.0625) & (dc < 1.0625)
    alpha = ds * (0.5 - dc.clamp(0.0, 1.0))
    clamped = (dc < 0.0) | (dc > 1.0)
    flags = d | (di << 1) | (use1.long() << 3) | (clamped.long() << 4)
    pix0 = (b * H + y) * W + x
    # rounding scales in the pair frame (first order): of the edge differences, the numerator and the ratio
    s_dy, s_dx = mY[:, nxt] + mY[:, nn], mX[:, nxt] + mX[:, nn]
    s_num = mX[:, nxt] * dye.abs() + xa.abs() * s_dy + mY[:, nxt] * dxe.abs() + ya.abs() * s_dx
    safe = torch.where(straddle, dye.abs(), torch.ones_like(dye))
    s_ratio = torch.where(straddle, s_num / safe + ratio.abs() * s_dy / safe, torch.zeros_like(num))
    return dict(t=t, use1=use1, ds=ds, di=di, ok=ok, dc=dc, alpha=alpha, flags=flags, pix0=pix0, both=both, bb=bb, w=w, s_bb=s_bb, s_w=s_w, own=(opp_l[t] < 0),
                Y=Y, mY=mY, ratio=ratio, s_ratio=s_ratio, straddle=straddle, dxe=dxe, dye=dye, s_dx=s_dx, s_dy=s_dy, pick=pick)


def margins(c, g):
    """Per candidate pair, the distance of every discrete decision from its switch, relative to what the roundings of a float32
    evaluation can move it by (``g``: the float64 geometry).  name -> float64 [n]; inf where the decision does not arise.

      depth     |z0 - z1| / max(|z0|, |z1|)                 both pixels covered: which triangle the pair takes
      straddle  min_k |Y_k| / (|y_k / w_k yh| + |fy|)        the sign of each vertex' coordinate across the pair direction
      ratio     min_k |best - ratio_k| / scale               the gaps between the crossing distances of the straddling edges
      slope     ||dy| - |dx|| / (scale dy + scale dx)        the 45-degree test of the chosen edge
      lo, hi    (dc + 1/16), (17/16 - dc) / (scale + 1)      the acceptance window
      zero, one |dc|, |1 - dc| / (scale + 1)                 the clamp flag
      w, bb     |w| / scale, |bb| / scale                    the silhouette test (w: only with a neighbour across the chosen edge)

    The depth rule compares two stored float32 values: an exact tie is decided the same way by every evaluation and has no margin.
    Second result: bool [n], the pairs REFUSED decisively -- one of the acceptance tests (slope, window, silhouette) fails with its own
    margin(s) at or above MARGINAL, so that no rounding of the others can turn the pair into a record.
    """
    n = c["b"].shape[0]
    inf = torch.full((n,), INF, dtype=F64)
    z0, z1 = c["z0"].double(), c["z1"].double()
    zs = torch.maximum(z0.abs(), z1.abs())
    out = dict(depth=torch.where(g["both"] & (z0 != z1), (z0 - z1).abs() / torch.where(zs > 0, zs, torch.ones_like(zs)), inf))
    out["straddle"] = (g["Y"].abs() / g["mY"]).min(-1).values
    pick, st = g["pick"], g["straddle"]
    any_st = pick(st)
    best, sb = g["dc"], pick(g["s_ratio"])
    gaps = torch.where(st, (best[:, None] - g["ratio"]).abs() / torch.maximum(sb[:, None], g["s_ratio"]).clamp_min(1e-300), inf[:, None])
    gaps = gaps.scatter(1, g["di"][:, None], INF)
    out["ratio"] = torch.where(any_st, gaps.min(-1).values, inf)
    out["slope"] = torch.where(any_st, (pick(g["dye"]).abs() - pick(g["dxe"]).abs()).abs() / (pick(g["s_dy"]) + pick(g["s_dx"])), inf)
    for name, v in (("lo", best + 0.0625), ("hi", 1.0625 - best), ("zero", best), ("one", 1.0 - best)):
        out[name] = torch.where(any_st, v.abs() / (sb + 1.0), inf)
    out["w"] = torch.where(any_st & ~pick(g["own"]), pick(g["w"]).abs() / pick(g["s_w"]).clamp_min(1e-300), inf)
    out["bb"] = torch.where(any_st, g["bb"].abs() / g["s_bb"].clamp_min(1e-300), inf)
    far = lambda *names: torch.stack([out[k] for k in names], 0).min(0).values >= MARGINAL
    slope_ok, sil_ok = pick(g["dye"]).abs() >= pick(g["dxe"]).abs(), _same_sign(pick(g["w"]), g["bb"])
    refused = (~any_st) | (~slope_ok & far("slope")) | (~(best > -0.0625) & far("lo")) | (~(best < 1.0625) & far("hi")) | (~sil_ok & far("w", "bb"))
    return out, refused


def decide(rast, clip, tri, opp=None, dtype=F32):
    """The crossing records of (rast, clip, tri) as a3d_aa_analyze defines them, decided in ``dtype``:
    dict(rec int64 [N,3] = (pix0, tri, flags) sorted lexicographically, alpha ``dtype`` [N] in that order,
         cand int64 [M,2] = (pix0, d) of every candidate pair, margins name -> float64 [M], margin float64 [M] their minimum,
         marginal bool [M]: a margin below MARGINAL that can change the pair's outcome, see ``margins``)."""
    from oracle import raster_ref

    if clip.dim() == 2:
        clip = clip[None]
    B, H, W = rast.shape[:3]
    if opp is None:
        opp = raster_ref.edge_opposites(tri.cpu().numpy())
    c = candidates(rast)
    g = geometry(c, clip, tri, opp, H, W, dtype)
    m, refused = margins(c, g if dtype == F64 else geometry(c, clip, tri, opp, H, W, F64))
    ok = g["ok"]
    rec = torch.stack([g["pix0"][ok], g["t"][ok], g["flags"][ok]], 1)
    order = torch.from_numpy(np.lexsort(rec.numpy().T[::-1])).long() if rec.shape[0] else torch.zeros(0, dtype=torch.long)
    least = lambda names: torch.stack([m[k] for k in names], 0).min(0).values
    # a pair is marginal when a rounding can change its OUTCOME: the choice of triangle and edge always can; the acceptance tests and
    # the clamp flag only where the pair is not refused decisively by one of them
    marginal = (least(("depth", "straddle", "ratio")) < MARGINAL) | (~refused & (least(("slope", "lo", "hi", "zero", "one", "w", "bb")) < MARGINAL))
    return dict(rec=rec[order], alpha=g["alpha"][ok][order], cand=torch.stack([g["pix0"], c["d"]], 1), margins=m, margin=least(tuple(m)), marginal=marginal)


# ---------------------------------------------------------------------------------------------------------------- the continuous half
def _den(true_abs, mag_sum):
    """A denominator of a magnitude expression: the true |value|, with the derivative of the absolute sum, negated."""
    return true_abs.detach() - (mag_sum - mag_sum.detach())


def unpack(rec, H, W):
    pix0, t, flags = rec[:, 0], rec[:, 1], rec[:, 2]
    d, di, use1, cl = flags & 1, (flags >> 1) & 3, (flags >> 3) & 1, (flags >> 4) & 1
    rem = pix0 % (H * W)
    y, x = rem // W, rem % W
    return dict(pix0=pix0, t=t, d=d, di=di, use1=use1, clamped=cl.bool(), b=pix0 // (H * W), px=x + use1 * (1 - d), py=y + use1 * d, p1=pix0 + torch.where(d == 1, W, 1))


def record_alpha(rec, alpha_rec, clip, tri, H, W, no_w=False):
    """alpha of every record from its pixel, triangle, edge and direction, in clip's dtype (the statements of the oracle on the ONE
    edge the record names); a clamped record's alpha is the recorded constant.  ``no_w``: the w-gradient is cut (a mutation for
    tests/test_aa_cpu.py)."""
    u = unpack(rec, H, W)
    dtype = clip.dtype
    tri_l = tri.long()
    pb = u["b"] if clip.shape[0] > 1 else torch.zeros_like(u["b"])
    ia, ib = tri_l[u["t"], (u["di"] + 1) % 3], tri_l[u["t"], (u["di"] + 2) % 3]
    xh, yh = W * 0.5, H * 0.5
    fx, fy = (u["px"].to(dtype) + 0.5 - xh), (u["py"].to(dtype) + 0.5 - yh)
    ds = torch.where(u["use1"] == 1, -1.0, 1.0).to(dtype)
    d1 = u["d"] == 1
    Pa, Pb = clip[pb, ia], clip[pb, ib]
    wa, wb = (Pa[:, 3].detach(), Pb[:, 3].detach()) if no_w else (Pa[:, 3], Pb[:, 3])
    sxa, sya, sxb, syb = Pa[:, 0] / wa * xh - fx, Pa[:, 1] / wa * yh - fy, Pb[:, 0] / wb * xh - fx, Pb[:, 1] / wb * yh - fy
    xa, ya, xb, yb = torch.where(d1, sya, sxa), torch.where(d1, sxa, sya), torch.where(d1, syb, sxb), torch.where(d1, sxb, syb)
    dxe, dye = xb - xa, yb - ya
    dc = ds * (xa * dye - ya * dxe) / dye
    alpha = ds * (0.5 - dc)
    return torch.where(u["clamped"], alpha_rec.to(dtype), alpha)


def alpha_scales(rec, clip, tri, H, W):
    """What the roundings of a float32 evaluation can move alpha and its position gradient by, to FIRST order, per record (float64, from
    the true values; ``clip`` [1|B,V,4] float64).  With S(.) the scale of a quantity's absolute error in units of 2^-24:

        X = x / w xh - fx        S(X) = |x / w xh| + |fx|                      (pair frame: X along the pair, Y across)
        D = Yb - Ya, dX = Xb - Xa   S(D) = S(Ya) + S(Yb), S(dX) = S(Xa) + S(Xb)
        num = Xa D - Ya dX       S(num) = S(Xa) |D| + |Xa| S(D) + S(Ya) |dX| + |Ya| S(dX) + |Xa D| + |Ya dX|
        dc = num / D             S(dc) = S(num) / |D| + |dc| S(D) / |D|
        alpha = ds (1/2 - dc)    S(alpha) = 1/2 + S(dc);  a clamped record: 1/2 (the constant itself)

    (The plain absolute-value restatement would multiply two coordinate magnitudes, |fx| |fy| / |D|: a pixel's distance from the image
    centre squared, where the error grows with the distance.)  ``gradient_scale`` turns d(loss)/d(alpha) into the scale of g_clip."""
    u = unpack(rec, H, W)
    tri_l = tri.long()
    pb = u["b"] if clip.shape[0] > 1 else torch.zeros_like(u["b"])
    ia, ib = tri_l[u["t"], (u["di"] + 1) % 3], tri_l[u["t"], (u["di"] + 2) % 3]
    xh, yh = W * 0.5, H * 0.5
    fx, fy = (u["px"].double() + 0.5 - xh), (u["py"].double() + 0.5 - yh)
    d1 = u["d"] == 1
    Pa, Pb = clip[pb, ia], clip[pb, ib]
    sxa, sya, sxb, syb = Pa[:, 0] / Pa[:, 3] * xh, Pa[:, 1] / Pa[:, 3] * yh, Pb[:, 0] / Pb[:, 3] * xh, Pb[:, 1] / Pb[:, 3] * yh
    sw = lambda p, q: (torch.where(d1, q, p), torch.where(d1, p, q))
    Xa, Ya = sw(sxa - fx, sya - fy)
    Xb, Yb = sw(sxb - fx, syb - fy)
    SXa, SYa = sw(sxa.abs() + fx.abs(), sya.abs() + fy.abs())
    SXb, SYb = sw(sxb.abs() + fx.abs(), syb.abs() + fy.abs())
    D, dX, SD, SdX = Yb - Ya, Xb - Xa, SYa + SYb, SXa + SXb
    aD = D.abs()
    Snum = SXa * aD + Xa.abs() * SD + SYa * dX.abs() + Ya.abs() * SdX + (Xa * D).abs() + (Ya * dX).abs()
    dc = (Xa * D - Ya * dX) / D
    Sdc = Snum / aD + dc.abs() * SD / aD
    S_alpha = torch.where(u["clamped"], torch.full_like(Sdc, 0.5), 0.5 + Sdc)
    return dict(u=u, rows_a=pb * clip.shape[1] + ia, rows_b=pb * clip.shape[1] + ib, Pa=Pa, Pb=Pb, d1=d1, Xa=Xa, Ya=Ya, Xb=Xb, Yb=Yb, SXa=SXa, SYa=SYa,
                SXb=SXb, SYb=SYb, D=D, dX=dX, SD=SD, SdX=SdX, S_alpha=S_alpha, xh=xh, yh=yh)


def gradient_scale(sc, g_alpha, M_alpha, clip_shape):
    """The scale of g_clip [1|B,V,4] from every record's d(loss)/d(alpha) (``g_alpha``) and that sum's own magnitude ``M_alpha`` (the sum of
    the absolute values of its terms).  The adjoint of xint = (Xa Yb - Ya Xb) / D, term by term, each factor's error in turn:

        gXa = g Yb / D                  S = M |Yb| / |D| + |g| (S(Yb) / |D| + |Yb| S(D) / D^2)          (gXb: Ya for Yb)
        gYa = g Yb (Xa - Xb) / D^2      S = M |Yb dX| / D^2 + |g| (S(Yb) |dX| + |Yb| S(dX)) / D^2 + 2 |g| |Yb dX| S(D) / |D|^3   (gYb: Ya for Yb)
        g_x = gsx xh / w                S = S(gsx) xh / |w|                                                (g_y alike)
        g_w = -(gsx x xh + gsy y yh) / w^2   S = (S(gsx) |x| xh + S(gsy) |y| yh) / w^2

    A clamped record has no position gradient: scale 0 (the kernels must leave exact zeros)."""
    g, M = g_alpha.abs(), M_alpha
    live = (~sc["u"]["clamped"]).double()
    aD, adX = sc["D"].abs(), sc["dX"].abs()
    out = torch.zeros(clip_shape[0] * clip_shape[1], 4, dtype=F64)
    for Y, SY, P, rows in ((sc["Yb"], sc["SYb"], sc["Pa"], sc["rows_a"]), (sc["Ya"], sc["SYa"], sc["Pb"], sc["rows_b"])):
        aY = Y.abs()
        SgX = (M * aY / aD + g * (SY / aD + aY * sc["SD"] / aD ** 2)) * live
        SgY = (M * aY * adX / aD ** 2 + g * (SY * adX + aY * sc["SdX"]) / aD ** 2 + 2 * g * aY * adX * sc["SD"] / aD ** 3) * live
        Sgsx, Sgsy = torch.where(sc["d1"], SgY, SgX), torch.where(sc["d1"], SgX, SgY)
        aw = P[:, 3].abs()
        col = torch.stack([Sgsx * sc["xh"] / aw, Sgsy * sc["yh"] / aw, torch.zeros_like(aw), (Sgsx * P[:, 0].abs() * sc["xh"] + Sgsy * P[:, 1].abs() * sc["yh"]) / aw ** 2], 1)
        out = out.index_add(0, rows, col)
    return out.view(clip_shape)


def blend(pre, rec, alpha, dst, W, mag=False, tap=None):
    """pre [B,H,W,C] + the blends of the records: pixel ``dst`` of a record takes alpha * (pre[p1] - pre[p0]); input colours only.
    ``tap`` (a list): the two colours every record reads are appended -- their adjoints are the records' own terms."""
    C = pre.shape[-1]
    flat = pre.reshape(-1, C)
    p0 = rec[:, 0]
    p1 = p0 + torch.where((rec[:, 2] & 1) == 1, W, 1)
    c1, c0 = flat[p1], flat[p0]
    if tap is not None:
        tap.append((c1, c0, p1, p0))
    if rec.shape[0] == 0:
        return pre
    diff = c1 + c0 if mag else c1 - c0
    return flat.index_add(0, dst, alpha[:, None] * diff).view(pre.shape)


def destinations(rec, alpha_rec, W):
    p0 = rec[:, 0]
    return torch.where(alpha_rec > 0, p0, p0 + torch.where((rec[:, 2] & 1) == 1, W, 1))


def covered_list(rast):
    """Flat indices of the covered pixels, ascending (the order of every row tensor of this module)."""
    return torch.nonzero(rast[..., 3].reshape(-1) > 0)[:, 0]


def _padded(bg, shape, dtype):
    """A background [1|B,H,W,<=C] as [B,H,W,C] (missing trailing channels zero) or zeros."""
    B, H, W, C = shape
    if bg is None:
        return torch.zeros(shape, dtype=dtype)
    bg = bg.to(dtype)
    return torch.cat([bg, bg.new_zeros(*bg.shape[:3], C - bg.shape[3])], -1).expand(B, H, W, C)


class Buffer:
    """One image of an evaluation: ``form`` 'dense' (color [B,H,W,C]), 'rows' (vals [>= P,C], bg, keep), 'mask' (C, bg), 'msaa' (vals
    [>= P_lo,C], null [B,C], bg on the shading grid, s, keep) or 'depth' (gb [P,3] positions, w2c [1|B,4,4]); ``g`` the upstream gradient
    of the image it hands out.  Tensors are float32 on the CPU; ``leaves`` names the differentiable ones."""

    def __init__(self, form, g, **kw):
        self.form, self.g, self.kw = form, g, kw
        self.leaves = {"dense": ("color",), "rows": ("vals",), "mask": (), "msaa": ("vals", "null"), "depth": ("gb",)}[form]

    def image(self, leaves, case, aa, dtype, mag=False):
        """The image from the leaf tensors ``leaves`` (dtype; absolute values when ``mag``) through the antialias callable ``aa``."""
        k, rast = self.kw, case["rast"]
        B, H, W = rast.shape[:3]
        absd = (lambda t: t.abs()) if mag else (lambda t: t)
        if self.form == "dense":
            return aa(leaves["color"])
        if self.form == "rows":
            vals, pix = leaves["vals"], covered_list(rast)
            C = vals.shape[1]
            bg = None if k.get("bg") is None else absd(k["bg"].to(dtype))
            pre = _padded(bg, (B, H, W, C + 1), dtype).reshape(-1, C + 1)
            pre = pre.index_copy(0, pix, torch.cat([vals[:pix.shape[0]], torch.ones(pix.shape[0], 1, dtype=dtype)], 1)).view(B, H, W, C + 1)
            return aa(pre)[..., :(C + 1 if k.get("keep") is None else k["keep"])]
        if self.form == "mask":
            C = k["C"]
            bg = None if k.get("bg") is None else absd(k["bg"].to(dtype))
            cov = (rast[..., 3:4] > 0).expand(B, H, W, C + 1)
            return aa(torch.where(cov, torch.ones((), dtype=dtype), _padded(bg, (B, H, W, C + 1), dtype)).contiguous())
        if self.form == "msaa":
            s = k["s"]
            vals, null = leaves["vals"], leaves["null"]
            C = vals.shape[1]
            # msaa_ref's chain with the magnification written as a GATHER per full-resolution sample (its block's row, or its image's
            # null row): the same values, but the adjoints of vals and null then accumulate sample by sample, as the kernels' atomics do
            # and as every other summed gradient of this module does (behind msaa_ref.magnify_nearest they are blocked sums).
            # compose(..., s = 1) composites and antialiases at full resolution as stated there; avg_pool follows.
            lo = msaa_ref.minify_nearest(rast, s)
            h, w, pix_lo = H // s, W // s, covered_list(lo)
            inv_lo = torch.full((B * h * w,), -1, dtype=torch.long)
            inv_lo[pix_lo] = torch.arange(pix_lo.shape[0])
            bb, yy, xx = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
            row = inv_lo[((bb * h + yy // s) * w + xx // s).reshape(-1)]
            rows = torch.where((row >= 0)[:, None], vals[row.clamp(min=0)], null[bb.reshape(-1)])
            shaded = torch.cat((rows, torch.ones_like(rows[:, :1])), -1).view(B, H, W, C + 1)
            bg = None if k.get("bg") is None else msaa_ref.magnify_nearest(absd(k["bg"].to(dtype)), s)
            out = msaa_ref.avg_pool(msaa_ref.compose(shaded, rast, bg, 1, aa), s)
            return out[..., :(C + 1 if k.get("keep") is None else k["keep"])]
        assert self.form == "depth" and not mag
        # depth_ref.image with its lerp(0, [d, 1], coverage) written as the select it is (coverage is 0 or 1): an image that nothing
        # covers has the range 0 and d = 0 / 0 on every pixel, which the lerp would hand on as NaN where the kernels write zeros
        d = depth_ref.depth(depth_ref.dense_positions(leaves["gb"], covered_list(rast), (B, H, W)), k["w2c"].to(dtype))
        cover = (rast[..., 3:4] > 0).expand(B, H, W, 2)
        return aa(torch.where(cover, torch.cat((d, torch.ones_like(d)), -1), torch.zeros((), dtype=dtype)).contiguous())[..., :1]

    def depth_magnitude(self, leaves_abs, true_gb, case, aa_mag):
        """The depth image's magnitude expression over |gb|: z = |p| . |row| + |t|, d = (z + lo) / R + |d| (hi + lo) / R with the true range R
        and the true normalised value d (the second term: what a rounding of the two extremes moves every value by), composited and blended."""
        k, rast = self.kw, case["rast"]
        B, H, W = rast.shape[:3]
        pix, cover = covered_list(rast), rast[..., 3] > 0
        w2c = k["w2c"].double()
        zt = depth_ref.camera_z(depth_ref.dense_positions(true_gb, pix, (B, H, W)), w2c)
        zm = depth_ref.camera_z(depth_ref.dense_positions(leaves_abs["gb"], pix, (B, H, W)), w2c.abs())
        flat_t, flat_m = zt.view(B, -1), zm.view(B, -1)
        i_lo, i_hi = flat_t.argmin(1, keepdim=True), flat_t.argmax(1, keepdim=True)
        lo_t, hi_t, lo_m, hi_m = flat_t.gather(1, i_lo), flat_t.gather(1, i_hi), flat_m.gather(1, i_lo), flat_m.gather(1, i_hi)
        R_t = torch.where(hi_t > lo_t, hi_t - lo_t, torch.ones_like(hi_t))  # (range 0: an image nothing covers, every pixel selected out)
        R = _den(R_t, hi_m + lo_m)
        d_t = ((flat_t - lo_t) / R_t).abs().detach()
        dm = ((flat_m + lo_m) / R + d_t * (hi_m + lo_m) / R).view(B, H, W, 1)
        cover2 = cover[..., None].expand(B, H, W, 2)
        return aa_mag(torch.where(cover2, torch.cat((dm, torch.ones_like(dm)), -1), torch.zeros((), dtype=F64)).contiguous())[..., :1]


def _flat_msaa_sums(case, buf, tap, loss, gen):
    """(g_vals, g_null) of a supersampled buffer as the flat sums the kernels form, one per value row and one per (image, channel): see
    ``evaluate`` (flat_null)."""
    rast, s = case["rast"], buf.kw["s"]
    B, H, W = rast.shape[:3]
    h, w, n = H // s, W // s, s * s
    vals = buf.kw["vals"]
    C, dt = vals.shape[1], loss.dtype
    cov = (rast[..., 3] > 0)
    k = cov.view(B, h, s, w, s).sum((2, 4)).reshape(-1)
    pix_lo = covered_list(rast[:, ::s, ::s])
    P = pix_lo.shape[0]
    group_of_block = torch.arange(B).repeat_interleave(h * w) + P  # a block without a row feeds its image's null row (group P + b)
    group_of_block[pix_lo] = torch.arange(P)
    g = buf.g.to(dt).reshape(B * h * w, -1)
    go = torch.zeros(B * h * w, C, dtype=dt)
    go[:, :min(C, g.shape[1])] = g[:, :min(C, g.shape[1])]
    block_terms = torch.where((k == n)[:, None], go, k.to(dt)[:, None] * go / n)
    c1, c0, p1, p0 = tap
    g1, g0 = torch.autograd.grad(loss, [c1, c0], retain_graph=True, allow_unused=True)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    blk = ((yy // s) * w + xx // s).reshape(-1)
    terms, groups = [block_terms[k > 0]], [group_of_block[k > 0]]  # ms_gather_kernel runs first: the blocks' terms lead
    rec_t, rec_g = [], []
    for gr, p in ((g1, p1), (g0, p0)):
        if gr is not None and p.shape[0]:
            live = cov.reshape(-1)[p]
            rec_t.append(gr[live][:, :C])
            rec_g.append(group_of_block[(p[live] // (H * W)) * h * w + blk[p[live] % (H * W)]])
    if rec_t:
        rt, rg = torch.cat(rec_t, 0), torch.cat(rec_g, 0)
        order = torch.randperm(rt.shape[0], generator=gen)
        terms.append(rt[order])
        groups.append(rg[order])
    terms, groups = torch.cat(terms, 0), torch.cat(groups, 0)
    acc = torch.zeros(P + B, C, dtype=dt)
    for t, q in zip(terms, groups.tolist()):  # one addition per term, each rounded to the dtype (torch's own sums accumulate wider)
        acc[q] = acc[q] + t
    g_vals = torch.zeros(vals.shape, dtype=dt)
    g_vals[:P] = acc[:P]
    return g_vals, acc[P:]


def evaluate(case, rec, alpha_rec, buffers, dtype=F64, mutate=None, flat_null=None):
    """The images of ``buffers`` over the records (rec, alpha_rec) of ``case`` (dict with rast, clip, tri) and the gradients of
    loss = sum_i (image_i * g_i).sum() in every leaf and in clip.  float64: name -> (value, magnitude); other dtypes: name -> value.
    Names: out{i}, g_{leaf}{i}, g_clip.  ``mutate`` = (kind, record index): a deliberately wrong evaluation (tests/test_aa_cpu.py):
    'drop' the record, 'flip' its alpha, 'unclamp' a clamped record (it gets its position gradient), 'swap' its destination pixel,
    'no_w' (every record: the w-gradient term omitted), 'slot' (rows with C = 1: the record's adjoint to its first pixel's row is lost,
    as if another record's store had overwritten the role slot).
    ``flat_null`` (a seed; float32 measurements): g_null and g_vals of the supersampled buffers as the FLAT sums the kernels form -- per
    (image, channel) one term per block that has covered samples but no row, (k go) / s^2 (ms_gather_kernel, launched first; a block
    with a row: that row's first term), then one term alpha g / s^2 per record and covered sample of the block (ms_bwd_kernel), in a
    seeded random order, added one by one in float32.  Tens of terms per row and some hundred per null row, many of them equal (a few
    alphas times a few block gradients), where every other output sums a handful; autograd groups them per sample and per block first,
    and the float32 error of a long sum depends on exactly that.  tests/test_aa_cpu.py measures these two quantities on this sum: the
    largest figure over eight orders, and autograd's."""
    rast, tri = case["rast"], case["tri"]
    B, H, W = rast.shape[:3]
    clip0 = case["clip"] if case["clip"].dim() == 3 else case["clip"][None]
    kind, which = mutate if mutate is not None else (None, None)
    dst = destinations(rec, alpha_rec, W)
    if kind == "drop":
        keep = torch.ones(rec.shape[0], dtype=torch.bool)
        keep[which] = False
        rec, alpha_rec, dst = rec[keep], alpha_rec[keep], dst[keep]
    if kind == "swap":
        dst = dst.clone()
        p0 = rec[which, 0]
        dst[which] = p0 if dst[which] != p0 else unpack(rec, H, W)["p1"][which]
    clip = clip0.detach().clone().to(dtype).requires_grad_(True)
    alpha = record_alpha(rec, alpha_rec, clip, tri, H, W, no_w=(kind == "no_w"))
    if kind == "unclamp":  # the clamped record keeps its alpha and gets the position gradient of the unclamped expression
        loose = rec.clone()
        loose[which, 2] &= ~16
        extra = record_alpha(loose, alpha_rec, clip, tri, H, W)
        only = torch.zeros_like(alpha)
        only[which] = 1.0
        alpha = alpha + only * (extra - extra.detach())
    if kind == "flip":
        sign = torch.ones_like(alpha)
        sign[which] = -1.0
        alpha = alpha * sign
    taps = []
    aa = lambda img: blend(img, rec, alpha, dst, W, tap=taps)
    leaves, outs, loss = [], [], 0.0
    for buf in buffers:
        lv = {n: buf.kw[n].detach().clone().to(dtype).requires_grad_(True) for n in buf.leaves}
        out = buf.image(lv, case, aa, dtype)
        assert out.shape == buf.g.shape, (buf.form, tuple(out.shape), tuple(buf.g.shape))
        loss = loss + (out * buf.g.to(dtype)).sum()
        leaves.append(lv)
        outs.append(out)
    flat = [clip] + [t for lv in leaves for t in lv.values()]
    grads = torch.autograd.grad(loss, flat, allow_unused=True, retain_graph=True) if torch.is_tensor(loss) and loss.requires_grad else [None] * len(flat)
    grads = [torch.zeros_like(t) if g is None else g for t, g in zip(flat, grads)]
    val = dict(g_clip=grads[0].view(case["clip"].shape) if case["clip"].dim() == 2 else grads[0])
    it = iter(grads[1:])
    for i, (buf, lv, out) in enumerate(zip(buffers, leaves, outs)):
        val[f"out{i}"] = out.detach()
        for n in lv:
            val[f"g_{n}{i}"] = next(it)
    if flat_null is not None:
        for i, buf in enumerate(buffers):
            if buf.form == "msaa":
                val[f"g_vals{i}"], val[f"g_null{i}"] = _flat_msaa_sums(case, buf, taps[i], loss, torch.Generator().manual_seed(1000 * flat_null + i))
    if kind == "slot":
        u = unpack(rec, H, W)
        pix = covered_list(rast)
        row = int(torch.searchsorted(pix, u["pix0"][which]))
        assert int(pix[row]) == int(u["pix0"][which]) and buffers[0].form == "rows" and buffers[0].kw["vals"].shape[1] == 1
        val["g_vals0"] = val["g_vals0"].clone()
        val["g_vals0"][row, 0] += alpha[which].detach() * buffers[0].g.to(dtype).reshape(-1, buffers[0].g.shape[-1])[dst[which], 0]
    if dtype != F64:
        return val
    # ---- magnitudes: the same chain over absolute values, alpha at its first-order scale; g_clip from the records' adjoints
    sc = alpha_scales(rec, clip0.double(), tri, H, W)
    alpha_m = sc["S_alpha"].clone().requires_grad_(True)
    aa_m = lambda img: blend(img, rec, alpha_m, dst, W, mag=True)
    leaves_m, outs_m, loss_m = [], [], 0.0
    for buf, lv in zip(buffers, leaves):
        la = {n: t.detach().abs().requires_grad_(True) for n, t in lv.items()}
        om = buf.depth_magnitude(la, lv["gb"].detach(), case, aa_m) if buf.form == "depth" else buf.image(la, case, aa_m, F64, mag=True)
        loss_m = loss_m + (om * buf.g.double().abs()).sum()
        leaves_m.append(la)
        outs_m.append(om)
    flat_m = [alpha_m] + [t for la in leaves_m for t in la.values()]
    gm = torch.autograd.grad(loss_m, flat_m, allow_unused=True) if torch.is_tensor(loss_m) and loss_m.requires_grad else [None] * len(flat_m)
    gm = [torch.zeros_like(t) if g is None else g for t, g in zip(flat_m, gm)]
    g_alpha = torch.autograd.grad(loss, alpha, allow_unused=True)[0] if torch.is_tensor(loss) and loss.requires_grad and rec.shape[0] else None
    g_alpha = torch.zeros_like(gm[0]) if g_alpha is None else g_alpha
    mag = dict(g_clip=gradient_scale(sc, g_alpha, gm[0], tuple(clip0.shape)).view(val["g_clip"].shape))
    it = iter(gm[1:])
    for i, (la, om) in enumerate(zip(leaves_m, outs_m)):
        mag[f"out{i}"] = om.detach()
        for n in la:
            mag[f"g_{n}{i}"] = next(it)
    return {k: (val[k], mag[k]) for k in val}


# ---------------------------------------------------------------------------------------------------------------- bounds
def figure(run, key):
    """What the float32 evaluation of the restatement reaches on quantity ``key`` of run ``run`` (units of 2^-24 x magnitude)."""
    return MEASURED[run][key]


def allowed_units(run, key):
    return FACTOR * figure(run, key)


def bad_elements(got, ref, mag, run, key, fig=None):
    """Indices where |got - ref| > 2^-24 (4 x figure(run, key) x magnitude + 4 |ref|); non-finite values violate."""
    return violations(got, ref, mag, figure(run, key) if fig is None else fig, factor=FACTOR, floor_ulp=4.0)


# what the float32 evaluation of ``evaluate`` reaches against its float64 evaluation, given the float32 decisions, in units of 2^-24 x
# magnitude (maximum over the elements; CPU, one thread; third decimal rounded up): written by tests/test_aa_cpu.py::measure_all,
# asserted by test_measured_table_is_current
MEASURED = {
    "checker_16x16:dense": {"g_clip": 0.476, "out0": 0.085, "g_color0": 0.068},
    "checker_16x16:rows": {"g_clip": 0.382, "out0": 0.065, "g_vals0": 0.041},
    "checker_16x16:rows2": {"g_clip": 1.178, "out0": 0.047, "g_vals0": 0.04, "out1": 0.102, "g_vals1": 0.08},
    "checker_16x16:mask": {"g_clip": 1.021, "out0": 0.057},
    "partial_16x16:dense": {"g_clip": 0.817, "out0": 0.085, "g_color0": 0.077},
    "partial_16x16:rows": {"g_clip": 0.698, "out0": 0.053, "g_vals0": 0.092},
    "partial_16x16:rows2": {"g_clip": 0.554, "out0": 0.064, "g_vals0": 0.102, "out1": 0.094, "g_vals1": 0.068},
    "partial_16x16:mask": {"g_clip": 0.345, "out0": 0.042},
    "checker_3x512:dense": {"g_clip": 0.833, "out0": 0.105, "g_color0": 0.113},
    "checker_3x512:rows": {"g_clip": 1.073, "out0": 0.054, "g_vals0": 0.088},
    "checker_3x512:rows2": {"g_clip": 0.718, "out0": 0.058, "g_vals0": 0.054, "out1": 0.087, "g_vals1": 0.122},
    "checker_3x512:mask": {"g_clip": 0.85, "out0": 0.047},
    "every_3x512:dense": {"g_clip": 1.295, "out0": 0.123, "g_color0": 0.13},
    "every_3x512:rows": {"g_clip": 1.268, "out0": 0.071, "g_vals0": 0.125},
    "every_3x512:rows2": {"g_clip": 1.318, "out0": 0.098, "g_vals0": 0.65, "out1": 0.144, "g_vals1": 0.377},
    "every_3x512:mask": {"g_clip": 0.0, "out0": 0.0},
    "narrow_1x1:dense": {"g_clip": 0.0, "out0": 0.0, "g_color0": 0.0},
    "narrow_1x1:rows": {"g_clip": 0.0, "out0": 0.0, "g_vals0": 0.0},
    "narrow_1x1:rows2": {"g_clip": 0.0, "out0": 0.0, "g_vals0": 0.0, "out1": 0.0, "g_vals1": 0.0},
    "narrow_1x1:mask": {"g_clip": 0.0, "out0": 0.0},
    "narrow_1x257:dense": {"g_clip": 0.848, "out0": 0.143, "g_color0": 0.59},
    "narrow_1x257:rows": {"g_clip": 0.878, "out0": 0.13, "g_vals0": 0.085},
    "narrow_1x257:rows2": {"g_clip": 0.784, "out0": 0.126, "g_vals0": 0.151, "out1": 0.152, "g_vals1": 0.134},
    "narrow_1x257:mask": {"g_clip": 0.916, "out0": 0.088},
    "narrow_300x1:dense": {"g_clip": 0.93, "out0": 0.233, "g_color0": 0.416},
    "narrow_300x1:rows": {"g_clip": 0.847, "out0": 0.326, "g_vals0": 0.554},
    "narrow_300x1:rows2": {"g_clip": 0.785, "out0": 0.343, "g_vals0": 0.687, "out1": 0.332, "g_vals1": 0.625},
    "narrow_300x1:mask": {"g_clip": 0.902, "out0": 0.315},
    "ragged_5x7:dense": {"g_clip": 0.443, "out0": 0.1, "g_color0": 0.097},
    "ragged_5x7:rows": {"g_clip": 0.365, "out0": 0.1, "g_vals0": 0.091},
    "ragged_5x7:rows2": {"g_clip": 0.396, "out0": 0.12, "g_vals0": 0.094, "out1": 0.108, "g_vals1": 0.098},
    "ragged_5x7:mask": {"g_clip": 0.613, "out0": 0.102},
    "ragged_17x15:dense": {"g_clip": 0.43, "out0": 0.145, "g_color0": 0.156},
    "ragged_17x15:rows": {"g_clip": 0.398, "out0": 0.148, "g_vals0": 0.126},
    "ragged_17x15:rows2": {"g_clip": 0.477, "out0": 0.151, "g_vals0": 0.102, "out1": 0.151, "g_vals1": 0.15},
    "ragged_17x15:mask": {"g_clip": 0.476, "out0": 0.147},
    "batch3_shared_17x15:dense": {"g_clip": 0.438, "out0": 0.153, "g_color0": 0.127},
    "batch3_shared_17x15:rows": {"g_clip": 0.409, "out0": 0.161, "g_vals0": 0.087},
    "batch3_shared_17x15:rows2": {"g_clip": 1.149, "out0": 0.164, "g_vals0": 0.126, "out1": 0.151, "g_vals1": 0.12},
    "batch3_shared_17x15:mask": {"g_clip": 0.837, "out0": 0.15},
    "batch3_own_17x15:dense": {"g_clip": 1.241, "out0": 0.149, "g_color0": 0.119},
    "batch3_own_17x15:rows": {"g_clip": 0.536, "out0": 0.146, "g_vals0": 0.119},
    "batch3_own_17x15:rows2": {"g_clip": 0.561, "out0": 0.151, "g_vals0": 0.135, "out1": 0.151, "g_vals1": 0.161},
    "batch3_own_17x15:mask": {"g_clip": 0.45, "out0": 0.146},
    "four_blends_8x8:dense": {"g_clip": 0.331, "out0": 0.077, "g_color0": 0.164},
    "four_blends_8x8:rows": {"g_clip": 0.208, "out0": 0.057, "g_vals0": 0.053},
    "four_blends_8x8:rows2": {"g_clip": 0.313, "out0": 0.029, "g_vals0": 0.047, "out1": 0.119, "g_vals1": 0.117},
    "four_blends_8x8:mask": {"g_clip": 0.214, "out0": 0.041},
    "four_roles_8x8:dense": {"g_clip": 0.235, "out0": 0.034, "g_color0": 0.142},
    "four_roles_8x8:rows": {"g_clip": 0.293, "out0": 0.034, "g_vals0": 0.05},
    "four_roles_8x8:rows2": {"g_clip": 0.245, "out0": 0.061, "g_vals0": 0.034, "out1": 0.104, "g_vals1": 0.095},
    "four_roles_8x8:mask": {"g_clip": 0.365, "out0": 0.038},
    "clamp_window_32x32:dense": {"g_clip": 0.403, "out0": 1.129, "g_color0": 0.844},
    "clamp_window_32x32:rows": {"g_clip": 0.529, "out0": 0.947, "g_vals0": 0.493},
    "clamp_window_32x32:rows2": {"g_clip": 0.211, "out0": 0.886, "g_vals0": 0.681, "out1": 0.0, "g_vals1": 0.859},
    "clamp_window_32x32:mask": {"g_clip": 0.251, "out0": 0.555},
    "slope_45_32x32:dense": {"g_clip": 0.467, "out0": 0.056, "g_color0": 0.255},
    "slope_45_32x32:rows": {"g_clip": 0.415, "out0": 0.077, "g_vals0": 0.053},
    "slope_45_32x32:rows2": {"g_clip": 0.567, "out0": 0.052, "g_vals0": 0.029, "out1": 0.069, "g_vals1": 0.065},
    "slope_45_32x32:mask": {"g_clip": 0.746, "out0": 0.059},
    "topology_16x32:dense": {"g_clip": 0.324, "out0": 0.023, "g_color0": 0.164},
    "topology_16x32:rows": {"g_clip": 0.128, "out0": 0.049, "g_vals0": 0.035},
    "topology_16x32:rows2": {"g_clip": 0.178, "out0": 0.032, "g_vals0": 0.026, "out1": 0.047, "g_vals1": 0.052},
    "topology_16x32:mask": {"g_clip": 0.396, "out0": 0.023},
    "perspective_16x16:dense": {"g_clip": 0.35, "out0": 0.086, "g_color0": 0.089},
    "perspective_16x16:rows": {"g_clip": 0.419, "out0": 0.053, "g_vals0": 0.054},
    "perspective_16x16:rows2": {"g_clip": 0.383, "out0": 0.097, "g_vals0": 0.052, "out1": 0.081, "g_vals1": 0.076},
    "perspective_16x16:mask": {"g_clip": 0.299, "out0": 0.042},
    "rasterised_24x40:dense": {"g_clip": 0.385, "out0": 0.342, "g_color0": 0.655},
    "rasterised_24x40:rows": {"g_clip": 0.698, "out0": 0.498, "g_vals0": 0.491},
    "rasterised_24x40:rows2": {"g_clip": 0.314, "out0": 0.496, "g_vals0": 0.565, "out1": 0.498, "g_vals1": 0.745},
    "rasterised_24x40:mask": {"g_clip": 0.492, "out0": 0.494},
    "checker_16x16:rows_C1_keepNone_none_random": {"g_clip": 0.306, "out0": 0.048, "g_vals0": 0.023},
    "checker_16x16:rows_C1_keep1_own_third": {"g_clip": 1.024, "out0": 0.04, "g_vals0": 0.038},
    "checker_16x16:rows_C4_keepNone_shared_channels": {"g_clip": 0.717, "out0": 0.053, "g_vals0": 0.053},
    "checker_16x16:rows_C4_keep4_own_random_equal": {"g_clip": 0.39, "out0": 0.092, "g_vals0": 0.051},
    "checker_16x16:rows_C16_keep1_short_pixels": {"g_clip": 0.301, "out0": 0.045, "g_vals0": 0.041},
    "checker_16x16:rows_C17_keepNone_own_third_equal": {"g_clip": 0.563, "out0": 0.062, "g_vals0": 0.089},
    "checker_16x16:rows_C17_keep17_none_channels": {"g_clip": 0.76, "out0": 0.087, "g_vals0": 0.083},
    "checker_16x16:rows_C33_keep33_shared_pixels": {"g_clip": 1.284, "out0": 0.094, "g_vals0": 0.077},
    "checker_16x16:rows_C33_keepNone_short_random": {"g_clip": 0.445, "out0": 0.079, "g_vals0": 0.075},
    "checker_16x16:rows_C64_keep64_own_third_equal": {"g_clip": 0.449, "out0": 0.083, "g_vals0": 0.097},
    "checker_16x16:rows_C64_keep1_none_random": {"g_clip": 0.272, "out0": 0.062, "g_vals0": 0.043},
    "checker_16x16:rows_C64_keepNone_shared_channels": {"g_clip": 0.349, "out0": 0.116, "g_vals0": 0.106},
    "checker_16x16:dense_C1_third": {"g_clip": 0.564, "out0": 0.051, "g_color0": 0.064},
    "checker_16x16:dense_C4_channels_equal": {"g_clip": 1.133, "out0": 0.069, "g_color0": 0.089},
    "checker_16x16:dense_C16_pixels": {"g_clip": 1.02, "out0": 0.093, "g_color0": 0.556},
    "checker_16x16:dense_C17_random_equal": {"g_clip": 0.452, "out0": 0.094, "g_color0": 0.261},
    "checker_16x16:dense_C33_channels": {"g_clip": 0.402, "out0": 0.088, "g_color0": 0.157},
    "checker_16x16:dense_C64_third_equal": {"g_clip": 0.318, "out0": 0.104, "g_color0": 0.397},
    "checker_16x16:mask_C1_none_random": {"g_clip": 0.261, "out0": 0.0},
    "checker_16x16:mask_C1_own_pixels": {"g_clip": 1.255, "out0": 0.075},
    "checker_16x16:mask_C3_own_third": {"g_clip": 0.393, "out0": 0.07},
    "checker_16x16:mask_C3_none_alpha": {"g_clip": 0.312, "out0": 0.0},
    "checker_16x16:mask_C16_shared_channels": {"g_clip": 0.403, "out0": 0.066},
    "four_roles_8x8:rows_C1": {"g_clip": 0.31, "out0": 0.077, "g_vals0": 0.033},
    "four_roles_8x8:depth": {"g_clip": 0.101, "out0": 0.006, "g_gb0": 0.067},
    "four_roles_8x8:depth2": {"g_clip": 0.308, "out0": 0.015, "g_gb0": 0.08, "out1": 0.094, "g_vals1": 0.09},
    "checker_16x16:depth": {"g_clip": 0.33, "out0": 0.021, "g_gb0": 0.056},
    "checker_16x16:depth2": {"g_clip": 0.486, "out0": 0.029, "g_gb0": 0.088, "out1": 0.074, "g_vals1": 0.099},
    "batch3_shared_17x15:depth": {"g_clip": 0.582, "out0": 0.874, "g_gb0": 1.818},
    "batch3_shared_17x15:depth2": {"g_clip": 0.477, "out0": 0.634, "g_gb0": 2.276, "out1": 0.163, "g_vals1": 0.162},
    "four_roles_12x12:dense": {"g_clip": 0.265, "out0": 0.065, "g_color0": 0.133},
    "four_roles_12x12:msaa2": {"g_clip": 0.127, "out0": 0.29, "g_vals0": 0.122, "g_null0": 0.146},
    "four_roles_12x12:msaa2_2": {"g_clip": 0.297, "out0": 0.145, "g_vals0": 0.085, "g_null0": 0.109, "out1": 0.132, "g_vals1": 0.153, "g_null1": 0.183},
    "four_roles_12x12:msaa3": {"g_clip": 0.237, "out0": 2.496, "g_vals0": 0.163, "g_null0": 0.153},
    "four_roles_12x12:msaa3_2": {"g_clip": 0.439, "out0": 2.136, "g_vals0": 0.183, "g_null0": 0.125, "out1": 0.163, "g_vals1": 0.169, "g_null1": 0.256},
    "checker_12x12:dense": {"g_clip": 0.557, "out0": 0.13, "g_color0": 0.084},
    "checker_12x12:msaa2": {"g_clip": 1.267, "out0": 0.071, "g_vals0": 0.16, "g_null0": 0.0},
    "checker_12x12:msaa2_2": {"g_clip": 0.252, "out0": 0.09, "g_vals0": 0.122, "g_null0": 0.0, "out1": 0.108, "g_vals1": 0.134, "g_null1": 0.0},
    "checker_12x12:msaa3": {"g_clip": 0.331, "out0": 0.065, "g_vals0": 0.226, "g_null0": 0.412},
    "checker_12x12:msaa3_2": {"g_clip": 0.408, "out0": 0.073, "g_vals0": 0.247, "g_null0": 0.123, "out1": 0.093, "g_vals1": 0.266, "g_null1": 0.129},
    "batch3_shared_18x12:dense": {"g_clip": 0.599, "out0": 0.152, "g_color0": 0.14},
    "batch3_shared_18x12:msaa2": {"g_clip": 0.332, "out0": 0.091, "g_vals0": 0.216, "g_null0": 0.0},
    "batch3_shared_18x12:msaa2_2": {"g_clip": 0.278, "out0": 0.103, "g_vals0": 0.135, "g_null0": 0.0, "out1": 0.131, "g_vals1": 0.211, "g_null1": 0.0},
    "batch3_shared_18x12:msaa3": {"g_clip": 1.254, "out0": 2.484, "g_vals0": 3.332, "g_null0": 0.181},
    "batch3_shared_18x12:msaa3_2": {"g_clip": 0.501, "out0": 2.465, "g_vals0": 3.313, "g_null0": 0.159, "out1": 2.493, "g_vals1": 3.27, "g_null1": 0.133},
}
