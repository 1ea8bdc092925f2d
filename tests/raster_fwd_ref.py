"""The rasteriser forward as a DEFINITION, in float64 over all (triangle, pixel) pairs -- no pixel box, no tile, no span, no loop over
candidates.  tests/test_raster_cases_cpu.py holds the box-free C oracle (oracle/raster_ref.c, a3d_ref_rasterize_whole) against it.

A triangle covers a pixel centre (fx, fy) -- the float32 centres the oracle and the kernel evaluate, taken to float64 unchanged -- when,
with q_i = (x_i - fx w_i, y_i - fy w_i):

    a0 = q1x q2y - q1y q2x,  a1 = q2x q0y - q2y q0x,  a2 = q0x q1y - q0y q1x      (homogeneous edge functions)
    s = a0 + a1 + a2 != 0  and  a_k sign(s) > 0 for k = 0, 1, 2
    wn sign(s) > 0  with  wn = sum w_k a_k                                        (in front of the eye)
    -1 <= zn / wn <= 1  with  zn = sum z_k a_k                                    (near / far clip)

and the pixel goes to the covering triangle of least zn / wn, a tie to the lower id.  (a_k == 0 -- the centre exactly on an edge line --
is decided by frag()'s owner rule; here it is always ambiguous, see below.)

Ambiguity.  frag() evaluates the same expressions in float32, u = 2^-24 per rounding:
  * q = fma(-f, w, x): one rounding, q (1 + d), |d| <= u;
  * a product q q': two rounded factors and its own rounding, (1 + d)^3: 3 u to first order;
  * the difference of the two products: one more rounding of the result, at most u (|P1| + |P2|).
  => |a_k(float32) - a_k| <= C_COVER u M_k,  M_k = |q_jx q_ky| + |q_jy q_kx|,  C_COVER = 3 + 1 = 4 (first order; the second-order terms
     and M_k being evaluated on exact q are covered by the factor 1 + 2^-10 below).
  * zn, wn: each term z_k a_k inherits |z_k| times that bound and one rounding of its own, the two additions one rounding each of a
    partial sum bounded by sum |z_k a_k|: d(zn) <= sum |z_k| C_COVER u M_k + C_SUM u sum |z_k a_k|, C_SUM = 1 + 2 = 3; d(wn) alike.
  * zw = zn / wn: d(zw) <= (d(zn) + |zw| d(wn)) / |wn| + u |zw| (the division's own rounding).
A pair is ambiguous in COVERAGE when it is not robustly outside (one a_k beyond its bound on the positive side and one on the negative
side) and some |a_k| <= bound, or |wn| <= d(wn), or | |zw| - 1 | <= d(zw).  A pixel's WINNER is ambiguous when the two nearest depths
lie closer than the sum of their d(zw).

Denormals.  A float32 result below 2^-126 carries an ABSOLUTE error of up to 2^-150 instead of a relative one.  Every bound therefore
also holds an absolute term, TINY = 2^-149: TINY/2 (3 + |q_jx| + |q_ky| + |q_jy| + |q_kx|) in d(a_k) -- a denormal q (error 2^-150) times its
partner, the two products' and the difference's own roundings --, 5 TINY/2 in d(zn) and d(wn) (three products, two sums).  They matter
only next to a vertex whose w is denormal.

Overflow.  Where a product of frag() -- q q', z_k a_k, w_k a_k -- reaches 2^127 in float64 it may be inf in float32, and the pair NaN
(not covered) whatever the definition says: ambiguous, unless robustly outside.

Null triangles.  With two vertices bit-identical in (x, y, w), or a vertex at x = y = w = 0, one edge function is a difference of two
identical products (or of zeros) at EVERY pixel: exactly zero in float32 as in float64, and frag()'s owner rule for a centre on an
edge line (A = y_j w_k - w_j y_k, B = w_j x_k - x_j w_k, both exactly zero here) rejects.  Such a triangle covers nothing, and nothing
about that is ambiguous.

Exact depths.  A triangle with z_k == kappa w_k at all three vertices, kappa zero or a signed power of two, has zn == kappa wn bit for
bit in frag() (multiplying by kappa is exact in every product and sum), so zw == kappa exactly: d(zw) = 0 for it, its clip test and its
ties are decided, not ambiguous.  This is what lets the cases state exact ties, z/w == +-1 and the signed-zero pair.
"""
import numpy as np

U = 2.0 ** -24
C_COVER = 4.0  # 3 (two rounded factors + the product's rounding) + 1 (the difference): derivation above
C_SUM = 3.0    # a term's own product rounding + the two additions of (t0 + t1) + t2
SLACK = 1.0 + 2.0 ** -10
OVER = 2.0 ** 127  # a float32 product of this size may already have overflowed
TINY = 2.0 ** -149  # the spacing of float32 denormals: a result below 2^-126 is rounded to that grid, not to 24 bits (see "Denormals")


def pixel_centres(H, W):
    """The float32 pixel centres of frag()'s callers: fma(2/W, px, 1/W - 1), exactly (float64 holds the product and sum of float32 exactly
    before the single rounding back)."""
    xs, xo = np.float32(2.0) / np.float32(W), np.float32(1.0) / np.float32(W) - np.float32(1.0)
    ys, yo = np.float32(2.0) / np.float32(H), np.float32(1.0) / np.float32(H) - np.float32(1.0)
    fx = (np.float64(xs) * np.arange(W, dtype=np.float64) + np.float64(xo)).astype(np.float32).astype(np.float64)
    fy = (np.float64(ys) * np.arange(H, dtype=np.float64) + np.float64(yo)).astype(np.float32).astype(np.float64)
    return fx, fy


def _exact_kappa(z, w):
    """[F,3] z, w -> [F] bool: z_k == kappa w_k at all three vertices for one kappa in {0} U {+-2^n} (module docstring)."""
    with np.errstate(all="ignore"):
        zero = np.all(z == 0.0, axis=1)
        k = z[:, 0] / w[:, 0]
        m, _ = np.frexp(k)
        pow2 = np.isfinite(k) & (np.abs(m) == 0.5) & np.all(z == k[:, None] * w, axis=1)
    return zero | pow2


def rasterize(clip, tri, H, W, chunk_pairs=1 << 21):
    """clip [V,4] float32 (one image), tri [F,3] -> dict of
    inside [F,H,W] bool   the definition, evaluated in float64
    amb    [F,H,W] bool   coverage of the pair is ambiguous
    winner [H,W] int      covering triangle of least z/w, ties to the lower id; -1 = empty
    zw     [H,W] float64  its depth
    winner_amb [H,W] bool the two nearest depths lie within their bounds of one another
    pixel_amb  [H,W] bool winner_amb, or the coverage of some triangle is ambiguous at the pixel
    Triangles with an index outside [0, V) cover nothing; non-finite input fails every comparison, as NaN does in frag()."""
    clip = np.asarray(clip, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int64)
    V, F = clip.shape[0], tri.shape[0]
    fx, fy = pixel_centres(H, W)
    FX, FY = np.broadcast_to(fx[None, :], (H, W)).reshape(1, -1), np.broadcast_to(fy[:, None], (H, W)).reshape(1, -1)
    HW = H * W
    inside = np.zeros((F, HW), dtype=bool)
    amb = np.zeros((F, HW), dtype=bool)
    best = np.full((2, HW), np.inf)      # the two nearest depths of every pixel ...
    best_e = np.zeros((2, HW))           # ... their d(zw) ...
    best_t = np.full((HW,), -1, dtype=np.int64)  # ... and the nearest one's triangle
    valid = np.all((tri >= 0) & (tri < V), axis=1)
    xyw = clip[np.clip(tri, 0, V - 1)][:, :, [0, 1, 3]]  # [F,3,3]
    null = np.zeros(F, dtype=bool)
    for j, k in ((0, 1), (1, 2), (2, 0)):
        null |= np.all(xyw[:, j] == xyw[:, k], axis=1)
    null |= np.any(np.all(xyw == 0.0, axis=2), axis=1)
    valid &= ~null  # (module docstring: "Null triangles")
    step = max(1, chunk_pairs // HW)
    with np.errstate(all="ignore"):
        for f0 in range(0, F, step):
            sel = np.arange(f0, min(F, f0 + step))
            sel = sel[valid[sel]]
            if sel.size == 0:
                continue
            P = clip[tri[sel]]  # [n,3,4]
            x, y, z, w = (P[:, :, i, None] for i in range(4))  # [n,3,1]
            qx, qy = x - FX[None] * w, y - FY[None] * w  # [n,3,HW]
            a, M = [], []
            for k in range(3):
                j, l = (k + 1) % 3, (k + 2) % 3
                p1, p2 = qx[:, j] * qy[:, l], qy[:, j] * qx[:, l]
                a.append(p1 - p2)
                M.append(np.abs(p1) + np.abs(p2))
            a, M = np.stack(a, 1), np.stack(M, 1)  # [n,3,HW]
            qa = np.stack([np.abs(qx[:, (k + 1) % 3]) + np.abs(qy[:, (k + 2) % 3]) + np.abs(qy[:, (k + 1) % 3]) + np.abs(qx[:, (k + 2) % 3]) for k in range(3)], 1)
            da = C_COVER * U * SLACK * M + 0.5 * TINY * (3.0 + qa)
            s = a.sum(1)
            sg = np.where(s > 0, 1.0, -1.0)[:, None]
            ins = (s != 0) & np.all(a * sg > 0, axis=1)
            robust_out = np.any(a > da, axis=1) & np.any(a < -da, axis=1)
            edge_amb = np.any(np.abs(a) <= da, axis=1) & ~robust_out
            zn, wn = (z * a).sum(1), (w * a).sum(1)
            dzn = (np.abs(z) * da).sum(1) + C_SUM * U * SLACK * np.abs(z * a).sum(1) + 2.5 * TINY
            dwn = (np.abs(w) * da).sum(1) + C_SUM * U * SLACK * np.abs(w * a).sum(1) + 2.5 * TINY
            zw = zn / wn
            dzw = ((dzn + np.abs(zw) * dwn) / np.abs(wn) + U * np.abs(zw)) * SLACK
            exact = _exact_kappa(z[:, :, 0], w[:, :, 0])[:, None]
            dzw = np.where(exact, 0.0, dzw)
            front = wn * sg[:, 0] > 0
            clipped_in = (zw >= -1.0) & (zw <= 1.0)
            ins = ins & front & clipped_in
            # ambiguity of the later tests only where the earlier ones could pass
            could = (ins | edge_amb) & ~robust_out
            eye_amb = could & (np.abs(wn) <= dwn)
            clip_amb = could & (np.abs(np.abs(zw) - 1.0) <= dzw) & ~exact
            pair_amb = (edge_amb & (front | eye_amb) & (clipped_in | clip_amb)) | (eye_amb & (clipped_in | clip_amb)) | clip_amb
            pair_amb |= could & ~np.isfinite(zw) & np.isfinite(s)
            # float32 overflow (docstring: "Overflow"): a product of frag() at or above 2^127 may be inf there and the pair NaN
            over = lambda v: (np.abs(v) >= OVER) & np.isfinite(v)  # (an infinite INPUT is no overflow: inf arithmetic is the same in both)
            big = over(M) | over(z * a) | over(w * a)
            pair_amb |= np.any(big, axis=1) & ~robust_out
            inside[sel], amb[sel] = ins, pair_amb
            for r, t in enumerate(sel):  # ascending ids: a strict '<' leaves a tie with the lower id
                d = np.where(ins[r], zw[r], np.inf)
                e = np.where(ins[r], dzw[r], 0.0)
                first = d < best[0]
                second = ~first & (d < best[1])
                best[1] = np.where(first, best[0], np.where(second, d, best[1]))
                best_e[1] = np.where(first, best_e[0], np.where(second, e, best_e[1]))
                best[0] = np.where(first, d, best[0])
                best_e[0] = np.where(first, e, best_e[0])
                best_t = np.where(first, t, best_t)
    covered = best_t >= 0
    both_exact = (best_e[0] == 0.0) & (best_e[1] == 0.0)
    gap = np.where(np.isfinite(best[1]), best[1], 0.0) - np.where(covered, best[0], 0.0)
    winner_amb = covered & np.isfinite(best[1]) & ~both_exact & (gap <= best_e[0] + best_e[1])
    pixel_amb = winner_amb | amb.any(0)
    return dict(inside=inside.reshape(F, H, W), amb=amb.reshape(F, H, W), winner=best_t.reshape(H, W),
                zw=np.where(covered, best[0], 0.0).reshape(H, W), winner_amb=winner_amb.reshape(H, W), pixel_amb=pixel_amb.reshape(H, W))
