"""Float64 restatement of the articulation glue, written from the reference's lines (InstancePredictorBase.py:337-382, 391-432, 435-511;
InstancePredictorFauna.py:102-147, 149-213, 229-230; AnimalModel.py:313-314) in plain numpy; it never calls the module under test.

Beside each value stands its MAGNITUDE on the scheme of tests/skin_ref.py (the same expression with absolute values and additions for
subtractions); errors are measured in units of 2^-24 x magnitude.  What is not a plain absolute-value restatement:

  * x / w carries w's own term: mag(x / w) = mag(x) / |w| + |x| mag(w) / w^2.
  * The sampled features are judged at the coordinates the op itself returned (bones_pos_in[..., :2] promoted to float64): a last-bit
    difference of the projection is judged once, in bones_pos_in, and not again through the image's slope.  A sample's magnitude is
    sum |weight * tap| plus the spread (max - min) of its taps times the magnitude of the pixel coordinate ((|x| + 1) size + 1) / 2 --
    the float32 spacing of the pixel coordinate, which moves the weights.  A float32 pixel coordinate may fall on the other side of an
    integer than the float64 one: the taps of both floors count for the spread, and in the gradient every pixel either floor taps
    carries |g| x that coordinate magnitude (the weights there are within that much of 0).  A pixel no bone can tap has magnitude 0
    and must be exactly 0.
  * tanh: angles = S tanh(u), u = m x has magnitude |S| (|t| + (1 - t^2) |u|); its gradient up S m (1 - t^2) carries the cancellation
    of 1 - t t, |up S m| (1 + t^2), and the slope of 1 - t^2 in u, |up S m| 2 |t| (1 - t^2) |u|.  Where S is 0 every magnitude is 0.

MEASURED holds, per case and quantity, what the torch float32 statements of 3danimals_amd/articulation.py reach on the CPU against this
restatement; tests/test_articulation_cpu.py measures it afresh and compares.  The kernels' bound is 4 x that figure in these units plus
4 ulp of the float64 value (``bad_elements``); nothing else enters it.
"""
import math

import numpy as np
import torch

from deriv_ref import EPS  # noqa: F401  (2^-24: the same unit as the derivative and skinning suites)

FACTOR, FLOOR_ULP = 4.0, 4.0
NEAR = 2.0 ** -20  # how far (x its magnitude) a float32 pixel coordinate is taken to stray from the float64 one: 16 roundings


def _np(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- descriptors
def _xfm(M, p, pm):
    """rows of M [N,4,4] applied to (p, 1), p [N,K,3] -> value and magnitude [N,K,4]."""
    val = np.einsum("nji,nki->nkj", M[:, :, :3], p) + M[:, None, :, 3]
    mag = np.einsum("nji,nki->nkj", np.abs(M[:, :, :3]), pm) + np.abs(M[:, None, :, 3])
    return val, mag


def _ratio(x, xm, w, wm):
    return x / w, xm / np.abs(w) + np.abs(x) * wm / (w * w)


def positions(bones, mvp, w2c, z_offset, spatial_scale):
    """bones_pos_in [N,K,9] and its magnitude, float64."""
    b, M, V = _np(bones), _np(mvp), _np(w2c)
    N, K = M.shape[0], b.shape[1]
    b = np.broadcast_to(b, (N,) + b.shape[1:])
    val, mag = np.empty((N, K, 9)), np.empty((N, K, 9))
    with np.errstate(all="ignore"):
        mid, mid_m = (b[:, :, 0] + b[:, :, 1]) / 2, (np.abs(b[:, :, 0]) + np.abs(b[:, :, 1])) / 2
        clip, clip_m = _xfm(M, mid, mid_m)
        val[..., :2], mag[..., :2] = _ratio(clip[..., :2], clip_m[..., :2], clip[..., 3:], clip_m[..., 3:])
        for e in range(2):
            cam, cam_m = _xfm(V, b[:, :, e], np.abs(b[:, :, e]))
            v, m = _ratio(cam[..., :3], cam_m[..., :3], cam[..., 3:], cam_m[..., 3:])
            v[..., 2] += z_offset
            m[..., 2] += abs(z_offset)
            val[..., 2 + 3 * e:5 + 3 * e], mag[..., 2 + 3 * e:5 + 3 * e] = v / spatial_scale * 2, m / abs(spatial_scale) * 2
    idx = (np.arange(K) + 0.5) / K * 2
    val[..., 8], mag[..., 8] = idx - 1, idx + 1
    return val, mag


def _pixel(c, size):
    return ((c + 1) * size - 1) / 2, ((abs(c) + 1) * size + 1) / 2


def taps(x, y, h, w):
    """The alive taps [(row, column, weight)] of grid_sample(bilinear, zeros, align_corners=False) at (x, y), in the order (y0,x0)
    (y0,x1) (y1,x0) (y1,x1); none when a coordinate is not finite."""
    if not (math.isfinite(x) and math.isfinite(y)):
        return []
    (ix, _), (iy, _) = _pixel(x, w), _pixel(y, h)
    x0, y0 = math.floor(ix), math.floor(iy)
    out = []
    for yy, wy in ((y0, y0 + 1 - iy), (y0 + 1, iy - y0)):
        for xx, wx in ((x0, x0 + 1 - ix), (x0 + 1, ix - x0)):
            if 0 <= xx <= w - 1 and 0 <= yy <= h - 1:
                out.append((int(yy), int(xx), wx * wy))
    return out


def near_pixels(x, y, h, w):
    """(pixels [(row, column)] inside the image that a float32 evaluation of the pixel coordinate may tap, how many it may tap in all,
    the coordinate's magnitude)."""
    if not (math.isfinite(x) and math.isfinite(y)):
        return [], 0, 0.0
    (ix, mx), (iy, my) = _pixel(x, w), _pixel(y, h)
    cols = sorted({f + d for c, m in ((ix, mx),) for f in (math.floor(c - NEAR * m), math.floor(c + NEAR * m)) for d in (0, 1)})
    rows = sorted({f + d for c, m in ((iy, my),) for f in (math.floor(c - NEAR * m), math.floor(c + NEAR * m)) for d in (0, 1)})
    inside = [(int(r), int(c)) for r in rows if 0 <= r <= h - 1 for c in cols if 0 <= c <= w - 1]
    return inside, len(rows) * len(cols), mx + my


def sample(patch, xy):
    """patch [N,C,h,w], xy [N,K,2] (float64: the coordinates the op returned) -> value and magnitude [N,K,C]."""
    P, xy = _np(patch), _np(xy)
    N, C, h, w = P.shape
    K = xy.shape[1]
    val, mag = np.zeros((N, K, C)), np.zeros((N, K, C))
    for n in range(N):
        for k in range(K):
            for r, c, wt in taps(xy[n, k, 0], xy[n, k, 1], h, w):
                val[n, k] += wt * P[n, :, r, c]
                mag[n, k] += np.abs(wt * P[n, :, r, c])
            inside, total, coord = near_pixels(xy[n, k, 0], xy[n, k, 1], h, w)
            if inside:
                vals = np.stack([P[n, :, r, c] for r, c in inside] + ([np.zeros(C)] if len(inside) < total else []))
                mag[n, k] += (vals.max(0) - vals.min(0)) * coord
    return val, mag


def scatter(g, xy, shape):
    """The adjoint of ``sample``: g [N,K,C], xy [N,K,2] -> value and magnitude [N,C,h,w]."""
    g, xy = _np(g), _np(xy)
    N, C, h, w = shape
    val, mag = np.zeros(shape), np.zeros(shape)
    for n in range(N):
        for k in range(xy.shape[1]):
            for r, c, wt in taps(xy[n, k, 0], xy[n, k, 1], h, w):
                val[n, :, r, c] += wt * g[n, k]
                mag[n, :, r, c] += np.abs(wt * g[n, k])
            inside, _, coord = near_pixels(xy[n, k, 0], xy[n, k, 1], h, w)
            for r, c in inside:
                mag[n, :, r, c] += np.abs(g[n, k]) * coord
    return val, mag


def evaluate_desc(c, xy):
    """Everything a descriptor case produces, key -> (value, magnitude): pos; with features also feat, and with the case's upstream
    gradient g_feat / g_patch (whichever the mode feeds).  ``xy``: bones_pos_in[..., :2] as the op under test returned it."""
    from articulation_cases import SPATIAL_SCALE, Z_OFFSET

    res = {"pos": positions(c["bones"], c["mvp"], c["w2c"], Z_OFFSET, SPATIAL_SCALE)}
    if c["feat"] is None or c["patch"] is None:
        return res
    N, K = c["mvp"].shape[0], c["bones"].shape[1]
    f, D = _np(c["feat"]), c["feat"].shape[1]
    parts, g = [], (None if c.get("g") is None else _np(c["g"]))
    if "global" in c["mode"]:
        rep = np.broadcast_to(f[:, None], (N, K, D))
        parts.append((rep, np.abs(rep)))
        if g is not None:
            res["g_feat"] = (g[..., :D].sum(1), np.abs(g[..., :D]).sum(1))
    if "sample" in c["mode"]:
        parts.append(sample(c["patch"], xy))
        if g is not None:
            res["g_patch"] = scatter(g[..., (D if "global" in c["mode"] else 0):], xy, tuple(c["patch"].shape))
    res["feat"] = (np.concatenate([p[0] for p in parts], -1), np.concatenate([p[1] for p in parts], -1))
    return res


# ---------------------------------------------------------------------------------------------------------------- limits
def _blend(a, bones, axes, c):
    """tmp_mask = zeros; tmp_mask[:, bones, axes] = 1; a = tmp_mask * (a * c) + (1 - tmp_mask) * a"""
    mask = np.zeros_like(a)
    for ax in axes:
        if len(bones):
            mask[..., list(bones), ax] = 1
    return mask * (a * c) + (1 - mask) * a


def _zero(a, bones, axes=(0, 1, 2), values=None):
    """tmp_mask = ones; tmp_mask[:, bones, axis] = value (0 unless given); a = a * tmp_mask"""
    mask = np.ones_like(a)
    for ax in axes:
        mask[..., list(bones), ax] = 0 if values is None else values[ax]
    return a * mask


def _legs(a, cfg):
    legs = cfg["num_body_bones"] + np.arange(cfg["num_leg_bones"] * cfg["num_legs"])
    return _blend(_blend(a, legs, (2,), 0.3), legs, (1,), 0.3)


def limits_passes(kind, cfg, a, tanh=np.tanh):
    """The reference's statements on a [...,K,3] = output_multiplier * x, float64.  ``tanh`` = identity on a table of ones gives the
    factor of every (bone, axis)."""
    nb = cfg["num_body_bones"]
    roots = [nb // 2 - 1, nb - 1]
    if kind == "base":  # InstancePredictorBase.py:437-511
        if cfg.get("static_root_bones"):
            a = _zero(a, roots)
        a = tanh(a)
        if cfg.get("constrain_legs"):
            a = _legs(a, cfg)
            if cfg.get("use_fauna_constraints"):
                top, bottom = [10, 13, 16, 19], [8, 9, 11, 12, 14, 15, 17, 18]
                a = _blend(a, top, (1, 2), 0.05)
                a = _blend(a, top, (0,), 0.75)
                a = _zero(a, bottom, values={0: 0.3, 1: 0, 2: 0})
                a = _blend(a, list(range(8)), (2,), 0.1)
        if cfg.get("extra_constraints"):
            half = cfg["num_leg_bones"] * cfg["num_legs"] // 2
            legs = [nb + i for i in range(half)] + [nb + half + i for i in range(half)]
            a = _blend(_blend(a, legs, (2,), 0.3), legs, (1,), 0.3)
            a = _blend(a, [8, 11, 14, 17], (1, 2), 0.05)
            a = _zero(a, [9, 10, 12, 13, 15, 16, 18, 19], (1, 2))
        return a * cfg["max_arti_angle"] / 180 * np.pi
    assert kind == "fauna", kind  # InstancePredictorFauna.py:229-230, 187-213, 149-185
    a = tanh(a)
    if cfg.get("static_root_bones"):
        a = _zero(a, roots)
    start, it = cfg["iter_leg_rotation_start"], cfg["total_iter"]
    if it <= start:
        a = _legs(a, cfg)
    if start > 0 and it > start and cfg["forbid_leg_rotate"]:
        if cfg["small_leg_angle"]:
            a = _blend(a, [8, 11, 14, 17], (1, 2), 0.05)
        a = _zero(a, [9, 10, 12, 13, 15, 16, 18, 19], (1, 2))
    a = a * cfg["max_arti_angle"] / 180 * np.pi
    mult = cfg["reg_body_rotate_mult"] * 180 * 1.0 / (cfg["max_arti_angle"] * np.pi)
    return _blend(a, list(range(8)), (2,), mult)


def factors(kind, cfg, K):
    """[K,3] float64: what the passes multiply each (bone, axis) by."""
    return limits_passes(kind, cfg, np.ones((K, 3)), tanh=lambda v: v)


def evaluate_limits(c, g_angles=True, g_reg=True):
    """key -> (value, magnitude) for angles, reg and g_x (the gradient of sum(angles * g_angles) + reg * g_reg; either may be off)."""
    x, m = _np(c["x"]), c["cfg"]["output_multiplier"]
    S = factors(c["kind"], c["cfg"], x.shape[-2])
    u = m * x
    t = np.tanh(u)
    angles = limits_passes(c["kind"], c["cfg"], u)
    sech2 = 1 - t * t
    a_mag = np.abs(S) * (np.abs(t) + sech2 * np.abs(u))
    n = x.size
    res = {"angles": (angles, a_mag), "reg": (np.mean(angles ** 2), np.mean(np.abs(angles) * (np.abs(angles) + 2 * a_mag)))}
    ga = _np(c["g_angles"]) if g_angles else np.zeros_like(x)
    gr = float(c["g_reg"]) if g_reg else 0.0
    up = ga + gr * 2 * angles / n
    up_mag = np.abs(ga) + abs(gr) * 2 * (np.abs(angles) + a_mag) / n
    sm = np.abs(S * m)
    res["g_x"] = (up * S * m * sech2, sm * (up_mag * sech2 + np.abs(up) * (2 * np.abs(t) * sech2 * np.abs(u) + 1 + t * t)))
    return res


# ---------------------------------------------------------------------------------------------------------------- comparison
def _same_non_finite(got, ref):
    """Boolean array: where ref is not finite, got is the same kind of non-finite value (a NaN, or the infinity of that sign)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(ref), np.isnan(got), got == ref)


def units(got, ref, mag):
    """max |got - ref| / (2^-24 magnitude) over the finite elements of ref; the others must be the same non-finite value in got, and an
    element without a magnitude (nothing feeds it) must be exactly zero."""
    got, ref, mag = _np(got), np.asarray(ref, dtype=np.float64), np.asarray(mag, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert _same_non_finite(got, ref)[~fin].all(), "a non-finite element differs"
    dead = fin & (mag == 0)
    assert (got[dead] == 0).all(), "an element nothing feeds is not zero"
    live = fin & ~dead
    if not live.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        u = np.abs(got - ref)[live] / (EPS * mag[live])
    return float(np.where(np.isnan(u), np.inf, u).max())


def bad_elements(got, ref, mag, figure):
    """Indices where got misses the kernels' bound: |got - ref| > 2^-24 (4 x figure x magnitude + 4 |ref|) on a finite element of ref
    (a non-finite got violates), another value than ref's on a non-finite one."""
    got, ref, mag = _np(got), np.asarray(ref, dtype=np.float64), np.asarray(mag, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - ref) <= EPS * (FACTOR * figure * np.where(fin, mag, 0.0) + FLOOR_ULP * np.abs(ref))
    return np.argwhere(~np.where(fin, ok, _same_non_finite(got, ref)))


def figure(name, key):
    return MEASURED[name][key]


# what the torch float32 statements reach against the restatement, in units of 2^-24 x magnitude (maximum over the elements; CPU; third
# decimal rounded up): written by tests/test_articulation_cpu.py::measure_all, asserted by test_measured_table_is_current
MEASURED = {
    "desc/n1_k1_c1_d1_1x1_nchw": {"pos": 1.162, "g_feat": 0.0, "g_patch": 0.294, "feat": 0.285},
    "desc/n3_k5_cbelow_dabove_3x5_nhwc_shared": {"pos": 1.179, "g_feat": 1.793, "g_patch": 0.403, "feat": 0.481},
    "desc/n3_k20_cat_dbelow_32x32_nchw": {"pos": 1.283, "g_feat": 0.879, "g_patch": 0.5, "feat": 0.523},
    "desc/n3_k64_cabove_dat_3x5_slice": {"pos": 1.238, "g_feat": 1.06, "g_patch": 0.295, "feat": 0.815},
    "desc/n1_k20_cabove_d1_32x32_nhwc": {"pos": 0.925, "g_feat": 0.399, "g_patch": 0.308, "feat": 0.423},
    "desc/n3_k5_c1_dabove_1x1_slice_shared": {"pos": 1.092, "g_feat": 1.66, "g_patch": 0.323, "feat": 0.351},
    "desc/n3_k5_sample_cat_3x5_nchw_shared": {"pos": 1.109, "g_patch": 0.719, "feat": 0.712},
    "desc/n3_k64_sample_c2above_32x32_nhwc": {"pos": 1.318, "g_patch": 0.64, "feat": 0.644},
    "desc/n3_k20_global_dabove_3x5_nchw": {"pos": 1.297, "g_feat": 0.976, "feat": 0.0},
    "desc/n3_k20_nofeat_shared": {"pos": 1.365},
    "desc/hand_k20_c5_d3_4x8_nchw": {"pos": 0.914, "g_feat": 0.2, "g_patch": 0.257, "feat": 0.175},
    "desc/hand_k20_cabove_d3_4x8_nhwc": {"pos": 1.199, "g_feat": 0.58, "g_patch": 0.392, "feat": 0.592},
    "desc/hand_k20_c5_d3_4x8_slice": {"pos": 1.233, "g_patch": 0.397, "feat": 0.375},
    "limits/k1_n1_plain": {"angles": 0.264, "reg": 0.23, "g_x": 0.429},
    "limits/k8_n3_bird": {"angles": 1.453, "reg": 0.06, "g_x": 1.34},
    "limits/k20_n3_magicpony": {"angles": 2.669, "reg": 0.732, "g_x": 1.612},
    "limits/k20_n1_ponymation": {"angles": 3.446, "reg": 0.237, "g_x": 1.293},
    "limits/k20_n3_fauna_constraints": {"angles": 2.783, "reg": 0.181, "g_x": 1.48},
    "limits/k20_n1201_fauna_late": {"angles": 3.325, "reg": 0.599, "g_x": 2.285},
    "limits/k20_n3_fauna_early": {"angles": 2.723, "reg": 0.473, "g_x": 1.365},
    "golden_bones/base_global_shared": {"pos": 1.164, "feat": 0.0},
    "golden_bones/base_sample_batched": {"pos": 1.259, "feat": 0.377},
    "golden_bones/base_sample+global_shared": {"pos": 1.174, "feat": 0.54},
    "golden_bones/base_sample+global_batched": {"pos": 1.181, "feat": 0.634},
    "golden_bones/fauna_sample+global_batched": {"pos": 0.997, "feat": 0.514},
    "golden_bones/fauna_sample_shared": {"pos": 1.117, "feat": 0.514},
    "golden_bones/refine_sample+global_batched": {"pos": 1.259, "feat": 0.537},
    "golden_limits/magicpony": {"angles": 2.37},
    "golden_limits/ponymation": {"angles": 4.166},
    "golden_limits/bird": {"angles": 1.794},
    "golden_limits/fauna_constraints": {"angles": 2.815},
    "golden_limits/fauna_early_forbid0_small0": {"angles": 2.884},
    "golden_limits/fauna_early_forbid0_small1": {"angles": 2.312},
    "golden_limits/fauna_early_forbid1_small0": {"angles": 2.354},
    "golden_limits/fauna_early_forbid1_small1": {"angles": 2.942},
    "golden_limits/fauna_late_forbid0_small0": {"angles": 1.902},
    "golden_limits/fauna_late_forbid0_small1": {"angles": 1.874},
    "golden_limits/fauna_late_forbid1_small0": {"angles": 2.17},
    "golden_limits/fauna_late_forbid1_small1": {"angles": 1.857},
}
