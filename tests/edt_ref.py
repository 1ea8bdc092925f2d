"""The exact Euclidean distance transform restated in numpy (include/a3d_edt.h's specification), for tests/test_edt_cpu.py and
tests/test_edt_gpu.py.  ``zero`` is always a bool array that is True where a pixel is ZERO.

brute(): every pixel against every zero pixel in int64, argmin over the zero pixels in row-major order (the tie rule: the smallest flat
index among equally near ones).  Quadratic, so kept to images of at most BRUTE_PIXELS pixels; above that the yardstick for d2 is
np.rint(scipy_edt ** 2), which agreed with brute() exactly on every shape both were run on (tests/test_edt_cpu.py holds that)."""
import numpy as np

BRUTE_PIXELS = 70 * 70


def none_value(h, w):
    """d2 of an image without a zero pixel: strictly above (h - 1)^2 + (w - 1)^2."""
    return h * h + w * w


def brute(zero):
    """zero bool [H,W] -> (d2 int64 [H,W], idx int64 [H,W])."""
    h, w = zero.shape
    qy, qx = np.nonzero(zero)  # row-major order
    if qy.size == 0:
        return np.full((h, w), none_value(h, w), np.int64), np.full((h, w), -1, np.int64)
    qy, qx = qy.astype(np.int64), qx.astype(np.int64)
    d2 = np.empty((h, w), np.int64)
    idx = np.empty((h, w), np.int64)
    px = np.arange(w, dtype=np.int64)
    for y in range(h):
        all_d2 = (y - qy)[None, :] ** 2 + (px[:, None] - qx[None, :]) ** 2  # [W, Z]
        k = np.argmin(all_d2, axis=1)  # the first minimum: the smallest (qy, qx)
        d2[y] = all_d2[px, k]
        idx[y] = qy[k] * w + qx[k]
    return d2, idx


def scipy_d2(zero):
    """np.rint(edt ** 2) as int64; an image without a zero pixel gets none_value (scipy's own answer there is arbitrary)."""
    from scipy.ndimage import distance_transform_edt

    h, w = zero.shape
    if not zero.any():
        return np.full((h, w), none_value(h, w), np.int64)
    return np.rint(distance_transform_edt(~zero) ** 2).astype(np.int64)


def reference(zero):
    """(d2 int64, idx int64 or None): brute force up to BRUTE_PIXELS pixels, scipy's squared distances (no idx) above."""
    if zero.size <= BRUTE_PIXELS:
        return brute(zero)
    return scipy_d2(zero), None


def dist_from_d2(d2, scale=1.0):
    """One float64 root, one float64 divide, one rounding to float32."""
    return (np.sqrt(d2.astype(np.float64)) / np.float64(scale)).astype(np.float32)


def zero_masks(src, thresholds=None):
    """The ZERO predicate of a source as the op reads it: uint8 / bool [M,H,W] -> [M,H,W]; float32 [N,H,W] with (t_in, t_out) ->
    [N,2,H,W] (channel 0 is non-zero where m >= t_in, channel 1 where m <= t_out; a NaN is zero in both)."""
    if thresholds is None:
        return src == 0
    t_in, t_out = (np.float32(t) for t in thresholds)
    with np.errstate(invalid="ignore"):
        return np.stack([~(src >= t_in), ~(src <= t_out)], axis=1)


def idx_is_a_nearest_zero(zero, d2, idx):
    """For images too large for brute(): the pixel at idx is zero and lies exactly d2 away (idx = -1 / none_value without a zero)."""
    h, w = zero.shape
    if not zero.any():
        return bool((idx == -1).all() and (d2 == none_value(h, w)).all())
    if idx.min() < 0 or idx.max() >= h * w:
        return False
    qy, qx = idx // w, idx % w
    py, px = np.mgrid[0:h, 0:w]
    return bool(zero[qy, qx].all() and ((py - qy) ** 2 + (px - qx) ** 2 == d2).all())
