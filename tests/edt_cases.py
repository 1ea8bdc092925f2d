"""Seeded inputs of the distance-transform tests (tests/test_edt_cpu.py, tests/test_edt_gpu.py) and their references, computed once per
process (functools.lru_cache) and shared; nothing here needs a GPU.

A case is a batch: ``make_case(name)`` -> dict(src=uint8 [M,H,W] or float32 [N,H,W], thresholds=None or (t_in, t_out)).  Every uint8
case also exists as the float kind: ``as_float(name)`` is float32(src != 0) with thresholds (1, 0), whose channel 0 has the uint8 case's
zero pixels and whose channel 1 has their complement."""
import functools
import zlib

import numpy as np

import edt_ref as R

# H x W; 3x300 is a row longer than a work-group of the row kernel, 255x257 the largest (references from scipy, not brute force)
SHAPES = ((1, 1), (1, 300), (300, 1), (7, 5), (64, 64), (65, 63), (33, 70), (255, 257), (3, 300))
FILLS = ("no_zero", "all_zero", "corner_00", "corner_0w", "corner_h0", "corner_hw", "centre", "zero_row", "zero_column", "checkerboard",
         "random_0.01", "random_0.5", "random_0.99")  # random_p: a pixel is zero with probability p
LONGEST_D2 = 254 ** 2 + 256 ** 2  # 255x257, its single zero pixel in a corner: the longest search


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _fill(kind, h, w, rng):
    """uint8 [H,W]: 0 is a zero pixel, anything else (1 or 255) is not."""
    img = np.full((h, w), 255 if (h + w) % 2 else 1, np.uint8)
    if kind == "all_zero":
        img[:] = 0
    elif kind.startswith("corner_"):
        img[{"0": 0, "h": h - 1}[kind[7]], {"0": 0, "w": w - 1}[kind[8]]] = 0
    elif kind == "centre":
        img[h // 2, w // 2] = 0
    elif kind == "zero_row":
        img[(2 * h) // 3] = 0
    elif kind == "zero_column":
        img[:, w // 3] = 0
    elif kind == "checkerboard":
        yy, xx = np.mgrid[0:h, 0:w]
        img[(yy + xx) % 2 == 0] = 0
    elif kind.startswith("random_"):
        img[rng.random((h, w)) < float(kind[7:])] = 0
    else:
        assert kind == "no_zero", kind
    return img


def _disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def _names():
    names = [f"fills_{h}x{w}" for h, w in SHAPES]
    return names + ["disc_64x64", "two_discs_65x63", "no_zero_first_33x70"]


U8_CASES = tuple(_names())
FLOAT_CASES = ("fractional_nan_65x63", "fractional_half_33x70")
ALL_CASES = U8_CASES + FLOAT_CASES


@functools.lru_cache(maxsize=None)
def make_case(name):
    rng = _rng(name)
    if name.startswith("fills_"):
        h, w = (int(v) for v in name[6:].split("x"))
        return dict(src=np.stack([_fill(k, h, w, rng) for k in FILLS]), thresholds=None)
    if name == "disc_64x64":  # a silhouette (non-zero disc on a zero ground) and its complement
        d = _disc(64, 64, 30, 33, 19)
        return dict(src=np.stack([d, ~d]).astype(np.uint8), thresholds=None)
    if name == "two_discs_65x63":
        # zero discs mirrored about the column x = 31 (every pixel of that column is equally near both: the left one wins, smaller qx)
        # and about the row y = 32 (the upper one wins, smaller qy)
        side = ~(_disc(65, 63, 30, 31 - 14, 9) | _disc(65, 63, 30, 31 + 14, 9))
        stack = ~(_disc(65, 63, 32 - 15, 28, 10) | _disc(65, 63, 32 + 15, 28, 10))
        return dict(src=np.stack([side, stack]).astype(np.uint8), thresholds=None)
    if name == "no_zero_first_33x70":
        second = _fill("random_0.01", 33, 70, rng)
        assert (second == 0).any()
        return dict(src=np.stack([_fill("no_zero", 33, 70, rng), second]), thresholds=None)
    if name == "fractional_nan_65x63":  # the reference's thresholds on a soft mask: the two channels are NOT complements
        m = rng.random((3, 65, 63)).astype(np.float32)
        m[rng.random(m.shape) < 0.3] = 0.0
        m[rng.random(m.shape) < 0.3] = 1.0
        m[0, 11, 7] = np.nan
        m[1, 0, 0] = np.nan
        m[2] = np.where(_disc(65, 63, 33, 30, 20), 1.0, 0.0)
        m[2, 33, 30] = np.nan  # a NaN in the middle of the disc is a zero pixel of BOTH channels
        m[2, 2, 3] = 0.5
        return dict(src=m, thresholds=(1.0, 0.0))
    if name == "fractional_half_33x70":
        m = (rng.random((2, 33, 70)).astype(np.float32) - 0.25) * 2.0  # values outside [0, 1] too
        m[1, 5, 5] = np.nan
        m[0, 0, 69] = np.inf
        m[0, 32, 0] = -np.inf
        return dict(src=m, thresholds=(0.75, 0.25))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def as_float(name):
    case = make_case(name)
    assert case["thresholds"] is None
    return dict(src=(case["src"] != 0).astype(np.float32), thresholds=(1.0, 0.0))


@functools.lru_cache(maxsize=None)
def zeros(name, float_kind=False):
    """bool, True where ZERO: [M,H,W] for a uint8 case, [N,2,H,W] for the float kind."""
    case = as_float(name) if float_kind and name in U8_CASES else make_case(name)
    return R.zero_masks(case["src"], case["thresholds"])


@functools.lru_cache(maxsize=None)
def _image_reference(key):
    h, w, packed = key
    return R.reference(np.unpackbits(np.frombuffer(packed, np.uint8), count=h * w).reshape(h, w).astype(bool))


def image_reference(zero):
    """R.reference of one image, remembered by content (the float kind of a case shares its channel 0 with the uint8 kind)."""
    return _image_reference((zero.shape[0], zero.shape[1], np.packbits(zero).tobytes()))


@functools.lru_cache(maxsize=None)
def expected(name, float_kind=False):
    """(d2 int64, idx int64 or None) with the shape of zeros(name, float_kind); idx is None where brute force did not run."""
    z = zeros(name, float_kind)
    flat = z.reshape(-1, *z.shape[-2:])
    refs = [image_reference(img) for img in flat]
    d2 = np.stack([r[0] for r in refs]).reshape(z.shape)
    idx = None if refs[0][1] is None else np.stack([r[1] for r in refs]).reshape(z.shape)
    return d2, idx
