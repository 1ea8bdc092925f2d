"""The Radiance .hdr codec (3danimals_amd/hdrio.py) on bytes written by hand: known answers, both scanline encodings, the truncation
bound of a write / read round trip, and what is refused."""
import importlib

import numpy as np
import pytest

HEAD = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"


@pytest.fixture(scope="module")
def hdrio():
    return importlib.import_module("3danimals_amd.hdrio")


def _flat(pixels, width, height=1, head=HEAD):
    return head + b"-Y %d +X %d\n" % (height, width) + bytes(v for p in pixels for v in p)


def test_known_pixels_decode_by_the_rgbe_c_convention(hdrio):
    img = hdrio.read_hdr_bytes(_flat([(128, 64, 32, 129), (200, 100, 50, 0), (255, 0, 1, 136), (0, 0, 0, 0)], 4))
    assert img.dtype == np.float32 and img.shape == (1, 4, 3)
    assert img[0, 0].tolist() == [1.0, 0.5, 0.25]
    assert img[0, 1].tolist() == [0.0, 0.0, 0.0]  # e == 0 is black whatever the mantissas
    assert img[0, 2].tolist() == [255.0, 0.0, 1.0]
    assert img[0, 3].tolist() == [0.0, 0.0, 0.0]
    assert hdrio.read_hdr_bytes(_flat([(128, 64, 32, 129)], 1, head=b"#?RGBE\nEXPOSURE=1.0\nFORMAT=32-bit_rle_rgbe\n\n"))[0, 0].tolist() == [1.0, 0.5, 0.25]


def test_flat_and_rle_scanlines_decode_to_the_same_array(hdrio):
    width = 10
    r = [7, 7, 7, 7, 7, 9, 10, 11, 12, 12]
    g = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    b = [0] * 10
    e = [130] * 10
    flat = _flat(list(zip(r, g, b, e)), width)
    rle = HEAD + b"-Y 1 +X 10\n" + bytes([2, 2, 0, 10]) \
        + bytes([128 + 5, 7, 5, 9, 10, 11, 12, 12]) \
        + bytes([10] + g) \
        + bytes([128 + 10, 0]) \
        + bytes([128 + 4, 130, 128 + 6, 130])
    a, c = hdrio.read_hdr_bytes(flat), hdrio.read_hdr_bytes(rle)
    assert a.shape == (1, width, 3) and np.array_equal(a, c)
    assert a[0, 0].tolist() == [7 / 64, 1 / 64, 0.0]
    # the writer's own two encodings of one picture
    img = np.random.default_rng(0).random((3, 40, 3)).astype(np.float32)
    img[1, 5:30] = 0.25
    packed, plain = hdrio.write_hdr_bytes(img), hdrio.write_hdr_bytes(img, rle=False)
    assert len(packed) != len(plain) and plain[-4 * 40 * 3:] == hdrio.encode_rgbe(img).tobytes()
    assert np.array_equal(hdrio.read_hdr_bytes(packed), hdrio.read_hdr_bytes(plain))


@pytest.mark.parametrize("shape", [(1, 1), (2, 7), (3, 8), (5, 33), (4, 300)])
def test_write_then_read_is_within_the_truncation_bound(hdrio, shape, tmp_path):
    """Every channel comes back within max(r, g, b) / 128 below its value: the quantum is 2^(e-8) and max >= 2^(e-1)."""
    rng = np.random.default_rng(shape[1])
    img = (rng.random(shape + (3,)) * np.exp(rng.uniform(-20, 20, shape + (1,)))).astype(np.float32)
    img[0, 0] = (0.0, 0.0, 0.0)
    img[-1, -1] = (1e-33, 0.0, 0.0)  # below 1e-32: written as black
    fn = str(tmp_path / "a.hdr")
    hdrio.write_hdr(fn, img)
    back = hdrio.read_hdr(fn)
    assert back.shape == img.shape and back.dtype == np.float32
    v = img.max(axis=-1, keepdims=True).astype(np.float64)
    bound = np.where(v < 1e-32, v, v / 128)  # (a pixel below the writer's 1e-32 threshold is black: it loses all of itself)
    err = img.astype(np.float64) - back
    assert (err >= 0).all() and (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert back[0, 0].tolist() == [0.0, 0.0, 0.0] and back[-1, -1].tolist() == [0.0, 0.0, 0.0]
    # W below 8 takes the flat path, from 8 on the run-length encoded one
    data = open(fn, "rb").read()
    body = data[data.index(b"+X") :].split(b"\n", 1)[1]
    if shape[1] < 8:
        assert len(body) == 4 * shape[0] * shape[1]
    else:
        assert body[:4] == bytes([2, 2, shape[1] >> 8, shape[1] & 255])


def test_out_of_range_input_is_clamped(hdrio):
    img = np.array([[[-1.0, 0.5, 0.25], [np.nan, 2.0, 1.0], [np.inf, 1.0, 0.0], [3e38, 0.0, 0.0]]], dtype=np.float32)
    back = hdrio.read_hdr_bytes(hdrio.write_hdr_bytes(img))
    assert back[0, 0].tolist() == [0.0, 0.5, 0.25] and back[0, 1].tolist() == [0.0, 2.0, 1.0]
    assert back[0, 2, 0] == np.float32(hdrio.RGBE_MAX) and back[0, 3, 0] == np.float32(hdrio.RGBE_MAX) and np.isfinite(back).all()
    with pytest.raises(ValueError):
        hdrio.write_hdr_bytes(np.zeros((2, 2, 4), dtype=np.float32))


def test_malformed_files_raise_value_error(hdrio):
    px = [(128, 64, 32, 129)] * 8
    good = _flat(px, 8)
    assert hdrio.read_hdr_bytes(good).shape == (1, 8, 3)
    bad = {
        "magic": good.replace(b"#?RADIANCE", b"#?RADIANT!"),
        "format": good.replace(b"32-bit_rle_rgbe", b"32-bit_rle_xyze"),
        "no format": good.replace(b"FORMAT=32-bit_rle_rgbe\n", b""),
        "no blank line": good.replace(b"\n\n", b"\n"),
        "orientation +Y": good.replace(b"-Y 1 +X 8", b"+Y 1 +X 8"),
        "orientation X first": good.replace(b"-Y 1 +X 8", b"+X 8 -Y 1"),
        "short": good[:-3],
        "old-style run": _flat([(128, 64, 32, 129), (1, 1, 1, 6)] + px[:6], 8),
        "run overruns": HEAD + b"-Y 1 +X 8\n" + bytes([2, 2, 0, 8, 128 + 9, 5]),
        "literal overruns": HEAD + b"-Y 1 +X 8\n" + bytes([2, 2, 0, 8, 6, 1, 2, 3, 4, 5, 6, 3, 1, 2, 3]),
        "rle width": HEAD + b"-Y 1 +X 8\n" + bytes([2, 2, 0, 9] + [128 + 9, 5] * 4),
        "rle cut": HEAD + b"-Y 1 +X 8\n" + bytes([2, 2, 0, 8, 128 + 8, 5, 128 + 8]),
    }
    for what, data in bad.items():
        with pytest.raises(ValueError):
            hdrio.read_hdr_bytes(data)
            pytest.fail(what)
