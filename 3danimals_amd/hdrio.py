"""Radiance .hdr (RGBE) pictures in plain numpy -- what light.load_env / save_env_map need of the reference's imageio.

This is the project's specification of the format, written from the published description of Radiance pictures and Greg Ward's public
rgbe.c, and UNPINNED against imageio (which is not a dependency): a file one of them writes has not been compared with what the other
reads.

File: a first line ``#?RADIANCE`` or ``#?RGBE``, header lines up to a blank line of which one must be ``FORMAT=32-bit_rle_rgbe``, a
resolution line ``-Y H +X W`` (rows top to bottom, columns left to right; every other orientation raises), then H scanlines.  A
scanline is flat (W pixels of 4 bytes r, g, b, e) or new-style run-length encoded: the bytes 2, 2, W >> 8, W & 255, then for each of the
four channels in turn codes ``n > 128, v`` (v repeated n - 128 times) or ``n <= 128`` followed by n literal bytes, until W bytes.
Old-style run-length encoding (pixels 1, 1, 1, n) raises.

Pixel: e == 0 is black, otherwise channel = mantissa * 2^(e - 136) -- the rgbe.c convention (no half added to the mantissa).
Writing: v = max(r, g, b); v < 1e-32 gives four zero bytes, otherwise v = m 2^x by frexp (0.5 <= m < 1), each mantissa is
trunc(channel * m * 256 / v) and e = x + 128, so a channel comes back within 2^(x - 8) <= v / 128 below its value.  Scanlines are
run-length encoded when 8 <= W < 32768 and flat otherwise.  Input is CLAMPED, not refused: negative values and NaN are written as 0,
values above the largest pixel (255 * 2^119, +inf included) as that one.
"""
import re

import numpy as np

RGBE_MAX = 255.0 * 2.0 ** 119  # mantissa 255 at exponent byte 255
_MIN_RUN = 4


def _rle_ok(width):
    return 8 <= width < 32768


def decode_rgbe(rgbe):
    """uint8 [..., 4] -> float32 [..., 3]."""
    rgbe = np.asarray(rgbe, dtype=np.uint8)
    e = rgbe[..., 3:4].astype(np.int32)
    scale = np.where(e == 0, np.float32(0), np.ldexp(np.float32(1), e - 136)).astype(np.float32)
    return rgbe[..., :3].astype(np.float32) * scale


def encode_rgbe(img):
    """float [..., 3] -> uint8 [..., 4] (clamped: see the module docstring)."""
    img = np.asarray(img, dtype=np.float32)
    if img.shape[-1] != 3:
        raise ValueError(f"hdrio: an image must have 3 channels, got shape {list(img.shape)}")
    img = np.clip(np.nan_to_num(img, nan=0.0, posinf=RGBE_MAX, neginf=0.0), 0.0, RGBE_MAX).astype(np.float64)
    v = img.max(axis=-1)
    _, x = np.frexp(v)
    live = v >= 1e-32
    out = np.zeros(img.shape[:-1] + (4,), dtype=np.uint8)
    # (m * 256 / v = 2^(8 - x): the scaling is exact, the truncation the only rounding)
    out[..., :3] = np.where(live[..., None], np.trunc(np.ldexp(img, (8 - x)[..., None])), 0.0).astype(np.uint8)
    out[..., 3] = np.where(live, x + 128, 0).astype(np.uint8)
    return out


def _read_scanline_rle(buf, pos, width, fn):
    row = np.empty((4, width), dtype=np.uint8)
    for c in range(4):
        x = 0
        while x < width:
            if pos >= len(buf):
                raise ValueError(f"{fn}: the file ends inside a run-length encoded scanline")
            n = buf[pos]
            pos += 1
            if n > 128:
                n -= 128
                if x + n > width or pos >= len(buf):
                    raise ValueError(f"{fn}: a run of {n} overruns its scanline (column {x} of {width})")
                row[c, x:x + n] = buf[pos]
                pos += 1
            else:
                if n == 0 or x + n > width or pos + n > len(buf):
                    raise ValueError(f"{fn}: a literal run of {n} overruns its scanline (column {x} of {width})")
                row[c, x:x + n] = np.frombuffer(buf, dtype=np.uint8, count=n, offset=pos)
                pos += n
            x += n
    return row.T, pos


def read_hdr_bytes(buf, fn="<bytes>"):
    """The picture in ``buf`` (bytes) as float32 [H, W, 3]."""
    buf = bytes(buf)
    end = buf.find(b"\n\n")
    if not (buf.startswith(b"#?RADIANCE") or buf.startswith(b"#?RGBE")) or end < 0:
        raise ValueError(f"{fn}: not a Radiance picture (no '#?RADIANCE' / '#?RGBE' header closed by a blank line)")
    lines = buf[:end].decode("latin-1").split("\n")[1:]
    formats = [l.split("=", 1)[1].strip() for l in lines if l.startswith("FORMAT=")]
    if formats != ["32-bit_rle_rgbe"]:
        raise ValueError(f"{fn}: FORMAT must be 32-bit_rle_rgbe, got {formats}")
    pos = buf.find(b"\n", end + 2)
    if pos < 0:
        raise ValueError(f"{fn}: the resolution line is missing")
    m = re.fullmatch(r"-Y (\d+) \+X (\d+)", buf[end + 2:pos].decode("latin-1").strip())
    if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        raise ValueError(f"{fn}: the resolution line must be '-Y H +X W', got {buf[end + 2:pos]!r}")
    height, width = int(m.group(1)), int(m.group(2))
    pos += 1
    rgbe = np.empty((height, width, 4), dtype=np.uint8)
    for y in range(height):
        head = buf[pos:pos + 4]
        if _rle_ok(width) and len(head) == 4 and head[0] == 2 and head[1] == 2 and not head[2] & 0x80:
            if (head[2] << 8 | head[3]) != width:
                raise ValueError(f"{fn}: scanline {y} is encoded for width {head[2] << 8 | head[3]}, the picture has {width}")
            rgbe[y], pos = _read_scanline_rle(buf, pos + 4, width, fn)
        else:
            if pos + 4 * width > len(buf):
                raise ValueError(f"{fn}: the file ends inside scanline {y}")
            rgbe[y] = np.frombuffer(buf, dtype=np.uint8, count=4 * width, offset=pos).reshape(width, 4)
            pos += 4 * width
            if bool(((rgbe[y, :, 0] == 1) & (rgbe[y, :, 1] == 1) & (rgbe[y, :, 2] == 1)).any()):
                raise ValueError(f"{fn}: old-style run-length encoding (a pixel 1, 1, 1, n) is not supported")
    return decode_rgbe(rgbe)


def read_hdr(fn):
    with open(fn, "rb") as f:
        return read_hdr_bytes(f.read(), fn)


def _literal(out, seg):
    for k in range(0, len(seg), 128):
        chunk = seg[k:k + 128]
        out.append(len(chunk))
        out += chunk.tobytes()


def _rle_channel(out, row):
    """One channel of a scanline: runs of at least 4 equal bytes as runs, what lies between them as literals."""
    width = row.size
    starts = np.concatenate(([0], np.flatnonzero(row[1:] != row[:-1]) + 1))
    lengths = np.diff(np.concatenate((starts, [width])))
    pos = 0
    for j in np.flatnonzero(lengths >= _MIN_RUN):
        s, n = int(starts[j]), int(lengths[j])
        if s > pos:
            _literal(out, row[pos:s])
        pos = s + n
        while n > 0:
            c = min(n, 127)
            out += bytes((128 + c, int(row[s])))
            n -= c
    if pos < width:
        _literal(out, row[pos:])


def write_hdr_bytes(img, rle=None):
    """float [H, W, 3] -> the bytes of the picture.  ``rle``: None = run-length encode when 8 <= W < 32768, False = flat."""
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[-1] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"hdrio: an image must have shape [H, W, 3], got {list(img.shape)}")
    height, width = img.shape[:2]
    rgbe = encode_rgbe(img)
    out = bytearray(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (height, width))
    if rle is None:
        rle = _rle_ok(width)
    if not rle:
        return bytes(out + rgbe.tobytes())
    if not _rle_ok(width):
        raise ValueError(f"hdrio: a scanline of {width} pixels cannot be run-length encoded (8 <= W < 32768)")
    for y in range(height):
        out += bytes((2, 2, width >> 8, width & 255))
        for c in range(4):
            _rle_channel(out, np.ascontiguousarray(rgbe[y, :, c]))
    return bytes(out)


def write_hdr(fn, img):
    data = write_hdr_bytes(img)
    with open(fn, "wb") as f:
        f.write(data)
