"""HIP-event timing of ops.distance_transform (csrc/edt.hip) against the host path it replaces on the same masks in the same process;
one JSON line per (shape, fill, idx).

    timeout -k 10 900 python tools/bench_edt.py [--window 0.2] [--repeats 5] [--batches 16 64] [--out FILE]

Masks are float32 [N,256,256] on the GPU, read as the float kind with thresholds (1, 0) and scale 256 (both channels from one call):
``disc`` a silhouette-like disc per image (centre and radius vary with the image), ``random`` a 0.5 fill.

``hip_us``        the op, host side included: the MEDIAN of ``--repeats`` windows of at least ``--window`` seconds timed with HIP events
                  around a loop of whole calls (iteration count sized from a probe, after three warm-up calls); fastest window beside it.
``host_us``       the path of the parent commit for the same mask: device -> host, the scipy loop over images and channels, host ->
                  device, under a host clock that ends in a synchronise; one call per window, windows alternating with the op's.
                  This is the baseline; the code under test is not.
``columns_us`` / ``rows_us``   device time of the two launches, from a torch.profiler trace of 20 calls taken after the timed windows
                  ("not measured" where the trace has no such kernel).
``*_gbs``         algorithmic bytes over that time: the mask read once and the 16-bit column offsets written once (columns); the
                  offsets read once and every output written once (rows).
``row_steps``     what the row launch executes: for every wave of 64 neighbouring pixels, 64 x the longest outward walk in it (a walk
                  ends at the first d with d * d >= d2, one step later with idx), summed -- each step is two candidates; computed on the
                  host from the squared distances.  ``row_gsteps_s`` is that over rows_us.
``bound``         which of the two the launch is closer to: ``bytes`` when its algorithmic bytes at 6.3 TB/s account for more than
                  half of its time, else ``steps`` (rows) / ``instructions`` (columns: the bit-mask arithmetic and its 2-byte stores).
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_US = 6.3e6  # achievable HBM rate


def window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def host_window_us(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6


def make_masks(n, side, fill):
    if fill == "random":
        return (torch.rand(n, side, side, generator=torch.Generator().manual_seed(n)) < 0.5).float()
    yy, xx = np.mgrid[0:side, 0:side]
    k = np.arange(n)[:, None, None]
    cy, cx, r = side * (0.45 + 0.01 * (k % 7)), side * (0.55 - 0.01 * (k % 5)), side * (0.2 + 0.01 * (k % 11))
    return torch.from_numpy(((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.float32))


def kernel_times_us(fn, calls=20):
    """name fragment -> mean device microseconds per call, from a torch.profiler trace."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        total = getattr(ev, "device_time_total", None)
        if total is None:
            total = getattr(ev, "cuda_time_total", 0.0)
        for frag in ("edt_columns_kernel", "edt_rows_kernel"):
            if frag in ev.key:
                out[frag] = out.get(frag, 0.0) + total / calls
    return out


def row_steps(d2, with_idx):
    """[.., H, W] int squared distances -> steps the row launch executes (64 x the longest walk of every 64 neighbouring pixels)."""
    d2 = d2.reshape(-1, d2.shape[-1]).astype(np.int64)
    w = d2.shape[1]
    root = np.ceil(np.sqrt(d2.astype(np.float64))).astype(np.int64)  # the first d with d * d >= d2
    steps = root + (1 if with_idx else 0)
    x = np.arange(w)
    steps = np.minimum(steps, np.maximum(x, w - 1 - x)[None, :] + 1)
    pad = (-w) % 64
    steps = np.pad(steps, ((0, 0), (0, pad)))
    return int(steps.reshape(steps.shape[0], -1, 64).max(-1).sum() * 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_edt needs the GPU (no CPU timing)"
    ops = importlib.import_module("3danimals_amd.ops")
    from scipy.ndimage import distance_transform_edt

    def host_path(mask_gpu):  # what pipeline._distance_transforms did with a mask on the GPU before the op existed (the same work, in the op's channel order)
        m = mask_gpu.cpu().numpy() > 0.5
        out = np.zeros((m.shape[0], 2, *m.shape[1:]), dtype=np.float32)
        for b in range(m.shape[0]):
            out[b, 0] = distance_transform_edt(m[b]) / max(m.shape[1:])
            out[b, 1] = distance_transform_edt(~m[b]) / max(m.shape[1:])
        return torch.from_numpy(out).to(mask_gpu.device)

    out_file = open(args.out, "w") if args.out else None
    side = args.side
    for n in args.batches:
        for fill in ("disc", "random"):
            mask = make_masks(n, side, fill).cuda()
            want = host_path(mask)
            d2 = ops.distance_transform(mask, squared=True, thresholds=(1.0, 0.0)).cpu().numpy()
            for with_idx in (False, True):
                fn = lambda: ops.distance_transform(mask, scale=float(side), return_indices=with_idx, thresholds=(1.0, 0.0))  # noqa: E731
                got = fn()
                equal = bool(torch.equal(got[0] if with_idx else got, want))
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                count = max(3, int(args.window * 1e6 / max(window_us(fn, 3), 1e-3)) + 1)
                hip, host = [], []
                for _ in range(args.repeats):
                    hip.append(window_us(fn, count))
                    host.append(host_window_us(lambda: host_path(mask)))
                hip.sort()
                host.sort()
                px = 2 * n * side * side  # image-channels x pixels
                bytes_columns = n * side * side * 4 + px * 2
                bytes_rows = px * 2 + px * 4 * (2 if with_idx else 1)
                row = dict(N=n, H=side, W=side, fill=fill, idx=with_idx, equal_to_host_path=equal, calls_per_window=count,
                           hip_us=round(hip[len(hip) // 2], 1), hip_us_min=round(hip[0], 1), host_us=round(host[len(host) // 2], 1),
                           host_us_min=round(host[0], 1), row_steps=row_steps(d2, with_idx), bytes_columns=bytes_columns, bytes_rows=bytes_rows)
                row["speedup"] = round(row["host_us"] / row["hip_us"], 1)
                try:
                    k = kernel_times_us(fn)
                except Exception as e:  # (no trace: say so, keep the timed figures)
                    k = {}
                    row["profiler_error"] = repr(e)[:200]
                for tag, frag, nbytes in (("columns", "edt_columns_kernel", bytes_columns), ("rows", "edt_rows_kernel", bytes_rows)):
                    us = k.get(frag)
                    if not us:
                        row[f"{tag}_us"] = row[f"{tag}_gbs"] = row[f"{tag}_bound"] = "not measured"
                        continue
                    row[f"{tag}_us"] = round(us, 2)
                    row[f"{tag}_gbs"] = round(nbytes / us / 1e3, 1)
                    row[f"{tag}_bound"] = "bytes" if nbytes / HBM_BYTES_PER_US > 0.5 * us else ("steps" if tag == "rows" else "instructions")
                    if tag == "rows":
                        row["row_gsteps_s"] = round(row["row_steps"] / us / 1e3, 1)
                text = json.dumps(row)
                print(text, flush=True)
                if out_file:
                    out_file.write(text + "\n")
                    out_file.flush()
            del mask, want
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
