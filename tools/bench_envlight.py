"""HIP-event timing of EnvironmentLight.build_mips (csrc/envlight.hip) for base resolutions 512, 256 and 64; one JSON line per case.

    timeout -k 10 900 python tools/bench_envlight.py [--window 0.2] [--repeats 5] [--bases 512,256,64]

Per base: build_mips forward and forward + backward (gradient to env_base); per specular level the number of (p, q) pairs the
filter visits (the rectangle areas of the bounds table, summed: what the loops walk, cone test included) and pairs per second from the
level's own forward time; the one-off cost and the bytes of the bounds tables (first build_mips of a resolution).
Every figure is the MEDIAN of ``--repeats`` timed windows of at least ``--window`` seconds each (the iteration count is sized from a
probe), with the fastest window beside it (``*_min``); a row whose time is a few tens of microseconds (the 64 x 64 level of a base-64
light: 0.09 M pairs) measures the launch and the autograd node, not the kernel.  ``bounds_ms`` is the bounds launch alone, between
two events, into a table allocated beforehand.
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, window, repeats):
    """(median, min) microseconds per call over ``repeats`` windows of >= ``window`` seconds."""
    def run(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    probe = run(5)
    n = max(5, int(window * 1e6 / max(probe, 1e-3)) + 1)
    us = sorted(run(n) for _ in range(repeats))
    return round(us[len(us) // 2], 1), round(us[0], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bases", default="512,256,64")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_envlight needs the GPU (no CPU timing)"
    ops = importlib.import_module("3danimals_amd.ops")
    light = importlib.import_module("3danimals_amd.model.render.light")
    ru_ops = importlib.import_module("3danimals_amd.model.render.renderutils.ops")

    def line(case, **kw):
        print(json.dumps(dict(case=case, **kw)), flush=True)

    for base in [int(b) for b in args.bases.split(",")]:
        torch.manual_seed(0)
        lgt = light.create_trainable_env_rnd(base)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lgt.build_mips()  # first call of this resolution: cutoff cosines and bounds tables
        torch.cuda.synchronize()
        first = time.perf_counter() - t0
        n = len(lgt.specular)
        rough = [(i / (n - 2)) * (lgt.MAX_ROUGHNESS - lgt.MIN_ROUGHNESS) + lgt.MIN_ROUGHNESS for i in range(n - 1)] + [1.0]
        table_bytes = 0
        levels = []
        for i, r in enumerate(rough):
            N = base >> i
            c, table = ru_ops.specular_bounds(N, r, 0.99, lgt.base.device)
            table_bytes += table.numel() * table.element_size()
            t = table.long()
            pairs = int(((t[..., 1] - t[..., 0] + 1).clamp(min=0) * (t[..., 3] - t[..., 2] + 1).clamp(min=0)).sum())
            x = torch.rand(6, N, N, 3, device=lgt.base.device)
            go = torch.rand(6, N, N, 4, device=lgt.base.device)
            xg = x.clone().requires_grad_(True)
            out = ops.specular_cubemap_raw(xg, r, c, table)
            T = lambda fn: timed(fn, args.window, args.repeats)
            fwd, fwd_min = T(lambda: ops.specular_cubemap_raw(x, r, c, table))
            bwd, bwd_min = T(lambda: torch.autograd.grad(out, xg, go, retain_graph=True))
            scratch = torch.empty_like(table)
            desc = ops._env_desc(N, None, None, None, scratch, 1.0, c)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.call("a3d_cubemap_specular_bounds", ctypes.byref(desc), ops.stream())
            e1.record()
            torch.cuda.synchronize()
            levels.append(dict(N=N, roughness=round(r, 4), cutoff_cosine=c, pairs=pairs, fwd_us=fwd, fwd_us_min=fwd_min, bwd_us=bwd,
                               bwd_us_min=bwd_min, fwd_gpairs_per_s=round(pairs / fwd * 1e-3, 2), bwd_gpairs_per_s=round(pairs / bwd * 1e-3, 2),
                               bounds_ms=round(e0.elapsed_time(e1), 3)))
        xd = torch.rand(6, 16, 16, 3, device=lgt.base.device)
        diffuse_us, diffuse_min = timed(lambda: ops.diffuse_cubemap(xd), args.window, args.repeats)

        def forward():
            lgt.build_mips()

        def forward_backward():
            lgt.base.grad = None
            lgt.build_mips()
            (sum(s.sum() for s in lgt.specular) + lgt.diffuse.sum()).backward()

        f, f_min = timed(forward, args.window, args.repeats)
        fb, fb_min = timed(forward_backward, args.window, args.repeats)
        line("build_mips", base=base, levels=n, fwd_us=f, fwd_us_min=f_min, fwd_bwd_us=fb, fwd_bwd_us_min=fb_min, first_call_s=round(first, 3),
             bounds_table_bytes=table_bytes, pairs=sum(l["pairs"] for l in levels), diffuse_fwd_us=diffuse_us, diffuse_fwd_us_min=diffuse_min)
        for l in levels:
            line("specular_level", base=base, **l)


if __name__ == "__main__":
    main()
