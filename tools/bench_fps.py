"""Farthest-point sampling with the switch skinning.DEVICE_FPS on (csrc/fps.hip) against off (the reference's torch loop, the parent
commit's path) on the same GPU in the same process; one JSON line per (function, N, V).

    timeout -k 10 900 python tools/bench_fps.py [--window 0.3] [--repeats 5] [--out FILE] [--small]

``fn``            ``sample``: util.sample_farthest_points(pts [N,3,V], V // 4) -- the first picks drawn, the picks, the gather;
                  ``bones``: skinning.estimate_bones(seq [1,N,V,3], resample=True, 8 body bones, 4 legs of 3 bones, 'z_minmax_y+',
                  bone_y_threshold 0.4, chain rebuilt: the call Fauna makes every iteration, its one read-back included).
``on_ms`` / ``off_ms``   one whole call, host side included: a host clock around a loop of calls that ends in a device synchronise.
                  MEDIAN of ``--repeats`` windows, smallest and largest beside it (the run-to-run spread of this record); on-windows hold
                  as many calls as fill ``--window`` seconds, on and off alike (each sized from a probe, after warm-up calls; one call
                  where a call is longer than the window: V = 107,000, ``calls_per_*_window`` says); the windows of the two alternate.
``off_over_on``   the two medians' ratio.
``same_picks``    (sample) the share of indices on which the two paths agree: they may differ where float32 rounding decides a pick
                  (torch's norm on the GPU is another float32 evaluation of the same distance; tests/test_fps_gpu.py bounds what the
                  kernel may do there).
Clouds: a seeded body-and-four-legs point cloud per instance (every leg quadrant stays populated after sampling), V = 5,720 (the R = 64
quadruped) with N in {1, 16, 200} and V = 107,000 with N = 1; ``--small`` cuts that to one small shape for a rehearsal.
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clouds(N, V, seed=21):
    """[N,V,3]: vertex v in cluster v % 5 -- a body around the z axis and four legs below it, one per top-view quadrant."""
    u = torch.rand(N, V, 3, generator=torch.Generator().manual_seed(seed + V))
    k = (torch.arange(V) % 5)[None, :]
    sx = torch.where((k == 1) | (k == 2), 1.0, -1.0)
    sz = torch.where((k == 1) | (k == 4), 1.0, -1.0)
    leg = torch.stack([sx * (0.05 + 0.55 * u[..., 0]), -1.4 + 0.8 * u[..., 1], sz * (0.05 + 0.75 * u[..., 2])], -1)
    body = torch.stack([-0.1 + 0.2 * u[..., 0], 0.2 + 0.4 * u[..., 1], -1.0 + 2.0 * u[..., 2]], -1)
    return torch.where((k == 0)[..., None], body, leg).contiguous()


def window_ms(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fps needs the GPU (no CPU timing)"
    L = importlib.import_module("3danimals_amd._lib")
    sk = importlib.import_module("3danimals_amd.model.geometry.skinning")
    util = importlib.import_module("3danimals_amd.model.geometry.util")
    shapes = [(2, 400)] if args.small else [(1, 5720), (16, 5720), (200, 5720), (1, 107000)]
    out_file = open(args.out, "w") if args.out else None
    switch = sk.DEVICE_FPS
    for N, V in shapes:
        pts = clouds(N, V).cuda()
        k = V // 4
        fns = {
            "sample": lambda: util.sample_farthest_points(pts.transpose(1, 2), k),
            "bones": lambda: sk.estimate_bones(pts[None], 8, resample=True, n_legs=4, n_leg_bones=3, body_bones_mode="z_minmax_y+",
                                               bone_y_threshold=0.4),
        }
        for name, fn in fns.items():
            def run(on, count=1):
                sk.DEVICE_FPS = on
                return window_ms(fn, count)

            row = dict(fn=name, N=N, V=V, k=k)
            if name == "sample":
                picks = []
                for on in (True, False):
                    sk.DEVICE_FPS = on
                    torch.manual_seed(1)
                    picks.append(util.sample_farthest_points(pts.transpose(1, 2), k, return_index=True)[1])
                row["same_picks"] = round(float((picks[0] == picks[1]).float().mean()), 6)
            run(True, 2)
            run(False, 1)
            count = max(1, int(args.window * 1e3 / max(run(True, 2), 1e-3)))
            count_off = max(1, int(args.window * 1e3 / max(run(False, 1), 1e-3)))
            on_ms, off_ms = [], []
            for _ in range(args.repeats):
                on_ms.append(run(True, count))
                off_ms.append(run(False, count_off))
            L.poll_deferred()
            on_ms.sort()
            off_ms.sort()
            row.update(calls_per_on_window=count, calls_per_off_window=count_off, on_ms=round(on_ms[len(on_ms) // 2], 3), on_ms_min=round(on_ms[0], 3), on_ms_max=round(on_ms[-1], 3),
                       off_ms=round(off_ms[len(off_ms) // 2], 3), off_ms_min=round(off_ms[0], 3), off_ms_max=round(off_ms[-1], 3))
            row["off_over_on"] = round(row["off_ms"] / row["on_ms"], 2)
            text = json.dumps(row)
            print(text, flush=True)
            if out_file:
                out_file.write(text + "\n")
                out_file.flush()
        del pts
    sk.DEVICE_FPS = switch
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
