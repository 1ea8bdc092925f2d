"""The environment-probe resamplers with the switch util.HIP_ENVMAP on (csrc/texture.hip with generated coordinates, one launch) against
off (the reference's torch statements with their lookups through ops.texture) on the same GPU in the same process; one JSON line per
(function, direction of the pass).

    timeout -k 10 600 python tools/bench_envmap.py [--window 0.3] [--repeats 5] [--out FILE] [--small]

``fn``            ``latlong_to_cubemap``: a 1024 x 2048 x 3 map to a 512^2 cube; ``cubemap_to_latlong``: a 512^2 x 3 cube to 512 x 1024.
``pass``          ``fwd``: the call; ``fwd_bwd``: the call on a map that requires grad, and the backward of sum(out * w).
``on_ms`` / ``off_ms``   one whole pass, host side included: a host clock around a loop of passes that ends in a device synchronise.
                  MEDIAN of ``--repeats`` windows, smallest and largest beside it; a window holds as many passes as fill ``--window``
                  seconds (sized from a probe after warm-up passes); the windows of the two alternate.
``off_over_on``   the two medians' ratio.  ``max_abs_diff``: the two routes' outputs against each other (same map).
``--small`` cuts the shapes down for a rehearsal.
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
    assert torch.cuda.is_available(), "bench_envmap needs the GPU (no CPU timing)"
    util = importlib.import_module("3danimals_amd.model.render.util")
    g = torch.Generator().manual_seed(5)
    if args.small:
        jobs = [("latlong_to_cubemap", torch.rand(32, 64, 3, generator=g), [16, 16]), ("cubemap_to_latlong", torch.rand(6, 16, 16, 3, generator=g), [16, 32])]
    else:
        jobs = [("latlong_to_cubemap", torch.rand(1024, 2048, 3, generator=g), [512, 512]), ("cubemap_to_latlong", torch.rand(6, 512, 512, 3, generator=g), [512, 1024])]
    out_file = open(args.out, "w") if args.out else None
    switch = util.HIP_ENVMAP
    for name, src, res in jobs:
        src = src.cuda()
        fn = getattr(util, name)
        util.HIP_ENVMAP = True
        a = fn(src, res)
        util.HIP_ENVMAP = False
        diff = float((a - fn(src, res)).abs().max())
        w = torch.rand(a.shape, generator=g).cuda()
        leaf = src.clone().requires_grad_(True)

        def fwd():
            fn(src, res)

        def fwd_bwd():
            leaf.grad = None
            (fn(leaf, res) * w).sum().backward()

        for pname, p in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
            def run(on, count=1):
                util.HIP_ENVMAP = on
                return window_ms(p, count)

            run(True, 3)
            run(False, 2)
            count = max(1, int(args.window * 1e3 / max(run(True, 3), 1e-3)))
            count_off = max(1, int(args.window * 1e3 / max(run(False, 2), 1e-3)))
            on_ms, off_ms = [], []
            for _ in range(args.repeats):
                on_ms.append(run(True, count))
                off_ms.append(run(False, count_off))
            on_ms.sort()
            off_ms.sort()
            row = {"fn": name, "pass": pname, "src": list(src.shape), "res": res, "calls_per_on_window": count, "calls_per_off_window": count_off,
                   "on_ms": round(on_ms[len(on_ms) // 2], 4), "on_ms_min": round(on_ms[0], 4), "on_ms_max": round(on_ms[-1], 4),
                   "off_ms": round(off_ms[len(off_ms) // 2], 4), "off_ms_min": round(off_ms[0], 4), "off_ms_max": round(off_ms[-1], 4),
                   "max_abs_diff": diff}
            row["off_over_on"] = round(row["off_ms"] / row["on_ms"], 2)
            text = json.dumps(row)
            print(text, flush=True)
            if out_file:
                out_file.write(text + "\n")
                out_file.flush()
    util.HIP_ENVMAP = switch
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
