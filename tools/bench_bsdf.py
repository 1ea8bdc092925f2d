"""HIP-event timing of the shading BSDFs and image_loss (csrc/bsdf.hip) against their torch twins on the same GPU; one JSON line per case.

    timeout -k 10 900 python tools/bench_bsdf.py [--window 0.2] [--repeats 5] [--shapes 1x512x512,16x512x512,1x2048x2048] [--out FILE]

Per public function and shape ([B,H,W], the reference's test_perf.py sizes), with per-pixel inputs and -- pbr_bsdf -- with view_pos
[B,1,1,3] / light_pos [1,1,1,3] broadcast: forward and forward + backward (every input requires a gradient), HIP and twin.  Each figure is
the MEDIAN of ``--repeats`` windows of at least ``--window`` seconds (iteration count sized from a probe) with the fastest window beside it.
``calls``: entry-point calls of the library per public call (KernelTimer); ``launches``: kernel launches those make -- one per call, plus
the finishing launch of the image-loss forward and of a backward that reduces a gradient.  ``bytes``: algorithmic bytes -- every input read once, the
result written once; backward: inputs and the upstream gradient read, every per-pixel gradient written.  ``frac``: bytes / time over the
bandwidth the library's own probe kernels (a3d_bw_probe_read / _fill, the kernels of tools/bw_probe) reach on this device in this run.
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, window, repeats):
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
    probe = run(3)
    n = max(3, int(window * 1e6 / max(probe, 1e-3)) + 1)
    us = sorted(run(n) for _ in range(repeats))
    return round(us[len(us) // 2], 1), round(us[0], 1)


def probe_bandwidth(L, window, repeats):
    """GB/s of the probe's read and fill kernels over 1 GiB (far above the 256 MiB last-level cache)."""
    n = 1 << 28
    buf = torch.empty(n, dtype=torch.float32, device="cuda")
    sink = torch.zeros(1024, dtype=torch.float32, device="cuda")
    fill = timed(lambda: L.call("a3d_bw_probe_fill", buf.data_ptr(), n, L.stream()), window, repeats)[0]
    read = timed(lambda: L.call("a3d_bw_probe_read", buf.data_ptr(), n, sink.data_ptr(), L.stream()), window, repeats)[0]
    return 4 * n / read * 1e-3, 4 * n / fill * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="1x512x512,16x512x512,1x2048x2048")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bsdf needs the GPU (no CPU timing)"
    L = importlib.import_module("3danimals_amd._lib")
    ru = importlib.import_module("3danimals_amd.model.render.renderutils")
    out_file = open(args.out, "w") if args.out else None

    def line(**kw):
        text = json.dumps(kw)
        print(text, flush=True)
        if out_file:
            out_file.write(text + "\n")
            out_file.flush()

    read_gbs, fill_gbs = probe_bandwidth(L, args.window, args.repeats)
    line(case="bw_probe", read_GBs=round(read_gbs, 1), fill_GBs=round(fill_gbs, 1))
    gen = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=gen)
    for shape in [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]:
        B, H, W = shape
        px = B * H * W
        full = lambda c=3: rand(B, H, W, c).requires_grad_(True)
        cases = {
            "lambert": (lambda py: ru.lambert(*ins, use_python=py), [full(), full()], 1),
            "frostbite_diffuse": (lambda py: ru.frostbite_diffuse(*ins, use_python=py), [full(), full(), full(), full(1)], 1),
            "pbr_specular": (lambda py: ru.pbr_specular(*ins, use_python=py), [full(), full(), full(), full(), full(1)], 3),
            "pbr_bsdf": (lambda py: ru.pbr_bsdf(*ins, use_python=py), [full() for _ in range(6)], 3),
            "pbr_bsdf frostbite": (lambda py: ru.pbr_bsdf(*ins, bsdf="frostbite", use_python=py), [full() for _ in range(6)], 3),
            "pbr_bsdf broadcast view/light": (lambda py: ru.pbr_bsdf(*ins, use_python=py),
                                              [full() for _ in range(4)] + [rand(B, 1, 1, 3).requires_grad_(True), rand(1, 1, 1, 3).requires_grad_(True)], 3),
        }
        for loss in ("l1", "mse", "smape", "relmse"):
            for tm in ("none", "log_srgb"):
                cases[f"image_loss {loss} {tm}"] = (lambda py, loss=loss, tm=tm: ru.image_loss(*ins, loss, tm, use_python=py), [full(), full()], 0)
        for name, (fn, ins, c_out) in cases.items():
            in_bytes = sum(4 * t.numel() for t in ins)
            fwd_bytes = in_bytes + 4 * px * c_out + (4 if c_out == 0 else 0)
            bwd_bytes = in_bytes + 4 * px * c_out + sum(4 * t.numel() for t in ins if t.numel() >= px)  # (reduced gradients: a few rows)
            row = dict(case=name, shape=list(shape), fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes)
            for tag, py in (("hip", False), ("twin", True)):
                with L.KernelTimer() as t:
                    out = fn(py)
                    n_fwd = sum(v[0] for v in t.summary().values())
                    go = torch.ones_like(out)
                    torch.autograd.grad(out, ins, go)
                    n_all = sum(v[0] for v in t.summary().values())

                def fwd():
                    with torch.no_grad():
                        fn(py)

                def both():
                    torch.autograd.grad(fn(py), ins, go)

                f_us, f_min = timed(fwd, args.window, args.repeats)
                a_us, a_min = timed(both, args.window, args.repeats)
                row.update({f"{tag}_fwd_us": f_us, f"{tag}_fwd_us_min": f_min, f"{tag}_fwdbwd_us": a_us, f"{tag}_fwdbwd_us_min": a_min})
                if tag == "hip":
                    reduces = any(t.numel() < px for t in ins)  # (an input broadcast over pixels: its gradient is reduced in the launch)
                    row.update(calls_fwd=n_fwd, calls_bwd=n_all - n_fwd, launches_fwd=n_fwd + (c_out == 0),
                               launches_bwd=(n_all - n_fwd) + reduces,
                               fwd_frac=round(fwd_bytes / f_us * 1e-3 / read_gbs, 3),
                               bwd_frac=round(bwd_bytes / max(a_us - f_us, 1e-3) * 1e-3 / read_gbs, 3))
                del out
            row["speedup_fwd"] = round(row["twin_fwd_us"] / row["hip_fwd_us"], 2)
            row["speedup_fwdbwd"] = round(row["twin_fwdbwd_us"] / row["hip_fwdbwd_us"], 2)
            line(**row)
            del ins
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
