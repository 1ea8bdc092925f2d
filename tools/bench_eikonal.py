"""What the eikonal regulariser (DMTetGeometry.get_sdf_gradient + loss + backward to the SDF field's parameters) costs on the bench
scene (magicpony, batch 16 at 256x256, 10,000 points), two ways; one JSON line.

    timeout -k 10 600 python tools/bench_eikonal.py [--calls 50] [--steps 40] [--warmup 10] [--rounds 3] [--out FILE]

``chain_us`` / ``chain_us_min``   HIP-event time of one get_sdf_gradient() + ((|g| - 1)^2).mean() + backward(), replayed from the
                  HIP graphs as the step replays it (the point sampling and the loss's own few launches included): median and best
                  of ``--calls`` single calls, each bracketed by events on an otherwise idle device.
``step_on_ms`` / ``step_off_ms``  SyntheticScene.step(sdf_reg=True) against step(sdf_reg=False): ``--steps`` steps after ``--warmup``,
                  wall clock around a synchronised loop, the two alternated ``--rounds`` times; medians, with every round listed.
``in_step_ms``    step_on_ms - step_off_ms: what the regulariser adds to the training step.
``launches``      GPU kernels of one chain call as the profiler counts them (graph replays included); ``launches_under_10us`` those of
                  less than 10 us, ``kernel_us`` their summed device time.  ``--kernels N`` also prints the N kernels with the most time.
``field_grad``    hostnets.USE_FIELD_GRAD where the tree has the switch (null before it).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_eikonal needs the GPU"
    pipeline = importlib.import_module("3danimals_amd.pipeline")
    hostnets = importlib.import_module("3danimals_amd.hostnets")
    importlib.import_module("3danimals_amd.gemm_tuning").enable()
    dev = torch.device("cuda", 0)
    scene = pipeline.SyntheticScene(grid_res=64, batch=16, resolution=(256, 256), device=dev, seed=0, workload="magicpony", deform=True)
    scene.netShape.capture_sdf_gradient_graph()
    for _ in range(3):
        scene.step()
    torch.cuda.synchronize()
    geo = scene.netShape
    params = [p for p in geo.mlp.parameters() if p.requires_grad]

    def chain():
        for p in params:
            p.grad = None
        loss = ((geo.get_sdf_gradient().norm(dim=-1) - 1) ** 2).mean()
        loss.backward()
        return loss

    for _ in range(5):
        chain()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        chain()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    launches = small = kernel_us = None
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            chain()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA]
        launches, small = len(kernels), sum(e.device_time < 10 for e in kernels)
        kernel_us = round(sum(e.device_time for e in kernels), 1)
        if args.kernels:
            table = {}
            for e in kernels:
                n, t = table.get(e.name, (0, 0.0))
                table[e.name] = (n + 1, t + e.device_time)
            for name, (n, t) in sorted(table.items(), key=lambda kv: -kv[1][1])[:args.kernels]:
                print(f"{t:9.1f} us {n:4d} x  {name[:150]}", flush=True)
    except Exception as err:  # the figure is a by-product: never lose the timings to it
        launches = f"unavailable ({type(err).__name__})"

    def steps_ms(flag):
        for _ in range(args.warmup):
            scene.step(sdf_reg=flag)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.steps):
            scene.step(sdf_reg=flag)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / args.steps

    on, off = [], []
    for _ in range(args.rounds):
        on.append(steps_ms(True))
        off.append(steps_ms(False))
    med = lambda v: sorted(v)[len(v) // 2]
    row = dict(points=10000, chain_us=round(times[len(times) // 2], 1), chain_us_min=round(times[0], 1), launches=launches,
               launches_under_10us=small, kernel_us=kernel_us,
               step_on_ms=round(med(on), 3), step_off_ms=round(med(off), 3), in_step_ms=round(med(on) - med(off), 3),
               step_on_rounds=[round(v, 3) for v in on], step_off_rounds=[round(v, 3) for v in off],
               field_grad=getattr(hostnets, "USE_FIELD_GRAD", None), device=torch.cuda.get_device_name(0))
    text = json.dumps(row)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
