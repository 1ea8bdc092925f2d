"""What the conditioned SDF field (hostnets.CoordMLP_Mod) costs on the bench's fauna scene (batch 16 at 256x256, Kuhn R=64 grid, 5 layers of 256,
128-d embedding) with hostnets.USE_FIELD_MOD off and on, in ONE process, the two alternated; one JSON line.

    timeout -k 10 400 python tools/bench_field_mod.py [--calls 30] [--points N ...] [--out FILE]

``chain_us``       HIP-event time of the eikonal regulariser alone: get_sdf_gradient(feats) + ((|g| - 1)^2).mean() + backward(), eager (the
                   conditioned field is not replayed from graphs); median and best of ``--calls`` calls on an otherwise idle device.
``grid_pass_us``   the grad-free pass of the field over every grid vertex (get_sdf under no_grad), the same way.
``launches``       GPU kernels of one chain call as the profiler counts them, ``launches_under_10us`` those of less than 10 us,
                   ``kernel_us`` their summed device time.
``epilogue_gemms`` torch._addmm_activation calls of one getMesh(feats): the grid pass reaches the epilogue-fused forward (0 with the switch off).
``sizes``          for every ``--points`` M: the eikonal chain of the field alone over M random points (value, autograd.grad with create_graph,
                   the loss, backward), the same way -- where the gate could be narrowed.
The step time itself is bench.py's figure (``--workload fauna --carry-state`` with A3D_FIELD_MOD=0 / 1): the share of the step these two
passes of the field take is (chain_us + grid_pass_us) over it; the few thousand surface rows of getMesh and their backward take the same
code either way.
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--points", type=int, nargs="*", default=[256, 2048, 10000, 32768])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_field_mod needs the GPU"
    pipeline = importlib.import_module("3danimals_amd.pipeline")
    hostnets = importlib.import_module("3danimals_amd.hostnets")
    importlib.import_module("3danimals_amd.gemm_tuning").enable()
    dev = torch.device("cuda", 0)
    scene = pipeline.SyntheticScene(grid_res=64, batch=16, resolution=(256, 256), device=dev, seed=0, workload="fauna")
    geo, feat = scene.netShape, scene.class_emb
    params = [p for p in geo.mlp.parameters() if p.requires_grad] + [feat]
    med = lambda v: sorted(v)[len(v) // 2]

    def clear():
        for p in params:
            p.grad = None

    def chain():
        clear()
        loss = ((geo.get_sdf_gradient(feats=feat).norm(dim=-1) - 1) ** 2).mean()
        loss.backward()

    def grid_pass():
        with torch.no_grad():
            geo.get_sdf(geo.verts, feats=feat)

    def field_chain(pts):
        def run():
            clear()
            x = pts.detach().requires_grad_(True)
            y = geo.mlp(x, feat=feat.unsqueeze(0))
            g, = torch.autograd.grad([y], x, grad_outputs=torch.ones_like(y), create_graph=True)
            ((g.norm(dim=-1) - 1) ** 2).mean().backward()
        return run

    def events(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        return round(med(times), 1), round(min(times), 1)

    def launches():
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            chain()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA]
        return len(kernels), sum(e.device_time < 10 for e in kernels), round(sum(e.device_time for e in kernels), 1)

    def epilogue_gemms():
        plain, calls = torch._addmm_activation, []
        torch._addmm_activation = lambda *a, **k: (calls.append(1), plain(*a, **k))[1]
        try:
            with torch.enable_grad():
                geo.getMesh(feats=feat)
        finally:
            torch._addmm_activation = plain
        return len(calls)

    was = hostnets.USE_FIELD_MOD
    row = dict(grid_vertices=int(geo.verts.shape[0]), device=torch.cuda.get_device_name(0))
    gen = torch.Generator().manual_seed(1)
    samples = {m: ((torch.rand(m, 3, generator=gen) - 0.5) * geo.grid_scale).to(dev) for m in args.points}
    try:
        geo.getMesh(feats=feat)  # mesh_verts for the regulariser's sample
        for on in (False, True):
            hostnets.USE_FIELD_MOD = on
            c, g = events(chain), events(grid_pass)
            n, small, kernel_us = launches()
            row["on" if on else "off"] = dict(chain_us=c[0], chain_us_min=c[1], grid_pass_us=g[0], grid_pass_us_min=g[1], launches=n,
                                              launches_under_10us=small, kernel_us=kernel_us, epilogue_gemms=epilogue_gemms(),
                                              sizes={str(m): events(field_chain(samples[m]))[0] for m in args.points})
    finally:
        hostnets.USE_FIELD_MOD = was
    text = json.dumps(row)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
