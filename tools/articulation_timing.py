"""Timing of the articulation glue (csrc/articulation.hip through 3danimals_amd/articulation.py) against the torch statements of the
same commit -- what a user of this package, or of the reference on ROCm, runs today -- on the same GPU and the same seeded inputs.

    timeout -k 10 600 python tools/articulation_timing.py [--iters 200] [--repeats 7] [--out FILE]

Shapes: the descriptors at N = 16, K = 20, C = D = 384, 32 x 32 patches, "sample+global", forward plus backward (gradients to feat and
patch_feat), with patch_feat NCHW and as a permuted NHWC view; the limits at N = 16, K = 20 (the Fauna table after the switch) with reg,
forward plus backward.  The two routes alternate window by window in one process, after a warm-up of both.  A window is ``--iters``
whole calls, timed twice over the same loop: with device events around it (``event_us``: what the stream was busy or waiting for) and
with a host clock -- ``enqueue_us`` until the last call has returned, ``host_us`` until a synchronise behind it.  Per figure: the median
of ``--repeats`` windows, with the fastest and the slowest beside it (the spread).  ``ratio`` is torch's median over HIP's;
``hip_not_slower`` is the issue's condition: HIP's median host_us is not above torch's by more than the spread of either.
``kernel_us``: per entry point of the HIP route, the mean over 100 calls of a pair of device events around that one call
(_lib.KernelTimer) -- the kernel with its launch, without the Python around it; the figure the chunk widths are compared on.
``A3D_LIB`` selects another build of the library (_lib), ``A3D_ARTICULATION_CHUNK_BUILT`` says which chunk width that build has.
One JSON object; with --out it is also written to that file."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return dict(event_us=a.elapsed_time(b) * 1e3 / iters, enqueue_us=(t1 - t0) * 1e6 / iters, host_us=(t2 - t0) * 1e6 / iters)


def compare(routes, iters, repeats, warmup=20):
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    rows = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():  # alternating
            rows[name].append(window(fn, iters))
    out = {}
    for name, ws in rows.items():
        out[name] = {k: dict(median=round(statistics.median(w[k] for w in ws), 2), min=round(min(w[k] for w in ws), 2),
                             max=round(max(w[k] for w in ws), 2)) for k in ws[0]}
    spread = max(out[n]["host_us"]["max"] - out[n]["host_us"]["min"] for n in out)
    out["ratio"] = {k: round(out["torch"][k]["median"] / out["hip"][k]["median"], 2) for k in out["hip"]}
    out["hip_not_slower"] = bool(out["hip"]["host_us"]["median"] <= out["torch"]["host_us"]["median"] + spread)
    return out


def kernel_us(fn, calls=100):
    L = importlib.import_module("3danimals_amd._lib")
    with L.KernelTimer() as timer:
        for _ in range(calls):
            fn()
        return {name: round(ms * 1e3, 2) for name, (_, ms) in timer.summary().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("articulation_timing: no GPU; a timing taken anywhere else says nothing")
    A = importlib.import_module("3danimals_amd.articulation")
    dev = "cuda"
    rng = np.random.default_rng(36)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    N, K, C, D, hw = 16, 20, 384, 384, 32
    bones = f32(rng.uniform(-0.6, 0.6, (1, K, 2, 3)))
    mvp = rng.normal(0.0, 1.0, (N, 4, 4))
    mvp[:, 3] = np.concatenate([rng.uniform(-0.3, 0.3, (N, 3)), rng.uniform(2.2, 2.8, (N, 1))], -1)
    w2c = np.tile(np.eye(4), (N, 1, 1))
    w2c[:, :3, 3] = rng.uniform(-1, 1, (N, 3))
    mvp, w2c = f32(mvp), f32(w2c)
    feat = f32(rng.normal(size=(N, D))).requires_grad_(True)
    values = f32(rng.normal(size=(N, C, hw, hw)))
    g = f32(rng.normal(size=(N, K, D + C)))
    result = dict(device=torch.cuda.get_device_name(0), library=os.path.relpath(importlib.import_module("3danimals_amd._lib").LIB_PATH, ROOT),
                  chunk=int(os.environ.get("A3D_ARTICULATION_CHUNK_BUILT", A.CHUNK)), iters=args.iters, repeats=args.repeats,
                  shapes=dict(N=N, K=K, C=C, D=D, patches=[hw, hw], mode="sample+global"))

    for layout in ("nchw", "nhwc"):
        patch = (values.clone() if layout == "nchw" else values.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)).requires_grad_(True)

        def step(fn):
            bf, _ = fn(bones, mvp, w2c, 10.0, 7.0, feat, patch, "sample+global")
            return torch.autograd.grad(bf, [feat, patch], g)

        routes = dict(hip=lambda: step(A.bone_inputs), torch=lambda: step(A._bone_inputs_torch))
        a, b = routes["hip"](), routes["torch"]()
        row = compare(routes, args.iters, args.repeats)
        row["max_abs_difference"] = dict(g_feat=float((a[0] - b[0]).abs().max()), g_patch=float((a[1] - b[1]).abs().max()))
        row["g_patch_strides_kept"] = bool(a[1].stride() == patch.stride())
        row["kernel_us"] = kernel_us(routes["hip"])
        result[f"bone_inputs_fwd_bwd_{layout}"] = row

    limits = A.limits_fauna(8, 4, 3, 0.1, 60, False, 300001, 300000, True, True, 0.1)
    x = f32(rng.normal(0.0, 12.0, (N, K, 3))).requires_grad_(True)
    ga, one = f32(rng.normal(size=(N, K, 3))), torch.ones((), device=dev)

    def lstep(fn):
        angles, reg = fn(x, limits, True)
        return torch.autograd.grad([angles, reg], x, [ga, one])

    routes = dict(hip=lambda: lstep(A.constrain_angles), torch=lambda: lstep(A._constrain_angles_torch))
    a, b = routes["hip"](), routes["torch"]()
    row = compare(routes, args.iters, args.repeats)
    row["max_abs_difference"] = dict(g_x=float((a[0] - b[0]).abs().max()))
    row["kernel_us"] = kernel_us(routes["hip"])
    result["constrain_angles_fwd_bwd"] = row

    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
