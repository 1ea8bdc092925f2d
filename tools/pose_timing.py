"""Timing of the camera-pose glue (csrc/pose.hip through 3danimals_amd/pose.py) against the torch statements of the same commit -- what
a user of this package, or of the reference on ROCm, runs today -- on the same GPU and the same seeded inputs.

    timeout -k 10 600 python tools/pose_timing.py [--iters 200] [--repeats 7] [--out profiles/pose_timing.json]

Shapes: predict_cameras (heads, pick, cameras) forward plus backward with all nine float outputs fed, random sampling on, at N = 16
(H = 4), N = 200 (H = 4) and N = 16 (H = 8, octlookat); cameras_from_pose alone, forward plus backward, at N = 16; random_view_cameras at
b = 16 against the reference's loop over the batch (one ``.item()``, one 4x4 host tensor and one host-to-device copy per image), forward
only.  The two routes alternate window by window in one process, after a warm-up of both; the torch route is the same public function
with ``pose.DEVICE = False``.  A window is ``--iters`` whole calls, timed twice over the same loop: with device events around it
(``event_us``: what the stream was busy or waiting for) and with a host clock -- ``enqueue_us`` until the last call has returned,
``host_us`` until a synchronise behind it.  Per figure: the median of ``--repeats`` windows, with the fastest and the slowest beside it
(the spread).  ``ratio`` is torch's median over HIP's; ``hip_not_slower``: HIP's median host_us is not above torch's by more than the
spread of either.  ``kernel_us``: per entry point of the HIP route, the mean over 100 calls of a pair of device events around that one
call (_lib.KernelTimer) -- the kernel with its launch, without the Python around it.  One JSON object; with --out it is also written to
that file."""
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
        sys.exit("pose_timing: no GPU; a timing taken anywhere else says nothing")
    P = importlib.import_module("3danimals_amd.pose")
    dev = "cuda"
    rng = np.random.default_rng(37)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    result = dict(device=torch.cuda.get_device_name(0), library=os.path.relpath(importlib.import_module("3danimals_amd._lib").LIB_PATH, ROOT),
                  iters=args.iters, repeats=args.repeats)

    def with_device(flag, fn):
        def run():
            P.DEVICE = flag
            try:
                return fn()
            finally:
                P.DEVICE = True

        return run

    quad = torch.tensor([[1, 1, 1], [-1, 1, 1], [-1, 1, -1], [1, 1, -1]], dtype=torch.float32)
    octs = torch.tensor([[x, y, z] for x in (1, -1) for y in (1, -1) for z in (1, -1)], dtype=torch.float32)
    max_trans = torch.tensor([0.44, 0.44, 1.1])  # (on the host, as the reference keeps them: its forward_pose moves them every call)
    names = ("poses_raw", "pose_raw", "pose", "mvp", "w2c", "campos", "rot_prob", "rot_logit", "rots_probs")
    for N, H in ((16, 4), (200, 4), (16, 8)):
        raw = f32(rng.normal(size=(N, 4 * H + 3))).requires_grad_(True)
        signs = quad if H == 4 else octs
        shapes = dict(poses_raw=(N, 4 * H + 3), pose_raw=(N, 6), pose=(N, 12), mvp=(N, 4, 4), w2c=(N, 4, 4), campos=(N, 3), rot_prob=(N,),
                      rot_logit=(N,), rots_probs=(N, H))
        g = [f32(rng.normal(size=shapes[k])) for k in names]

        def step():
            out = P.predict_cameras(raw, 7000, orthant_signs=signs, max_trans_xyz_range=max_trans, cam_pos_z_offset=10.0, fov=25.0, oct=H == 8,
                                    num_hypos=H)  # (the two permutations are drawn inside, by either route)
            res = list(out[:6]) + [out[6][k] for k in names[6:]]
            return torch.autograd.grad(res, raw, g)[0]

        routes = dict(hip=with_device(True, step), torch=with_device(False, step))
        torch.manual_seed(1)
        a = routes["hip"]()
        torch.manual_seed(1)
        b = routes["torch"]()
        row = compare(routes, args.iters, args.repeats)
        row["max_abs_difference"] = dict(g_raw=float((a - b).abs().max()))
        row["kernel_us"] = kernel_us(routes["hip"])
        result[f"predict_cameras_fwd_bwd_n{N}_h{H}"] = row

    N = 16
    pose = f32(rng.normal(size=(N, 12))).requires_grad_(True)
    g = [f32(rng.normal(size=s)) for s in ((N, 4, 4), (N, 4, 4), (N, 3))]
    step = lambda: torch.autograd.grad(list(P.cameras_from_pose(pose, 10.0, 25.0)), pose, g)[0]
    routes = dict(hip=with_device(True, step), torch=with_device(False, step))
    a, b = routes["hip"](), routes["torch"]()
    row = compare(routes, args.iters, args.repeats)
    row["max_abs_difference"] = dict(g_pose=float((a - b).abs().max()))
    row["kernel_us"] = kernel_us(routes["hip"])
    result[f"cameras_from_pose_fwd_bwd_n{N}"] = row

    w2c_pred = f32(rng.normal(size=(N, 4, 4)))
    step = lambda: P.random_view_cameras(w2c_pred, torch.randint(360, [N]), 25.0, 360)  # (rand_degree drawn on the host, as the reference draws it)
    routes = dict(hip=with_device(True, step), torch=with_device(False, step))
    torch.manual_seed(2)
    a = routes["hip"]()
    torch.manual_seed(2)
    b = routes["torch"]()
    row = compare(routes, args.iters, args.repeats)
    row["max_abs_difference"] = dict(mvp=float((a[0] - b[0]).abs().max()), campos=float((a[2] - b[2]).abs().max()))
    row["kernel_us"] = kernel_us(routes["hip"])
    result[f"random_view_cameras_b{N}"] = row

    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
