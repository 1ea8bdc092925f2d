"""HIP-event timing of the keypoint-transfer evaluation (csrc/keypoints.hip, 3danimals_amd/evaluation.py) against what it replaces, in the
same process; one JSON line per size.

    timeout -k 10 900 python tools/bench_keypoints.py [--window 0.1] [--repeats 5] [--out FILE]

Sizes: (N images, V vertices) = (256, 6000), (256, 24000), (2048, 24000); K = 16 keypoints, P = 10000 sampled pairs, rasters of
256 x 256.  Inputs are seeded: vertices uniform in [-1, 1]^2, 60 % visible, keypoints near vertices; the raster buffer is synthetic -- a
disc of 2 x 2-pixel runs of triangle ids over a random triangle list of 2 V rows (neighbouring pixels mostly share a triangle).

``visibility_us``   ops.vertex_visibility (a3d_vertex_visibility_fwd: clear + one thread per pixel), host side included: the MEDIAN of
                    ``--repeats`` windows of at least ``--window`` seconds timed with HIP events around a loop of whole calls (iteration
                    count sized from a probe, after three warm-up calls); the fastest window beside it.  ``visibility_gbs``: the
                    algorithmic bytes (16 per pixel, 4 per cleared vertex) over it.
``nearest_us``      ops.nearest_visible_vertex (a3d_nearest_visible_vertex_fwd), the same way.  ``nearest_gdist_s``: N * V * K
                    distance evaluations over it.
``torch_argmin_us`` the same rule as plain torch statements on the same device (invisible rows set to inf, dx, dy, dx * dx + dy * dy,
                    argmin): [N,K,V] intermediates of ``intermediate_mb`` each.  ``torch_argmin_agree``: share of equal indices
                    (argmin returns SOME smallest index on a tie and does not promise the first; the inputs are tie-free).
``cdist_argmin_us`` torch.cdist in its default matrix-multiply form + argmin, invisible rows moved to 1e4 (an inf turns that form
                    into NaN).  ``cdist_agree``: share of equal indices; that form cancels (|a|^2 + |b|^2 - 2ab), so close
                    candidates may swap.
``pck_us``          evaluation.keypoint_transfer_pck, whole: the nearest-vertex call, the float64 pair stage in torch, its one read-back.
``numpy_100_pairs_us`` / ``numpy_scaled_us``   the reference's per-pair procedure as restated in tests/keypoints_ref.py -- per pair a
                    float64 [K,V] distance matrix, argmin, un-crop, error -- under a host clock on this host for 100 pairs, and that
                    times P / 100: SCALED, not measured at P.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = ((256, 6000), (256, 24000), (2048, 24000))
K, P, SIDE = 16, 10000, 256


def window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def timed(fn, window, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    count = max(3, int(window * 1e6 / max(window_us(fn, 3), 1e-3)) + 1)
    us = sorted(window_us(fn, count) for _ in range(repeats))
    return round(us[len(us) // 2], 1), round(us[0], 1), count


def make_inputs(n, v, seed):
    g = torch.Generator().manual_seed(seed)
    uv = torch.rand(n, v, 2, generator=g) * 2 - 1
    vis = (torch.rand(n, v, generator=g) < 0.6).float()
    layout = torch.randint(0, v, (K,), generator=g)
    kp = uv[:, layout] + (torch.rand(n, K, 2, generator=g) - 0.5) * 0.1
    kp_visible = (torch.rand(n, K, generator=g) < 0.8).float()
    boxes = torch.stack([torch.rand(n, generator=g) * 200, torch.rand(n, generator=g) * 200, 60 + torch.rand(n, generator=g) * 340,
                         60 + torch.rand(n, generator=g) * 340], -1).double()
    pairs = torch.randint(0, n, (P, 2), generator=g)
    return uv, vis, kp, kp_visible, boxes, pairs


def make_raster(n, v, seed, device):
    """A synthetic raster buffer [n,SIDE,SIDE,4] and a triangle list [2v,3]: ids in 2 x 2 runs inside a disc, 0 outside."""
    g = torch.Generator().manual_seed(seed)
    f = 2 * v
    tri = torch.randint(0, v, (f, 3), generator=g, dtype=torch.int32).to(device)
    y, x = torch.meshgrid(torch.arange(SIDE, device=device), torch.arange(SIDE, device=device), indexing="ij")
    inside = ((y - SIDE / 2) ** 2 + (x - SIDE / 2) ** 2) <= (0.4 * SIDE) ** 2
    run = (y // 2) * (SIDE // 2) + x // 2
    img = torch.arange(n, device=device)[:, None, None]
    ids = torch.where(inside[None], (run[None] * 7 + img * 131) % f + 1, torch.zeros((), dtype=torch.long, device=device))
    rast = torch.zeros(n, SIDE, SIDE, 4, device=device)
    rast[..., 3] = ids.float()
    return rast, tri


def numpy_pairs(R, uv, vis, kp, kp_visible, boxes, pairs):
    """The per-pair procedure (evaluate.py:557-587 as restated): float64, a [K,V] matrix per pair."""
    errs, seen = [], []
    for s, t in pairs:
        src = uv[s].astype(np.float64)
        src[vis[s] == 0] = np.inf
        d = np.linalg.norm(src[None, :, :] - kp[s].astype(np.float64)[:, None, :], axis=2)
        idx = np.argmin(d, axis=1)
        pred = R.uncrop(uv[t].astype(np.float64)[idx], boxes[t])
        gt = R.uncrop(kp[t], boxes[t])
        errs.append(np.linalg.norm(gt - pred, axis=-1) / max(boxes[t][2], boxes[t][3]))
        seen.append(kp_visible[s] * kp_visible[t])
    return R.pck(np.stack(errs), np.stack(seen), 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_keypoints needs the GPU (no CPU timing)"
    ops = importlib.import_module("3danimals_amd.ops")
    E = importlib.import_module("3danimals_amd.evaluation")
    L = importlib.import_module("3danimals_amd._lib")
    import keypoints_ref as R

    out_file = open(args.out, "w") if args.out else None
    for n, v in SIZES:
        cpu = make_inputs(n, v, seed=n + v)
        uv, vis, kp, kp_visible, boxes, pairs = (t.cuda() for t in cpu)
        rast, tri = make_raster(n, v, n + v, uv.device)
        row = dict(N=n, V=v, K=K, P=P, H=SIDE, W=SIDE, slab=L.lib().a3d_nearest_visible_vertex_slab(n, v))
        row["workgroups"] = n * -(-v // row["slab"])

        row["visibility_us"], row["visibility_us_min"], row["visibility_calls_per_window"] = timed(lambda: ops.vertex_visibility(rast, tri, v), args.window, args.repeats)
        row["visibility_gbs"] = round((n * SIDE * SIDE * 16 + n * v * 4) / row["visibility_us"] / 1e3, 1)
        row["visible_share"] = round(float(ops.vertex_visibility(rast, tri, v).mean()), 3)

        row["nearest_us"], row["nearest_us_min"], row["nearest_calls_per_window"] = timed(lambda: ops.nearest_visible_vertex(uv, vis, kp), args.window, args.repeats)
        row["nearest_gdist_s"] = round(n * v * K / row["nearest_us"] / 1e3, 1)

        def torch_argmin():  # the rule as plain torch statements: [N,K,V] intermediates
            src = torch.where((vis == 0)[..., None], torch.full_like(uv, float("inf")), uv)
            dx = src[:, None, :, 0] - kp[:, :, None, 0]
            dy = src[:, None, :, 1] - kp[:, :, None, 1]
            return (dx * dx + dy * dy).argmin(-1)

        def cdist_argmin():  # torch.cdist in its default (matrix-multiply) form; invisible rows far away but finite, inf would give NaN
            src = torch.where((vis == 0)[..., None], torch.full_like(uv, 1e4), uv)
            return torch.cdist(kp, src).argmin(-1)

        mine = ops.nearest_visible_vertex(uv, vis, kp)
        row["torch_argmin_us"], row["torch_argmin_us_min"], _ = timed(torch_argmin, args.window, args.repeats)
        row["torch_argmin_agree"] = round(float((torch_argmin() == mine).float().mean()), 6)
        row["cdist_argmin_us"], row["cdist_argmin_us_min"], _ = timed(cdist_argmin, args.window, args.repeats)
        row["cdist_agree"] = round(float((cdist_argmin() == mine).float().mean()), 6)
        row["nearest_equal_after_the_loops"] = bool(torch.equal(ops.nearest_visible_vertex(uv, vis, kp), mine))
        row["intermediate_mb"] = round(n * K * v * 4 / 2 ** 20, 1)

        row["pck_us"], row["pck_us_min"], _ = timed(lambda: E.keypoint_transfer_pck(uv, vis, kp, kp_visible, boxes, pairs), args.window, args.repeats)
        pck = E.keypoint_transfer_pck(uv, vis, kp, kp_visible, boxes, pairs)[0]
        row["pck"] = round(pck, 6)

        arrays = [t.numpy() for t in cpu]
        t0 = time.perf_counter()
        numpy_pairs(R, *arrays[:5], arrays[5][:100])
        row["numpy_100_pairs_us"] = round((time.perf_counter() - t0) * 1e6, 1)
        row["numpy_scaled_us"] = round(row["numpy_100_pairs_us"] * P / 100, 1)
        row["numpy_scaled_note"] = f"100 pairs measured on this host, times {P // 100}: scaled, not measured"
        text = json.dumps(row)
        print(text, flush=True)
        if out_file:
            out_file.write(text + "\n")
            out_file.flush()
        del uv, vis, kp, rast, tri
        torch.cuda.empty_cache()
    L.poll_deferred()
    if out_file:
        out_file.close()


if __name__ == "__main__":
    main()
