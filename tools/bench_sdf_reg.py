"""HIP-event timing of sdf_bce_reg_loss (csrc/sdfreg.hip) against the torch statements of the same commit on the same GPU, host side
included; one JSON line per (grid, mode).

    timeout -k 10 900 python tools/bench_sdf_reg.py [--window 0.3] [--repeats 5] [--grid-res 64 128] [--out FILE]

The grid is the Kuhn grid of --grid-res cells at scale 7 (R = 64: Ne = 1,872,064 edges, R = 128: Ne = 14,827,904), the SDF the geometry's
ellipsoid initialisation (0.15 * 7 - |(x, y, z / 2)|) plus N(0, 0.01^2), as [Nv,1] -- what DMTetGeometry.get_sdf_reg_loss passes.  Two
modes through model/geometry/dmtet.py with HIP_SDF_REG on and off: ``fwd`` (the forward alone: what the default configurations, with
weight 0, run every iteration) and ``fwd_bwd`` (the forward and the gradient with respect to the SDF).

``*_us``          a call on an edge tensor the caches know: the MEDIAN of ``--repeats`` windows of at least ``--window`` seconds
                  (iteration count sized from a probe, after three warm-up calls), the two paths' windows alternating, with the fastest
                  window beside it (``*_us_min``).  A window is timed with HIP events around a loop of whole calls, so the host's share
                  (launches, allocations, a read-back where a path has one) is inside it.
``*_syncs``       host synchronisations per call: torch.cuda.set_sync_debug_mode("warn") warnings of one call of that mode.
``first_bwd_us``  the first backward on a fresh edge tensor (int32 rows, index range and the vertex -> (edge, side) list built inside
                  the timed call): one call.
``value_rel`` / ``grad_rel``  the two paths' results at the timed size: |hip - torch| / |torch| of the loss, and the largest gradient
                  difference over the largest gradient magnitude.
"""
import argparse
import importlib
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def count_syncs(fn):
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    # ("called a synchronizing CUDA operation"; not the one-off notice that the debug mode is a prototype feature)
    return sum("synchronizing" in str(w.message).lower() and "prototype" not in str(w.message).lower() for w in caught)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid-res", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sdf_reg needs the GPU (no CPU timing)"
    a3d = importlib.import_module("3danimals_amd")
    M = importlib.import_module("3danimals_amd.model.geometry.dmtet")
    out_file = open(args.out, "w") if args.out else None

    for res in args.grid_res:
        v, t = a3d.tetgrid.kuhn_grid(res)
        pos = (torch.from_numpy(v) * 7.0).cuda()
        topo = M.TetGridTopology(torch.from_numpy(t).cuda(), positions=pos)
        edges = topo.all_edges
        gen = torch.Generator(device="cuda").manual_seed(0)
        x, y, z = pos.unbind(-1)
        sdf = (0.15 * 7.0 - torch.stack([x, y, z / 2], -1).norm(dim=-1, keepdim=True)
               + 0.01 * torch.randn(pos.shape[0], 1, device="cuda", generator=gen)).requires_grad_(True)

        def step(hip, backward, idx=edges):
            prev, M.HIP_SDF_REG = M.HIP_SDF_REG, hip
            try:
                if not backward:
                    with torch.no_grad():
                        return M.sdf_bce_reg_loss(sdf, idx), None
                loss = M.sdf_bce_reg_loss(sdf, idx)
                return loss, torch.autograd.grad(loss, sdf)[0]
            finally:
                M.HIP_SDF_REG = prev

        (lh, gh), (lt, gt) = step(True, True), step(False, True)
        common = dict(grid_res=res, Nv=pos.shape[0], Ne=edges.shape[0],
                      value_rel=float((lh.double() - lt.double()).abs() / lt.double().abs()),
                      grad_rel=float((gh.double() - gt.double()).abs().max() / gt.double().abs().max()))
        for mode, backward in (("fwd", False), ("fwd_bwd", True)):
            row = dict(common, mode=mode)
            counts, windows = {}, {True: [], False: []}
            for hip in (True, False):
                for _ in range(3):
                    step(hip, backward)
                torch.cuda.synchronize()
                counts[hip] = max(3, int(args.window * 1e6 / max(window_us(lambda: step(hip, backward), 3), 1e-3)) + 1)
            for _ in range(args.repeats):
                for hip in (True, False):
                    windows[hip].append(window_us(lambda: step(hip, backward), counts[hip]))
            for tag, hip in (("hip", True), ("torch", False)):
                us = sorted(windows[hip])
                row.update({f"{tag}_us": round(us[len(us) // 2], 1), f"{tag}_us_min": round(us[0], 1),
                            f"{tag}_syncs": count_syncs(lambda: step(hip, backward))})
            row["speedup"] = round(row["torch_us"] / row["hip_us"], 2)
            if backward:
                fresh = edges.clone()
                torch.cuda.synchronize()
                row["first_bwd_us"] = round(window_us(lambda: step(True, True, fresh), 1), 1)
                del fresh
            text = json.dumps(row)
            print(text, flush=True)
            if out_file:
                out_file.write(text + "\n")
                out_file.flush()
        del topo, edges, sdf, pos, lh, gh, lt, gt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
