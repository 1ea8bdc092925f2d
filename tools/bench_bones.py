"""HIP-event timing of skinning.estimate_bones on batches of deformed meshes: a3d_estimate_bones (csrc/bones_wide.hip for more than 32
instances, csrc/bones.hip's one work-group up to there) against the torch statements of the same commit on the same GPU, host side
included; one JSON line per (shape, mode, chain).

    timeout -k 10 900 python tools/bench_bones.py [--window 0.3] [--repeats 5] [--grid-res 64] [--out FILE]

The meshes are B x F copies of the quadruped extracted by DMTet from the Kuhn grid of --grid-res cells (R = 64: V = 5,720) plus 0.02 *
U(-1, 1) per instance -- what forward_articulation hands to estimate_bones once the instance deformation is on.  Shapes: (20, 10) (the
sequence configuration: 200 meshes per call), (5, 8), (3, 11), and (16, 1) on the one work-group for scale.  Modes: 'z_minmax' and
'z_minmax_y+' with the default quadrants, 'z_minmax_y+' with Fauna's bone_y_threshold = 0.4; 8 body bones, 4 legs of 3 bones.  ``chain``:
``cached`` (compute_kinematic_chain=False: every iteration after the first) or ``rebuilt`` (Fauna: every iteration; one read-back).

``*_us``      a whole call through skinning.estimate_bones: the MEDIAN of ``--repeats`` windows of at least ``--window`` seconds (iteration
              count sized from a probe, after three warm-up calls), the two paths' windows alternating, the fastest window beside it
              (``*_us_min``).  ``hip``: DEVICE_ESTIMATE_BONES and DEVICE_ESTIMATE_BONES_WIDE on; ``torch``: DEVICE_ESTIMATE_BONES off.
``*_syncs``   host synchronisations of one call: torch.cuda.set_sync_debug_mode("warn") warnings.
``max_diff``  the largest difference of the two paths' bones at the timed size.
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

SHAPES = [(20, 10), (5, 8), (3, 11), (16, 1)]
MODES = [("z_minmax", None), ("z_minmax_y+", None), ("z_minmax_y+", 0.4)]


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
    return sum("synchronizing" in str(w.message).lower() and "prototype" not in str(w.message).lower() for w in caught)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid-res", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bones needs the GPU (no CPU timing)"
    a3d = importlib.import_module("3danimals_amd")
    sk = importlib.import_module("3danimals_amd.model.geometry.skinning")
    ops = importlib.import_module("3danimals_amd.ops")
    L = importlib.import_module("3danimals_amd._lib")
    dmtet = importlib.import_module("3danimals_amd.model.geometry.dmtet")
    out_file = open(args.out, "w") if args.out else None

    v, t = a3d.tetgrid.kuhn_grid(args.grid_res)
    pos, tets = (torch.from_numpy(v) * 7.0).cuda(), torch.from_numpy(t).cuda()
    with torch.no_grad():
        verts, _, _, _ = dmtet.DMTet()(pos, a3d.synthetic.quadruped_sdf(pos.cpu()).cuda()[:, None], tets)
    V = verts.shape[0]

    for B, F in SHAPES:
        seq = verts[None, None] + 0.02 * a3d.synthetic.seeded((B, F, V, 3), 9, -1, 1).cuda()
        for mode, thr in MODES:
            kw = dict(n_body_bones=8, n_legs=4, n_leg_bones=3, body_bones_mode=mode, bone_y_threshold=thr)

            def step(hip, rebuild, aux=None):
                prev, sk.DEVICE_ESTIMATE_BONES = sk.DEVICE_ESTIMATE_BONES, hip
                try:
                    if rebuild:
                        return sk.estimate_bones(seq, compute_kinematic_chain=True, **kw)
                    return sk.estimate_bones(seq, compute_kinematic_chain=False, aux=aux, **kw)
                finally:
                    sk.DEVICE_ESTIMATE_BONES = prev

            assert sk.DEVICE_ESTIMATE_BONES_WIDE, "the wide path is switched off (A3D_ESTIMATE_BONES_WIDE=0): nothing to compare"
            (bh, _, aux), (bt, _, _) = step(True, True), step(False, True)
            common = dict(B=B, F=F, V=V, mode=mode, y_threshold=thr, path="wide" if ops.estimate_bones_is_wide(B * F, V) else "one_group",
                          max_diff=float((bh - bt).abs().max()))
            for chain, rebuild in (("cached", False), ("rebuilt", True)):
                row = dict(common, chain=chain)
                counts, windows = {}, {True: [], False: []}
                for hip in (True, False):
                    for _ in range(3):
                        step(hip, rebuild, aux)
                    torch.cuda.synchronize()
                    counts[hip] = max(3, int(args.window * 1e6 / max(window_us(lambda: step(hip, rebuild, aux), 3), 1e-3)) + 1)
                for _ in range(args.repeats):
                    for hip in (True, False):
                        windows[hip].append(window_us(lambda: step(hip, rebuild, aux), counts[hip]))
                for tag, hip in (("hip", True), ("torch", False)):
                    us = sorted(windows[hip])
                    row.update({f"{tag}_us": round(us[len(us) // 2], 1), f"{tag}_us_min": round(us[0], 1),
                                f"{tag}_syncs": count_syncs(lambda: step(hip, rebuild, aux))})
                row["speedup"] = round(row["torch_us"] / row["hip_us"], 2)
                L.poll_deferred()
                text = json.dumps(row)
                print(text, flush=True)
                if out_file:
                    out_file.write(text + "\n")
                    out_file.flush()


if __name__ == "__main__":
    main()
