"""HIP-event timing of render_mesh(spp > 1, msaa=True) on the fused supersampled route (render.FUSED_MSAA = True, A3D_FUSED_MSAA=1: the covered shading
samples shaded as a point list, ops.msaa_composite_antialias) against the generic path of the same commit (FUSED_MSAA = False: dense
interpolates, nearest up-scales to the full-resolution frame, lerp, dense antialias, avg_pool) in the same process on the same GPU;
one JSON line per case, the box first.

    timeout -k 10 900 python tools/bench_msaa.py [--window 0.3] [--repeats 5] [--out FILE]

Shapes: 'stage1' -- renderer_spp 4, 10 frames of one instance, 256 x 256, modes shaded + dino_pred + flow (the ponymation stage-1
config); 'visualisation' -- spp 4, one image, 256 x 256, shaded.  Fields: hostnets' CoordMLPs and the directional light of the
synthetic scene.  Forward (no_grad) and forward + backward (vertex positions and every network parameter require a gradient).
Each figure is the MEDIAN of ``--repeats`` windows of at least ``--window`` seconds (iteration count sized from a probe, after three
warm-up calls); the two paths' windows ALTERNATE, so that a drift of the clock reaches both; ``_min`` / ``_max`` are the fastest and
slowest window (the run-to-run spread).  ``launches``: device kernels of one forward + backward (torch.profiler); ``host_syncs``:
blocking synchronisations of one forward + backward (torch's sync-debug hook).

The two paths do not compute the same image where a block's shading sample is uncovered while another of its samples is covered
("Supersampled rendering"): the fused route follows the reference there, the generic path composites background.
"""
import argparse
import importlib
import json
import os
import platform
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternating(fns, window, repeats):
    """{tag: (median us, fastest us, slowest us)} of the closures ``fns`` {tag: fn}: window r of every closure before window r + 1 of any."""
    def run(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    count = {}
    for tag, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        count[tag] = max(3, int(window * 1e6 / max(run(fn, 3), 1e-3)) + 1)
    us = {tag: [] for tag in fns}
    for _ in range(repeats):
        for tag, fn in fns.items():
            us[tag].append(run(fn, count[tag]))
    return {tag: (round(sorted(v)[len(v) // 2], 1), round(min(v), 1), round(max(v), 1)) for tag, v in us.items()}


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile

    try:
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(e.count for e in prof.key_averages()))
    except Exception as e:  # (a profiler that cannot start must not cost the line)
        return f"unavailable ({type(e).__name__})"


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum(1 for w in caught if "synchroniz" in str(w.message).lower() and "prototype feature" not in str(w.message))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_msaa needs the GPU (no CPU timing)"
    pipeline = importlib.import_module("3danimals_amd.pipeline")
    render = importlib.import_module("3danimals_amd.model.render.render")
    mesh_mod = importlib.import_module("3danimals_amd.model.render.mesh")
    out_file = open(args.out, "w") if args.out else None

    def line(**kw):
        text = json.dumps(kw)
        print(text, flush=True)
        if out_file:
            out_file.write(text + "\n")
            out_file.flush()

    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(0)
    line(case="box", device=prop.name, arch=getattr(prop, "gcnArchName", ""), cus=prop.multi_processor_count, hip=torch.version.hip,
         torch=torch.__version__, host=platform.machine(), window=args.window, repeats=args.repeats)
    H = args.res
    shapes = {"stage1": dict(frames=10, modes=["shaded", "dino_pred", "flow"]), "visualisation": dict(frames=1, modes=["shaded"])}
    for name, cfg in shapes.items():
        F = cfg["frames"]
        scene = pipeline.SyntheticScene(grid_res=64, batch=1, resolution=(H, H), device=dev, seed=0, num_frames=F,
                                        workload="magicpony" if F == 1 else "ponymation")
        scene.step(backward=False)  # (one step of the canonical scene: its posed meshes are what is rendered below)
        verts = scene.last["shape"].v_pos.detach().clone().requires_grad_(True)
        prior = scene.last["prior"]
        nets = [scene.netTexture, scene.netLight, scene.netDINO]
        params = [verts] + [p for n in nets for p in n.parameters()]
        mvp, w2c, campos, feat, bg = (t.detach() for t in (scene.mvp, scene.w2c, scene.campos, scene.feat, scene.background))

        def render_once(fused):
            was, render.FUSED_MSAA = render.FUSED_MSAA, fused
            try:
                shape = mesh_mod.make_mesh(verts, prior.t_pos_idx, prior.v_tex.expand(verts.shape[0], -1, -1), prior.t_tex_idx, None)
                return render.render_mesh(None, shape, mvp, w2c, campos, nets[0], nets[1], (H, H), spp=args.spp, msaa=True, background=bg,
                                          bsdf="diffuse", feat=feat, render_modes=cfg["modes"], prior_mesh=prior, dino_net=nets[2], num_frames=F)
            finally:
                render.FUSED_MSAA = was

        def fwd(fused):
            def run():
                with torch.no_grad():
                    render_once(fused)
            return run

        def both(fused):
            def run():
                outs = render_once(fused)
                torch.autograd.grad(sum(o.sum() for o in outs), params, allow_unused=True)
            return run

        render_once(True)
        cover = render.LAST_RAST[0][..., 3] > 0
        row = dict(case=name, spp=args.spp, images=F, resolution=[H, H], modes=cfg["modes"], covered_samples=int(cover.sum()),
                   covered_shading_samples=int(cover[:, ::args.spp, ::args.spp].sum()))
        t = alternating({"fused": fwd(True), "generic": fwd(False)}, args.window, args.repeats)
        row.update(fused_fwd_us=t["fused"][0], fused_fwd_us_min=t["fused"][1], fused_fwd_us_max=t["fused"][2], generic_fwd_us=t["generic"][0],
                   generic_fwd_us_min=t["generic"][1], generic_fwd_us_max=t["generic"][2], speedup_fwd=round(t["generic"][0] / t["fused"][0], 2))
        t = alternating({"fused": both(True), "generic": both(False)}, args.window, args.repeats)
        row.update(fused_fwdbwd_us=t["fused"][0], fused_fwdbwd_us_min=t["fused"][1], fused_fwdbwd_us_max=t["fused"][2],
                   generic_fwdbwd_us=t["generic"][0], generic_fwdbwd_us_min=t["generic"][1], generic_fwdbwd_us_max=t["generic"][2],
                   speedup_fwdbwd=round(t["generic"][0] / t["fused"][0], 2))
        row.update(fused_launches=count_launches(both(True)), generic_launches=count_launches(both(False)),
                   fused_host_syncs=count_syncs(both(True)), generic_host_syncs=count_syncs(both(False)))
        line(**row)
        del scene


if __name__ == "__main__":
    main()
