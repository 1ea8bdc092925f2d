"""HIP-event timing of render_mesh with the 'depth' / 'tangent' modes on the fused path (render.FUSED_DEPTH_TANGENT = True,
A3D_FUSED_DEPTH_TANGENT: the tangent as the G-buffer launch's extra attribute, the depth computed by the compositor from the G-buffer rows,
ops.depth_composite_antialias) against the generic path of the same commit (FUSED_DEPTH_TANGENT = False: dense interpolates, shade() as
torch launches, lerp, dense antialias -- for EVERY mode of the call) in the same process on the same GPU; one JSON line per case, the box
first.

    timeout -k 10 900 python tools/bench_render_modes.py [--window 0.3] [--repeats 5] [--out FILE]

Cases: modes ['shaded', 'dino_pred', 'depth'] and ['tangent'], each on 16 images and on a single image of 256 x 256, spp 1.  Fields:
hostnets' CoordMLPs and the directional light of the synthetic scene.  Forward (no_grad) and forward + backward (vertex positions and
every network parameter require a gradient).  Each figure is the MEDIAN of ``--repeats`` windows of at least ``--window`` seconds and at
least 30 iterations (iteration count sized from a probe, after three warm-up calls); the two paths' windows ALTERNATE, so that a drift of
the clock reaches both; ``_min`` / ``_max`` are the fastest and slowest window (the run-to-run spread).  ``launches``: device kernels of
one forward + backward (torch.profiler); ``host_syncs``: blocking synchronisations of one forward + backward (torch's sync-debug hook).
"""
import argparse
import importlib
import json
import os
import platform
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_msaa import count_launches, count_syncs  # noqa: E402

MIN_ITERATIONS = 30


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
        count[tag] = max(MIN_ITERATIONS, int(window * 1e6 / max(run(fn, 3), 1e-3)) + 1)
    us = {tag: [] for tag in fns}
    for _ in range(repeats):
        for tag, fn in fns.items():
            us[tag].append(run(fn, count[tag]))
    return {tag: (round(sorted(v)[len(v) // 2], 1), round(min(v), 1), round(max(v), 1)) for tag, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render_modes needs the GPU (no CPU timing)"
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
         torch=torch.__version__, host=platform.machine(), window=args.window, repeats=args.repeats, min_iterations=MIN_ITERATIONS)
    H = args.res
    for B in (16, 1):
        scene = pipeline.SyntheticScene(grid_res=64, batch=B, resolution=(H, H), device=dev, seed=0, num_frames=1, workload="magicpony")
        scene.step(backward=False)  # (one step of the canonical scene: its posed meshes are what is rendered below)
        verts = scene.last["shape"].v_pos.detach().clone().requires_grad_(True)
        prior = scene.last["prior"]
        nets = [scene.netTexture, scene.netLight, scene.netDINO]
        params = [verts] + [p for n in nets for p in n.parameters()]
        mvp, w2c, campos, feat, bg = (t.detach() for t in (scene.mvp, scene.w2c, scene.campos, scene.feat, scene.background))
        # a texture coordinate per vertex (the tangents need an atlas that is not degenerate)
        uvs = torch.rand(1, verts.shape[1], 2, generator=torch.Generator().manual_seed(5)).to(dev)
        for modes in (["shaded", "dino_pred", "depth"], ["tangent"]):
            def render_once(fused):
                was, render.FUSED_DEPTH_TANGENT = render.FUSED_DEPTH_TANGENT, fused
                try:
                    shape = mesh_mod.make_mesh(verts, prior.t_pos_idx, uvs.expand(verts.shape[0], -1, -1), prior.t_pos_idx, None)
                    return render.render_mesh(None, shape, mvp, w2c, campos, nets[0], nets[1], (H, H), spp=1, msaa=False, background=bg,
                                              bsdf="diffuse", feat=feat, render_modes=modes, prior_mesh=prior, dino_net=nets[2], num_frames=1)
                finally:
                    render.FUSED_DEPTH_TANGENT = was

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
            row = dict(case="+".join(modes), images=B, resolution=[H, H], modes=modes, covered_pixels=int(cover.sum()))
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
