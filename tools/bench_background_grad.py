"""HIP-event timing of render_mesh forward + backward with a background that REQUIRES GRAD: the fused compositor returning the
background's gradient (render.FUSED_BACKGROUND_GRAD = True, A3D_FUSED_BACKGROUND_GRAD=1: a3d_ca_buffer.g_null at spp 1) against what such a call
takes with the switch off, the default (the covered-point path with the torch compositor -- a background fill, an index_copy, a
stand-alone antialias per image and autograd's dense adjoints of all three) in the same process on the same GPU; one JSON line per case,
the box first.

    timeout -k 10 900 python tools/bench_background_grad.py [--window 0.3] [--repeats 5] [--out FILE]

Cases: modes ['shaded', 'dino_pred'] on 16 images and on a single image of 256 x 256, spp 1, a background per image [B,H,W,3].  Fields:
hostnets' CoordMLPs and the directional light of the synthetic scene.  Forward + backward: the background, the vertex positions and every
network parameter require a gradient (a forward-only figure is given beside it: with grad enabled, as the switch only matters then).
Each figure is the MEDIAN of ``--repeats`` windows of at least ``--window`` seconds and at least 30 iterations (tools/bench_render_modes.py's
``alternating``: the two paths' windows alternate, so that a drift of the clock reaches both); ``_min`` / ``_max`` are the fastest and
slowest window.  ``launches`` / ``host_syncs``: device kernels and blocking synchronisations of one forward + backward.
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
from bench_render_modes import MIN_ITERATIONS, alternating  # noqa: E402

MODES = ["shaded", "dino_pred"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_background_grad needs the GPU (no CPU timing)"
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
        bg = torch.rand(B, H, H, 3, generator=torch.Generator().manual_seed(7)).to(dev).requires_grad_(True)
        params = [bg, verts] + [p for n in nets for p in n.parameters()]
        mvp, w2c, campos, feat = (t.detach() for t in (scene.mvp, scene.w2c, scene.campos, scene.feat))
        uvs = torch.rand(1, verts.shape[1], 2, generator=torch.Generator().manual_seed(5)).to(dev)
        routes = {}

        def render_once(fused):
            was, render.FUSED_BACKGROUND_GRAD = render.FUSED_BACKGROUND_GRAD, fused
            try:
                shape = mesh_mod.make_mesh(verts, prior.t_pos_idx, uvs.expand(verts.shape[0], -1, -1), prior.t_pos_idx, None)
                r = render._plan_route(MODES, shape, w2c, (H, H), 1, 1, False, bg, nets[0], nets[1], nets[2], mtx=mvp, num_frames=1)
                routes[fused] = f"{r.path}{'+compositor' if r.composite else ''}"
                return render.render_mesh(None, shape, mvp, w2c, campos, nets[0], nets[1], (H, H), spp=1, msaa=False, background=bg,
                                          bsdf="diffuse", feat=feat, render_modes=MODES, prior_mesh=prior, dino_net=nets[2], num_frames=1)
            finally:
                render.FUSED_BACKGROUND_GRAD = was

        def fwd(fused):
            return lambda: render_once(fused)

        def both(fused):
            def run():
                outs = render_once(fused)
                torch.autograd.grad(sum(o.sum() for o in outs), params, allow_unused=True)
            return run

        render_once(True)
        cover = render.LAST_RAST[0][..., 3] > 0
        row = dict(case="+".join(MODES) + ", background requires grad", images=B, resolution=[H, H], modes=MODES, covered_pixels=int(cover.sum()))
        t = alternating({"fused": both(True), "generic": both(False)}, args.window, args.repeats)
        row.update(fused_fwdbwd_us=t["fused"][0], fused_fwdbwd_us_min=t["fused"][1], fused_fwdbwd_us_max=t["fused"][2],
                   generic_fwdbwd_us=t["generic"][0], generic_fwdbwd_us_min=t["generic"][1], generic_fwdbwd_us_max=t["generic"][2],
                   speedup_fwdbwd=round(t["generic"][0] / t["fused"][0], 2))
        t = alternating({"fused": fwd(True), "generic": fwd(False)}, args.window, args.repeats)
        row.update(fused_fwd_us=t["fused"][0], fused_fwd_us_min=t["fused"][1], fused_fwd_us_max=t["fused"][2], generic_fwd_us=t["generic"][0],
                   generic_fwd_us_min=t["generic"][1], generic_fwd_us_max=t["generic"][2], speedup_fwd=round(t["generic"][0] / t["fused"][0], 2))
        row.update(fused_route=routes[True], generic_route=routes[False], fused_launches=count_launches(both(True)),
                   generic_launches=count_launches(both(False)), fused_host_syncs=count_syncs(both(True)), generic_host_syncs=count_syncs(both(False)))
        line(**row)
        del scene


if __name__ == "__main__":
    main()
