"""HIP-event timing of EnvironmentLight.shade as one fused launch each way (csrc/envshade.hip, light.HIP_ENV_SHADE = True) against the
torch statements of the same commit (HIP_ENV_SHADE = False: ~20 element-wise launches, two matmuls and three ops.texture calls) in the
same process on the same GPU; one JSON line per case, the box first.

    timeout -k 10 900 python tools/bench_envshade.py [--window 0.2] [--repeats 5] [--batch 16] [--res 256] [--bases 64 512] [--out FILE]

Frames: [B,res,res] dense, and the covered pixels of the canonical bench scene (its quadruped rasterised at that batch and resolution)
as a [1,1,P] point list with one view_pos row per point, the route render_mesh takes.  Lights: create_trainable_env_rnd(base)
.build_mips() for every --bases entry.  specular False / True, with and without a [1,4,4] lookup transform, view_pos [B,1,1,3] on the
dense frame.  Forward (no_grad) and forward + backward (the four G-buffers and env_base require a gradient); the backward on smooth
normals (a sphere per image: neighbouring pixels share texels, the in-wave merge's best case) and on random normals (its worst).
Each figure is the MEDIAN of ``--repeats`` windows of at least ``--window`` seconds (iteration count sized from a probe, after three
warm-up calls); the two paths' windows ALTERNATE, so that a drift of the clock reaches both.  ``fwd_bytes`` / ``bwd_bytes``:
algorithmic -- every per-pixel input read once, the result (or the four gradients) written once; the maps stay in cache.
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


def alternating(fns, window, repeats):
    """{tag: (median us, fastest us)} of the closures ``fns`` {tag: fn}: window r of every closure before window r + 1 of any."""
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
    return {tag: (round(sorted(v)[len(v) // 2], 1), round(min(v), 1)) for tag, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--bases", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_envshade needs the GPU (no CPU timing)"
    pipeline = importlib.import_module("3danimals_amd.pipeline")
    ops = importlib.import_module("3danimals_amd.ops")
    ru = importlib.import_module("3danimals_amd.model.render.renderutils")
    light = importlib.import_module("3danimals_amd.model.render.light")
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
    B, H = args.batch, args.res
    gen = torch.Generator(device=dev).manual_seed(0)

    # the bench mesh's coverage: the canonical scene's quadruped rasterised at this batch and resolution
    scene = pipeline.SyntheticScene(grid_res=64, batch=B, resolution=(H, H), device=dev, seed=0, net_width=32, net_layers=3, feat_dim=16,
                                    embedder_freq=4)
    scene.step(backward=False)
    clip = ru.xfm_points(scene.last["shape"].v_pos, scene.mvp).detach().contiguous()
    rast = ops.rasterize(clip, ops.tri_int32(scene.last["prior"].t_pos_idx[0]), (H, H))
    cover = rast[..., 3] > 0
    del scene
    line(case="coverage", pixels=B * H * H, covered=int(cover.sum()))

    # G-buffers: a unit sphere per image (smooth normals) or random unit normals; albedo and ks random; the camera in front
    y, x = torch.meshgrid(torch.linspace(-0.9, 0.9, H, device=dev), torch.linspace(-0.9, 0.9, H, device=dev), indexing="ij")
    z = torch.sqrt((1.0 - 0.5 * (x * x + y * y)).clamp(min=0.05))
    sphere = torch.nn.functional.normalize(torch.stack((x, y, z), -1), dim=-1)[None].expand(B, H, H, 3).contiguous()
    rnd = torch.nn.functional.normalize(torch.randn(B, H, H, 3, device=dev, generator=gen), dim=-1)
    pos = (sphere + 0.01 * torch.randn(B, H, H, 3, device=dev, generator=gen)).contiguous()
    kd, ks = torch.rand(B, H, H, 3, device=dev, generator=gen), torch.rand(B, H, H, 3, device=dev, generator=gen)
    view = torch.tensor([0.3, 0.2, 2.5], device=dev) + 0.1 * torch.randn(B, 1, 1, 3, device=dev, generator=gen)
    rot = torch.tensor([[[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]], device=dev)

    def frame(form, normals):
        ins = [pos, sphere if normals == "smooth" else rnd, kd, ks, view]
        if form == "list":
            ins = [t.expand(B, H, H, 3)[cover].reshape(1, 1, -1, 3) for t in ins]
        return [t.detach().clone().requires_grad_(i < 4) for i, t in enumerate(ins)]

    for base in args.bases:
        torch.manual_seed(0)
        lgt = light.create_trainable_env_rnd(base)
        lgt.build_mips()
        lgt.specular = [s.detach().requires_grad_(True) for s in lgt.specular]  # (the shade alone: build_mips' own backward is not timed)
        lgt.diffuse = lgt.diffuse.detach().requires_grad_(True)
        maps = lgt.specular + [lgt.diffuse]
        for form in ("dense", "list"):
            for normals in ("smooth", "random"):
                ins = frame(form, normals)
                px = ins[0].numel() // 3
                go = torch.rand(*ins[0].shape, device=dev, generator=gen)
                for specular in (False, True):
                    for xfm in (False, True):
                        lgt.xfm(rot if xfm else None)

                        def shade(fused):
                            light.HIP_ENV_SHADE = fused
                            try:
                                return lgt.shade(*ins, specular=specular)
                            finally:
                                light.HIP_ENV_SHADE = True

                        def fwd(fused):
                            def run():
                                with torch.no_grad():
                                    shade(fused)
                            return run

                        def both(fused):
                            return lambda: torch.autograd.grad(shade(fused), ins[:4] + maps, go, allow_unused=True)

                        row = dict(case="env_shade", base=base, levels=len(lgt.specular), frame=form, shape=list(ins[0].shape[:3]), normals=normals,
                                   specular=specular, xfm=xfm, fwd_bytes=4 * (sum(t.numel() for t in ins) + 3 * px), bwd_bytes=4 * (sum(t.numel() for t in ins) + 15 * px))
                        if normals == "smooth":  # (the forward does not care which normals)
                            t = alternating({"hip": fwd(True), "torch": fwd(False)}, args.window, args.repeats)
                            row.update(hip_fwd_us=t["hip"][0], hip_fwd_us_min=t["hip"][1], torch_fwd_us=t["torch"][0], torch_fwd_us_min=t["torch"][1],
                                       speedup_fwd=round(t["torch"][0] / t["hip"][0], 2))
                        t = alternating({"hip": both(True), "torch": both(False)}, args.window, args.repeats)
                        row.update(hip_fwdbwd_us=t["hip"][0], hip_fwdbwd_us_min=t["hip"][1], torch_fwdbwd_us=t["torch"][0],
                                   torch_fwdbwd_us_min=t["torch"][1], speedup_fwdbwd=round(t["torch"][0] / t["hip"][0], 2))
                        line(**row)
        lgt.xfm(None)


if __name__ == "__main__":
    main()
