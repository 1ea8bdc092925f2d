"""HIP-event timing of the image-space derivative kernels (csrc/deriv.hip) beside the torch statements they replace; one JSON line per case.

    timeout -k 10 600 python tools/bench_deriv.py [--mesh quadruped|spiky] [--iters 30]

B = 16 at 256 x 256 on the bench workload's mesh (pipeline.SyntheticScene; --mesh spiky = the trained-like one with long thin triangles):
  a  rast_db alone                                                    ops.rasterize_db        | ops._rasterize_db_torch
  b  interpolate with diff_attrs='all' on a 2-channel uv attribute    ops.interpolate_da      | ops._interpolate_da_torch  (rast_db given)
  c  the whole chain rast_db -> interpolate -> uv_da -> dr.texture of a 1024 x 1024 x 3 trilinear lookup, both ways
each forward (no_grad) and forward + backward, the kernels first and then the torch statements, in the same process.  Times are device events over
``iters`` back-to-back calls after 5 warm-up calls (autograd and launch overhead included: what a caller pays); bytes are what the algorithm
must move at least (per pixel forward: a 16 B texel + 16 B row = 32 B; b 16 B texel + 16 B rast_db + 16 B row = 48 B; backward: a 32 B,
b 64 B; plus the vertex rows once), not what the torch path moves.
The fused single-launch entry (rast_db and out_da straight from clip) was not built.  The first line records the box."""
import argparse
import importlib
import json
import os
import platform
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3danimals_amd", "shims"))


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--mesh", default="quadruped", choices=("quadruped", "spiky"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_deriv needs the GPU (no CPU timing)"
    pipeline = importlib.import_module("3danimals_amd.pipeline")
    ops = importlib.import_module("3danimals_amd.ops")
    ru = importlib.import_module("3danimals_amd.model.render.renderutils")
    dr = importlib.import_module("nvdiffrast.torch")
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(0)
    print(json.dumps(dict(case="box", device=prop.name, arch=getattr(prop, "gcnArchName", ""), cus=prop.multi_processor_count,
                          hip=torch.version.hip, torch=torch.__version__, host=platform.machine(), mesh=args.mesh, iters=args.iters)), flush=True)
    B, H, W = 16, 256, 256
    scene = pipeline.SyntheticScene(grid_res=64, batch=B, resolution=(H, W), device=dev, seed=0, net_width=32, net_layers=3, feat_dim=16,
                                    embedder_freq=4, mesh=args.mesh)
    scene.step(backward=False)
    prior, shape = scene.last["prior"], scene.last["shape"]
    tri = ops.tri_int32(prior.t_pos_idx[0])
    clip = ru.xfm_points(shape.v_pos, scene.mvp).detach().contiguous().requires_grad_(True)
    V, F = clip.shape[1], tri.shape[0]
    rast = ops.rasterize(clip.detach(), tri, (H, W)).contiguous()
    g = torch.Generator(device=dev).manual_seed(0)
    uv_attr = torch.rand(1, V, 2, device=dev, generator=g).requires_grad_(True)
    tex = torch.rand(1, 1024, 1024, 3, device=dev, generator=g).requires_grad_(True)
    gout = torch.rand(B * H * W * 4, device=dev, generator=g)
    n, it = B * H * W, args.iters
    covered = int((rast[..., 3] > 0).sum())

    def fwd_bwd(f, ins):
        def run():
            for t in ins:
                t.grad = None
            out = f()
            out.backward(gout[: out.numel()].view_as(out))
        return run

    def case(name, new, old, ins, fwd_bytes, bwd_bytes):
        with torch.no_grad():
            k_f, t_f = timed(new, it), timed(old, it)
        k_fb, t_fb = timed(fwd_bwd(new, ins), it), timed(fwd_bwd(old, ins), it)
        print(json.dumps(dict(case=name, pixels=n, covered=covered, V=V, F=F, hip_fwd_us=round(k_f, 2), torch_fwd_us=round(t_f, 2),
                              hip_fwd_bwd_us=round(k_fb, 2), torch_fwd_bwd_us=round(t_fb, 2), speedup_fwd=round(t_f / k_f, 2),
                              speedup_fwd_bwd=round(t_fb / k_fb, 2), fwd_bytes=fwd_bytes, fwd_bwd_bytes=fwd_bytes + bwd_bytes,
                              hip_fwd_GBps=round(fwd_bytes / k_f / 1e3, 1))), flush=True)

    case("a_rast_db", lambda: ops.rasterize_db(clip, tri, rast), lambda: ops._rasterize_db_torch(clip, tri, rast), [clip],
         n * 32 + V * B * 16, n * 32 + V * B * 32)
    db = ops.rasterize_db(clip.detach(), tri, rast).requires_grad_(True)
    case("b_interpolate_da_uv", lambda: ops.interpolate_da(uv_attr, rast, tri, db, "all"),
         lambda: ops._interpolate_da_torch(uv_attr, rast, tri, db, "all"), [uv_attr, db], n * 48 + V * 8, n * 64 + V * 16)

    def chain(kernels):
        def run():
            uv = ops.interpolate(uv_attr, rast, tri)
            if kernels:
                da = ops.interpolate_da(uv_attr, rast, tri, ops.rasterize_db(clip, tri, rast), "all")
            else:
                da = ops._interpolate_da_torch(uv_attr, rast, tri, ops._rasterize_db_torch(clip, tri, rast), "all")
            return dr.texture(tex, uv, da, filter_mode="linear-mipmap-linear")
        return run

    case("c_chain_into_texture_1024", chain(True), chain(False), [clip, uv_attr, tex], n * (32 + 48 + 24 + 36), n * (32 + 64 + 24 + 36))


if __name__ == "__main__":
    main()
