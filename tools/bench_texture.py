"""HIP-event timing of dr.texture (csrc/texture.hip) at four shapes; one JSON line per case.

    timeout -k 10 300 python tools/bench_texture.py [--iters 50]

  a  2-D linear, B = 16, 256 x 256 lookups, 512 x 512 x 3 texture, forward and forward + backward, beside the shim's torch tap:
     uniformly random uv (no two neighbouring lookups share a texel: the scatter's worst case) and a smooth uv field (each image a
     rotated, scaled view of the texture, 0.8 texels per lookup step: what a rasterised surface hands over)
  b  2-D trilinear with uv_da (internal stack), 1024 x 1024 x 3 base, B = 16, 256 x 256 lookups
  c  cube trilinear with a bias over a 6 x 512 x 512 x 3 stack (the EnvironmentLight shape), B = 16, 256 x 256 lookups
  d  mip construction (a3d_texture_mip_fwd) of 2048 x 2048 x 4

Bytes are what the algorithm must move at least: uv (+ uv_da, bias) read and the output written per lookup, the texture's texels read
once (forward); backward adds g_out read, g_uv (+ ...) written and the level gradients read-modified-written once.  Bytes / kernel time
is reported as GB/s; the forward with every tap from cache is bounded by those bytes, the backward by its atomics.
"""
import argparse
import importlib
import json
import os
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
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_texture needs the GPU (no CPU timing)"
    ops = importlib.import_module("3danimals_amd.ops")
    dr = importlib.import_module("nvdiffrast.torch")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    B, H, W = 16, 256, 256
    n = B * H * W
    it = args.iters

    def line(case, **kw):
        print(json.dumps(dict(case=case, **kw)), flush=True)

    def fwd_bwd(f, ins):
        def run():
            for t in ins:
                t.grad = None
            out = f()
            out.backward(gout[: out.numel()].view_as(out))
        return run

    gout = torch.rand(n * 4, device=dev, generator=g)
    # (a) 2-D linear
    tex = torch.rand(1, 512, 512, 3, device=dev, generator=g).requires_grad_(True)
    uv = torch.rand(B, H, W, 2, device=dev, generator=g).requires_grad_(True)
    fb = n * (8 + 12) + tex.numel() * 4
    bb = fb + n * (12 + 8) + tex.numel() * 8
    with torch.no_grad():
        hip_f = timed(lambda: ops.texture(tex, uv, filter_mode="linear", boundary_mode="wrap"), it)
        tap_f = timed(lambda: dr._torch_tap(tex, uv, "linear", "wrap"), it)
    hip_fb = timed(fwd_bwd(lambda: ops.texture(tex, uv, filter_mode="linear", boundary_mode="wrap"), [tex, uv]), it)
    tap_fb = timed(fwd_bwd(lambda: dr._torch_tap(tex, uv, "linear", "wrap"), [tex, uv]), it)
    line("a_2d_linear_random_uv", lookups=n, texture=[512, 512, 3], hip_fwd_us=round(hip_f, 2), torch_tap_fwd_us=round(tap_f, 2),
         hip_fwd_bwd_us=round(hip_fb, 2), torch_tap_fwd_bwd_us=round(tap_fb, 2), speedup_fwd=round(tap_f / hip_f, 2),
         speedup_fwd_bwd=round(tap_fb / hip_fb, 2), hip_fwd_GBps=round(fb / hip_f / 1e3, 1), hip_fwd_bwd_GBps=round(bb / hip_fb / 1e3, 1))
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32) / H, torch.arange(W, device=dev, dtype=torch.float32) / W,
                            indexing="ij")
    ang = torch.arange(B, device=dev, dtype=torch.float32)[:, None, None] * 0.37
    smooth = torch.stack([0.4 * (xx * torch.cos(ang) - yy * torch.sin(ang)) + 0.3, 0.4 * (xx * torch.sin(ang) + yy * torch.cos(ang)) + 0.2], -1)
    uv_s = smooth.contiguous().requires_grad_(True)
    with torch.no_grad():
        hip_f = timed(lambda: ops.texture(tex, uv_s, filter_mode="linear", boundary_mode="wrap"), it)
        tap_f = timed(lambda: dr._torch_tap(tex, uv_s, "linear", "wrap"), it)
    hip_fb = timed(fwd_bwd(lambda: ops.texture(tex, uv_s, filter_mode="linear", boundary_mode="wrap"), [tex, uv_s]), it)
    tap_fb = timed(fwd_bwd(lambda: dr._torch_tap(tex, uv_s, "linear", "wrap"), [tex, uv_s]), it)
    line("a_2d_linear_smooth_uv", lookups=n, texture=[512, 512, 3], hip_fwd_us=round(hip_f, 2), torch_tap_fwd_us=round(tap_f, 2),
         hip_fwd_bwd_us=round(hip_fb, 2), torch_tap_fwd_bwd_us=round(tap_fb, 2), speedup_fwd=round(tap_f / hip_f, 2),
         speedup_fwd_bwd=round(tap_fb / hip_fb, 2))
    # (b) 2-D trilinear with uv_da over the internal stack (its construction and backward included)
    tex = torch.rand(1, 1024, 1024, 3, device=dev, generator=g).requires_grad_(True)
    da = ((torch.rand(B, H, W, 4, device=dev, generator=g) - 0.5) * (4.0 / 1024)).requires_grad_(True)
    texels = tex.numel() * 4 / 3
    fb = n * (8 + 16 + 12) + texels * 4 * 2
    bb = fb + n * (12 + 8 + 16) + texels * 4 * 3
    f = lambda: ops.texture(tex, uv, uv_da=da, filter_mode="linear-mipmap-linear")
    with torch.no_grad():
        t_f = timed(f, it)
    t_fb = timed(fwd_bwd(f, [tex, uv, da]), it)
    line("b_2d_trilinear_uv_da", lookups=n, texture=[1024, 1024, 3], fwd_us=round(t_f, 2), fwd_bwd_us=round(t_fb, 2),
         fwd_GBps=round(fb / t_f / 1e3, 1), fwd_bwd_GBps=round(bb / t_fb / 1e3, 1))
    # (c) cube trilinear with a bias over a custom stack (EnvironmentLight.shade's specular lookup)
    spec = [torch.rand(1, 6, 512 >> k, 512 >> k, 3, device=dev, generator=g).requires_grad_(True) for k in range(6)]
    d = torch.randn(B, H, W, 3, device=dev, generator=g).requires_grad_(True)
    bias = (torch.rand(B, H, W, device=dev, generator=g) * 5).requires_grad_(True)
    texels = sum(s.numel() for s in spec)
    fb = n * (12 + 4 + 12) + texels * 4
    bb = fb + n * (12 + 12 + 4) + texels * 8
    f = lambda: ops.texture(spec[0], d, mip=spec[1:], mip_level_bias=bias, filter_mode="linear-mipmap-linear", boundary_mode="cube")
    with torch.no_grad():
        t_f = timed(f, it)
    t_fb = timed(fwd_bwd(f, spec + [d, bias]), it)
    line("c_cube_trilinear_bias", lookups=n, texture=[6, 512, 512, 3], fwd_us=round(t_f, 2), fwd_bwd_us=round(t_fb, 2),
         fwd_GBps=round(fb / t_f / 1e3, 1), fwd_bwd_GBps=round(bb / t_fb / 1e3, 1))
    # (d) mip construction
    tex = torch.rand(1, 2048, 2048, 4, device=dev, generator=g)
    sizes = ops.texture_mip_sizes(2048, 2048)
    byts = sum(h * w * 4 * 4 for h, w in sizes[:-1]) + sum(h * w * 4 * 4 for h, w in sizes[1:])
    with torch.no_grad():
        t_m = timed(lambda: ops.texture_construct_mip(tex), it)
    line("d_mip_construct", texture=[2048, 2048, 4], levels=len(sizes), us=round(t_m, 2), GBps=round(byts / t_m / 1e3, 1))


if __name__ == "__main__":
    main()
