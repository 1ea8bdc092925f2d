"""HIP-event timing of the tangent frame (csrc/tangent.hip) against the torch statements of the same commit on the same GPU; one JSON
line per case.

    timeout -k 10 600 python tools/bench_tangent.py [--window 0.2] [--repeats 5] [--batch 16] [--res 256] [--grid-res 64] [--out FILE]

prepare_shading_normal with a perturbed normal: [B,res,res,3] per-pixel inputs with view_pos [B,1,1,3] (its gradient is reduced inside
the launch), HIP (use_python=False) against the torch statements (use_python=True).  Mesh.v_tng: the quadruped of the canonical bench
scene extracted by DMTet from a Kuhn grid of --grid-res cells, B copies with per-image noise and given normals, HIP_TANGENTS on
against off.  Forward
(no_grad) and forward + backward (every float input requires a gradient).  Each figure is the MEDIAN of ``--repeats`` windows of at
least ``--window`` seconds (iteration count sized from a probe, after three warm-up calls) with the fastest window beside it.
``bytes``: algorithmic -- every input read once, the result written once.
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_bsdf import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--grid-res", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tangent needs the GPU (no CPU timing)"
    a3d = importlib.import_module("3danimals_amd")
    ru = importlib.import_module("3danimals_amd.model.render.renderutils")
    M = importlib.import_module("3danimals_amd.model.render.mesh")
    dmtet = importlib.import_module("3danimals_amd.model.geometry.dmtet")
    out_file = open(args.out, "w") if args.out else None

    def line(**kw):
        text = json.dumps(kw)
        print(text, flush=True)
        if out_file:
            out_file.write(text + "\n")
            out_file.flush()

    def compare(case, fn, ins, extra):
        row = dict(case=case, **extra)
        for tag, hip in (("hip", True), ("torch", False)):
            go = torch.ones_like(fn(hip))

            def fwd():
                with torch.no_grad():
                    fn(hip)

            def both():
                torch.autograd.grad(fn(hip), ins, go)

            f_us, f_min = timed(fwd, args.window, args.repeats)
            a_us, a_min = timed(both, args.window, args.repeats)
            row.update({f"{tag}_fwd_us": f_us, f"{tag}_fwd_us_min": f_min, f"{tag}_fwdbwd_us": a_us, f"{tag}_fwdbwd_us_min": a_min})
        row["speedup_fwd"] = round(row["torch_fwd_us"] / row["hip_fwd_us"], 2)
        row["speedup_fwdbwd"] = round(row["torch_fwdbwd_us"] / row["hip_fwdbwd_us"], 2)
        line(**row)

    gen = torch.Generator(device="cuda").manual_seed(0)
    B, H = args.batch, args.res
    full = lambda: torch.rand(B, H, H, 3, device="cuda", generator=gen).requires_grad_(True)
    ins = [full(), torch.rand(B, 1, 1, 3, device="cuda", generator=gen).requires_grad_(True), full(), full(), full(), full()]
    px = B * H * H
    compare("prepare_shading_normal", lambda hip: ru.prepare_shading_normal(*ins, use_python=not hip), ins,
            dict(shape=[B, H, H], fwd_bytes=4 * (sum(t.numel() for t in ins) + 3 * px)))

    v, t = a3d.tetgrid.kuhn_grid(args.grid_res)
    pos, tets = (torch.from_numpy(v) * 7.0).cuda(), torch.from_numpy(t).cuda()
    with torch.no_grad():
        verts, faces, uvs, uv_idx = dmtet.DMTet()(pos, a3d.synthetic.quadruped_sdf(pos)[:, None], tets)
    V, F = verts.shape[0], faces.shape[0]
    v_pos = (verts[None] + 0.01 * (torch.rand(B, V, 3, device="cuda", generator=gen) - 0.5)).requires_grad_(True)
    v_nrm = M.make_mesh(v_pos.detach(), faces[None], uvs[None].expand(B, -1, -1), uv_idx[None], None).v_nrm.clone().requires_grad_(True)

    def tangents(hip):
        prev, M.HIP_TANGENTS = M.HIP_TANGENTS, hip
        try:
            mesh = M.Mesh(v_pos, faces[None], v_nrm, faces[None], uvs[None].expand(B, -1, -1), uv_idx[None])
            return M.compute_tangents(mesh).v_tng
        finally:
            M.HIP_TANGENTS = prev

    _ = tangents(True)  # (the vertex -> face lists are built once per triangle list)
    compare("Mesh.v_tng", tangents, [v_pos, v_nrm], dict(B=B, V=V, F=F))


if __name__ == "__main__":
    main()
