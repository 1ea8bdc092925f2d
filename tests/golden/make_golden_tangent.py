"""Golden vectors for the tangent frame, recorded by IMPORTING the reference (build container only).

Run:  python tests/golden/make_golden_tangent.py        (needs the reference tree make_golden.py imports; writes tests/golden/tangent_*.npz)

bsdf_prepare_shading_normal (renderutils/bsdf.py, pure torch) and compute_tangents (model/render/mesh.py, imported the way
make_golden.py imports the reference) are evaluated on the inputs of tests/tangent_cases.py in float64 and in float32, values and
input gradients for a fixed upstream gradient.  Only data is written; no reference source travels.  The shading-normal files hold the
inputs too (the test checks that the builders still produce them); the mesh file holds outputs only, the meshes are rebuilt from
tests/tangent_cases.py and the committed mesh_*.npz.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import tangent_cases as C  # noqa: E402
from make_golden import import_reference  # noqa: E402
from make_golden_bsdf import load  # noqa: E402


def record_shading_normal(B):
    for kind, two_sided, opengl, seed in C.SN_GOLDEN_CASES:
        inputs = C.make_sn_inputs(kind, C.GOLDEN_PIXELS, seed, opengl)
        g_out = torch.randn(C.sn_out_shape(inputs), generator=torch.Generator().manual_seed(2000 + seed))
        data = {"g_out": g_out.numpy()}
        for i, t in enumerate(inputs):
            data[f"in_{i}"] = t.numpy()
        for tag, dt in (("64", torch.float64), ("32", torch.float32)):
            xs = [t.to(dt).requires_grad_(True) for t in inputs]
            out = B.bsdf_prepare_shading_normal(*xs, two_sided, opengl)
            gs = torch.autograd.grad(out, xs, g_out.to(dt))
            data["out" + tag] = out.detach().numpy()
            for i, g in enumerate(gs):
                data[f"g{tag}_{i}"] = g.numpy()
        path = os.path.join(HERE, f"tangent_sn_{kind}_{int(two_sided)}{int(opengl)}.npz")
        np.savez(path, **data)
        print(path, os.path.getsize(path))


def record_tangents(ref_mesh):
    data = {}
    for name in C.MESH_NAMES:
        case = C.make_mesh_case(name)
        B = case["v_pos"].shape[0]
        w = C.mesh_weights(case)
        for tag, dt in (("64", torch.float64), ("32", torch.float32)):
            v_pos, v_nrm = (case[k].to(dt).requires_grad_(True) for k in ("v_pos", "v_nrm"))
            v_tex = case["v_tex"].to(dt).expand(B, -1, -1)
            m = ref_mesh.Mesh(v_pos, case["faces"][None], v_nrm, case["faces"][None], v_tex, case["uv_idx"][None])
            tng = ref_mesh.compute_tangents(m).v_tng
            keep = ~C.isolated_vertices(case)  # (the isolated vertex is NaN: it takes no part in the gradient)
            g_pos, g_nrm = torch.autograd.grad((tng[:, keep] * w.to(dt)[:, keep]).sum(), [v_pos, v_nrm])
            data[f"{name}_tng{tag}"], data[f"{name}_gpos{tag}"], data[f"{name}_gnrm{tag}"] = tng.detach().numpy(), g_pos.numpy(), g_nrm.numpy()
    path = os.path.join(HERE, "tangent_meshes.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path))


def main():
    record_shading_normal(load("bsdf"))
    record_tangents(import_reference()["mesh"])


if __name__ == "__main__":
    main()
