"""Golden vectors for the shading BSDFs and the HDR image loss, recorded by IMPORTING the reference (build container only).

Run:  python tests/golden/make_golden_bsdf.py        (needs /root/reference; writes tests/golden/bsdf_*.npz)

The reference's renderutils/bsdf.py and renderutils/loss.py are pure torch and import on a CPU with nothing stubbed.  For every case the
file holds the float32 inputs (in_0 ..), a fixed upstream gradient (g_out), and the reference's output and input gradients evaluated in
float64 (out64, g64_0 ..) and in float32 (out32, g32_0 ..).  Only data is written; no reference source travels.  Input builders are shared
with the tests (tests/bsdf_cases.py), so the GPU tests can generate larger sets of the same kind.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bsdf_cases as C  # noqa: E402

REF = "/root/reference"


def load(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "model", "render", "renderutils", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def record(path, fn, inputs, g_out):
    data = {"g_out": g_out.numpy()}
    for i, t in enumerate(inputs):
        data[f"in_{i}"] = t.numpy()
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        xs = [t.to(dt).requires_grad_(True) for t in inputs]
        out = fn(*xs)
        gs = torch.autograd.grad(out, xs, g_out.to(dt).reshape(out.shape))
        data["out" + tag] = out.detach().numpy()
        for i, g in enumerate(gs):
            data[f"g{tag}_{i}"] = g.numpy()
    np.savez(os.path.join(HERE, path), **data)
    print(path, os.path.getsize(os.path.join(HERE, path)))


def main():
    B, L = load("bsdf"), load("loss")
    fns = {
        "lambert": B.bsdf_lambert,
        "frostbite_diffuse": B.bsdf_frostbite,
        "pbr_specular": lambda *a: B.bsdf_pbr_specular(*a, min_roughness=0.08),
        "pbr_bsdf_lambert": lambda *a: B.bsdf_pbr(*a, 0.08, 0),
        "pbr_bsdf_frostbite": lambda *a: B.bsdf_pbr(*a, 0.08, 1),
        "_fresnel_shlick": B.bsdf_fresnel_shlick,
        "_ndf_ggx": B.bsdf_ndf_ggx,
        "_lambda_ggx": B.bsdf_lambda_ggx,
        "_masking_smith": B.bsdf_masking_smith_ggx_correlated,
    }
    for name, kind, seed in C.GOLDEN_CASES:
        inputs = C.make_inputs(name, kind, C.GOLDEN_PIXELS, seed)
        out_shape = C.out_shape(name, inputs)
        g_out = torch.randn(out_shape, generator=torch.Generator().manual_seed(1000 + seed))
        record(f"bsdf_{name.lstrip('_')}_{kind}.npz", fns[name], inputs, g_out)
    for loss in C.LOSSES:
        for tm in C.TONEMAPS:
            img, target = C.make_images(C.GOLDEN_PIXELS, 7)
            record(f"bsdf_image_loss_{loss}_{tm}.npz", lambda a, b: L.image_loss_fn(a, b, loss, tm), [img, target], torch.tensor(1.5))


if __name__ == "__main__":
    main()
