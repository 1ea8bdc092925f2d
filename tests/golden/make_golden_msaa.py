"""Golden vectors for supersampled rendering: the REFERENCE's render_mesh(spp > 1, msaa=True) with the CPU oracle standing in for
nvdiffrast (as in make_golden.py, G7), on the quadruped of render_mesh_e2e.npz.

Run:  python tests/golden/make_golden_msaa.py      (build container only; writes tests/golden/msaa_render_mesh.npz)

Only data is written: inputs, network weights and the reference's outputs, plus -- per case -- the number of blocks whose shading
sample (the top-left one: the nearest-minified raster, render.py:170-171) is uncovered while another sample of the block is covered.
Those blocks are where the reference shades all-zero attributes; the cameras are picked so that every case has at least 8.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from make_golden import import_reference  # noqa: E402  (also injects the oracle as nvdiffrast.torch)

RES = (16, 16)
CASES = {
    "s2_nets": dict(spp=2, modes=["shaded", "dino_pred"], nets=True, kw={}),
    "s4_nets": dict(spp=4, modes=["shaded", "dino_pred"], nets=True, kw={}),
    "s2_flow": dict(spp=2, modes=["shaded", "flow"], nets=False, kw=dict(num_frames=2)),
    "s2_kd": dict(spp=2, modes=["kd", "geo_normal"], nets=True, kw={}),
}


def main():
    import importlib

    synthetic = importlib.import_module("3danimals_amd").synthetic
    R = import_reference()
    from oracle import raster_ref, render_ref

    e2e = np.load(os.path.join(HERE, "render_mesh_e2e.npz"))
    tex = R["mlps"].CoordMLP(3, 9, 3, nf=32, activation="sigmoid", min_max=torch.tensor([[0.0, 1.0]] * 9), n_harmonic_functions=4, extra_feat_dim=16,
                             symmetrize=True)
    dino = R["mlps"].CoordMLP(3, 16, 3, nf=32, activation="sigmoid", min_max=torch.tensor([[0.0, 1.0]] * 16), n_harmonic_functions=4)
    lgt = R["light"].DirectionalLight(16, 3, 32, intensity_min_max=torch.tensor([[0.0, 1.0], [0.5, 1.0]]))
    sd = {}
    for prefix, net in (("tex.", tex), ("dino.", dino), ("lgt.", lgt)):
        net.load_state_dict({k[len(prefix):]: torch.from_numpy(e2e[k]) for k in e2e.files if k.startswith(prefix)}, strict=True)
        sd.update({prefix + k: v.numpy() for k, v in net.state_dict().items()})

    B = 2
    v_pos, prior, faces = torch.from_numpy(e2e["v_pos"][:B]), torch.from_numpy(e2e["prior_v_pos"]), torch.from_numpy(e2e["faces"])
    feat = synthetic.seeded((B, 16), 41, -1, 1)
    bg = synthetic.seeded((B, *RES, 3), 42, 0, 1)

    def null_blocks(mvp, s):
        rast = raster_ref.rasterize(render_ref.xfm_points(v_pos, mvp).contiguous(), faces.int(), (RES[0] * s, RES[1] * s))
        cov = rast[..., 3] > 0
        any_cov = cov.view(B, RES[0], s, RES[1], s).any(dim=4).any(dim=2)
        return int((any_cov & ~cov[:, ::s, ::s]).sum())

    # the first camera seed whose views have >= 8 such blocks at every spp used (a close camera: the animal fills the 16 x 16 frame)
    for seed in range(100, 200):
        mvp, w2c, campos = synthetic.random_cameras(B, seed=seed, cam_z=5.5)
        counts = {s: null_blocks(mvp, s) for s in (2, 4)}
        if min(counts.values()) >= 8:
            break
    else:
        raise SystemExit("no camera seed gives 8 null-sample blocks")
    print("camera seed", seed, "null-sample blocks", counts)

    rmesh, rrender = R["mesh"], R["render"]
    uvs = torch.zeros(1, 4, 2)
    uvi = torch.zeros(1, faces.shape[0], 3, dtype=torch.long)
    shape = rmesh.make_mesh(v_pos, faces[None], uvs.repeat(B, 1, 1), uvi, None)
    prior_mesh = rmesh.make_mesh(prior[None], faces[None], uvs, uvi, None)
    out = dict(v_pos=v_pos.numpy(), prior_v_pos=prior.numpy(), faces=faces.numpy(), mvp=mvp.numpy(), w2c=w2c.numpy(), campos=campos.numpy(),
               feat=feat.numpy(), background=bg.numpy(), resolution=np.array(RES))
    ctx = sys.modules["nvdiffrast.torch"].RasterizeGLContext()
    with torch.no_grad():
        for tag, c in CASES.items():
            n = null_blocks(mvp, c["spp"])
            assert n >= 8, (tag, n)
            outs = rrender.render_mesh(ctx, shape, mvp, w2c, campos, tex if c["nets"] else None, lgt if c["nets"] else None, RES, spp=c["spp"],
                                       num_layers=1, msaa=True, background=bg, bsdf="diffuse", feat=feat if c["nets"] else None,
                                       render_modes=c["modes"], prior_mesh=prior_mesh, dino_net=dino if c["nets"] else None, **c["kw"])
            for m, o in zip(c["modes"], outs):
                assert tuple(o.shape[2:]) == RES
                out[f"{tag}_{m}"] = o.contiguous().numpy()
            out[f"{tag}_modes"] = np.array(",".join(c["modes"]))
            out[f"{tag}_spp"] = np.array(c["spp"])
            out[f"{tag}_nets"] = np.array(c["nets"])
            out[f"{tag}_null_blocks"] = np.array(n)
    np.savez_compressed(os.path.join(HERE, "msaa_render_mesh.npz"), **out, **sd)
    print("wrote msaa_render_mesh.npz", os.path.getsize(os.path.join(HERE, "msaa_render_mesh.npz")), "bytes")


if __name__ == "__main__":
    main()
