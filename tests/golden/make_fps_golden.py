"""Golden vectors for farthest-point sampling, recorded by IMPORTING the reference (build container only, CPU only).

Run:  python tests/golden/make_fps_golden.py        (needs the reference tree make_golden.py imports; writes tests/golden/fps_reference.npz)

The reference's sample_farthest_points (model/geometry/util.py:5-27, float32 on the CPU) with torch.randint patched to hand out the
case's first picks, on the inputs of tests/fps_cases.py: the named equality clouds (all V picks), the shuffled 8 x 6 x 5 integer lattice
(all 240 picks: exact distances, ties everywhere) and the two noisy quadrupeds estimate_bones(resample=True) is tested with (V // 4
picks).  Only the picked indices are written: the inputs are regenerated from their seeds; no reference source travels.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import fps_cases as C  # noqa: E402
from make_golden import import_reference  # noqa: E402


def main():
    inputs = {name: (C.cloud(V, seed)[None], [start], V) for name, (V, seed, start) in C.EQUALITY.items()}
    inputs["lattice"] = (C.lattice()[None], [C.LATTICE_START], C.lattice().shape[0])
    quad = C.quadruped()  # (built before the reference shadows ``model``)
    inputs["quadruped"] = (quad.reshape(-1, quad.shape[2], 3), list(C.QUADRUPED_START), quad.shape[2] // 4)
    ref_util = import_reference()["skin"].util
    data = {}
    randint = torch.randint
    try:
        for name, (pts, start, k) in inputs.items():
            torch.randint = lambda n, shape, device=None, _s=start: torch.tensor(_s, dtype=torch.int64)
            out, idx = ref_util.sample_farthest_points(pts.transpose(1, 2).contiguous(), k, return_index=True)
            assert torch.equal(out, pts.transpose(1, 2).gather(2, idx[:, None, :].expand(-1, 3, -1)))
            data[name] = idx.numpy()
            print(name, tuple(pts.shape), k, idx[:, :6].tolist())
    finally:
        torch.randint = randint
    path = os.path.join(HERE, "fps_reference.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
