"""Golden vectors for the mesh regularisers, recorded by IMPORTING the reference (build container only, CPU only).

Run:  python tests/golden/make_golden_regularizer.py        (needs the reference tree make_golden.py imports; writes tests/golden/regularizer.npz)

The reference's model/render/regularizer.py and mesh.py (imported the way make_golden.py imports the reference, .cuda() a no-op) are
evaluated in float32 on every mesh of tests/regularizer_cases.py: normal_consistency, avg_edge_length, get_edge_length, compute_edges
and compute_edge_to_face_mapping.  laplace_regularizer_const is asserted to raise RuntimeError on every mesh (its [B,F,3] index does not
fit its [B,V,1] normaliser), so there is nothing of it to record.  Only data is written; no reference source travels.  The meshes are
rebuilt from tests/regularizer_cases.py and the committed fixtures.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import regularizer_cases as C  # noqa: E402
from make_golden import import_reference  # noqa: E402


def main():
    ref_mesh = import_reference()["mesh"]
    from model.render import regularizer as ref_reg

    data = {}
    for name in C.NAMES:
        case = C.make_case(name)
        v_pos, tri = case["v_pos"], case["faces"][None]
        try:
            ref_reg.laplace_regularizer_const(v_pos, tri)
        except RuntimeError as e:
            assert "Expected index" in str(e), e
        else:
            raise AssertionError("the reference's laplace_regularizer_const no longer raises: record it")
        data[f"{name}_nc32"] = ref_reg.normal_consistency(v_pos, tri).numpy()
        data[f"{name}_ael32"] = ref_reg.avg_edge_length(v_pos, tri).numpy()
        data[f"{name}_gel32"] = ref_reg.get_edge_length(v_pos, tri).numpy()
        data[f"{name}_edges"] = ref_mesh.compute_edges(tri).numpy().astype(np.int32)
        data[f"{name}_tris_per_edge"] = ref_mesh.compute_edge_to_face_mapping(tri).numpy().astype(np.int32)
        print(name, "V", v_pos.shape[1], "F", tri.shape[1], "E", data[f"{name}_edges"].shape[0], float(data[f"{name}_nc32"]), float(data[f"{name}_ael32"]))
    path = os.path.join(HERE, "regularizer.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
