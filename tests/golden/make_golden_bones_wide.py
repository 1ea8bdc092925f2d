"""Golden vectors for estimate_bones on a whole batch of deformed meshes, recorded by IMPORTING the reference (build container only, CPU only).

Run:  python tests/golden/make_golden_bones_wide.py        (needs the reference tree make_golden.py imports; writes tests/golden/bones_wide.npz)

The reference's estimate_bones (model/geometry/skinning.py:50-248, imported the way make_golden.py imports the reference) on B x F = 5 x 8
noisy copies of the V = 386 quadruped -- 40 instances, the regime of the multi-work-group kernels (csrc/bones_wide.hip) -- with 8 body
bones, 4 legs of 3 bones, 'z_minmax_y+', without and with Fauna's bone_y_threshold = 0.4.  Only outputs and seeds are written: the
inputs are regenerated from the seed (tests/bones_wide_cases.py: base); no reference source travels.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import bones_wide_cases as C  # noqa: E402
from make_golden import import_reference  # noqa: E402

SHAPE = (5, 8)


def main():
    seq = C.base(*SHAPE)  # (built before the reference shadows ``model``)
    ref_skin = import_reference()["skin"]
    data = dict(shape=np.array(SHAPE), noise_seed=9, V=seq.shape[2])
    for tag, thr in (("default", None), ("fauna", 0.4)):
        kw = {} if thr is None else dict(bone_y_threshold=thr)
        bones, chain, aux = ref_skin.estimate_bones(seq.clone(), n_body_bones=8, n_legs=4, n_leg_bones=3, body_bones_mode="z_minmax_y+",
                                                    compute_kinematic_chain=True, attach_legs_to_body=True, **kw)
        data[f"{tag}_bones"] = bones.numpy()
        data[f"{tag}_chain"] = np.array(repr(chain))
        data[f"{tag}_leg_body_idx"] = np.array([l["body_bone_idx"] for l in aux["legs"]])
        print(tag, bones.shape, data[f"{tag}_leg_body_idx"])
    path = os.path.join(HERE, "bones_wide.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
