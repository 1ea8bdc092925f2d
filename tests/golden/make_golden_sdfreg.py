"""Golden vectors for the SDF sign-agreement regulariser, recorded by IMPORTING the reference (build container only, CPU only).

Run:  python tests/golden/make_golden_sdfreg.py        (needs the reference tree make_golden.py imports; writes tests/golden/sdfreg.npz)

The reference's sdf_bce_reg_loss (model/geometry/dmtet.py:161-169, imported the way make_golden.py imports the reference) is evaluated
in float32 on the finite cases of tests/sdfreg_cases.py: its value, and its gradient with respect to the SDF (left out for the one
large grid, whose value alone is recorded, to keep the file at a few KB).  Only data is written; no reference source travels.  The
cases are rebuilt from tests/sdfreg_cases.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import sdfreg_cases as C  # noqa: E402
from make_golden import import_reference  # noqa: E402

GRADIENT_MAX_VERTICES = 1000


def main():
    cases = {name: C.make_case(name) for name in C.FINITE}  # (built before the reference shadows ``model``)
    import_reference()
    from model.geometry.dmtet import sdf_bce_reg_loss as ref_loss

    data = {}
    for name, case in cases.items():
        for shape in ("1d", "col"):
            sdf = case["sdf"].clone() if shape == "1d" else case["sdf"].clone()[:, None]
            sdf.requires_grad_(True)
            loss = ref_loss(sdf, case["edges"])
            (grad,) = torch.autograd.grad(loss, sdf)
            if shape == "1d":
                data[f"{name}_loss32"] = loss.detach().numpy()
                if sdf.shape[0] <= GRADIENT_MAX_VERTICES:
                    data[f"{name}_grad32"] = grad.numpy()
            else:  # the [Nv,1] form the geometry passes: the same statements, the same bits
                assert np.array_equal(loss.detach().numpy(), data[f"{name}_loss32"]) and grad.shape == sdf.shape
        print(name, "Nv", case["sdf"].shape[0], "Ne", case["edges"].shape[0], float(data[f"{name}_loss32"]))
    path = os.path.join(HERE, "sdfreg.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
