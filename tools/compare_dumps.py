"""Compare two `bench.py --dump-outputs` folders array by array (two runs, or two builds, of the same arguments):

    python tools/compare_dumps.py DIR_A DIR_B        -> one JSON object on stdout

Per array: element count, max |a - b|, the largest |a| (for scale) and how many elements differ by more than 1e-5.
"""
import json
import os
import sys

import numpy as np


def compare(a_dir, b_dir):
    names = sorted(f[:-4] for f in os.listdir(a_dir) if f.endswith(".npy"))
    missing = sorted(set(f[:-4] for f in os.listdir(b_dir) if f.endswith(".npy")) ^ set(names))
    out = {}
    for n in names:
        if n in missing:
            continue
        a = np.load(os.path.join(a_dir, n + ".npy")).astype(np.float64)
        b = np.load(os.path.join(b_dir, n + ".npy")).astype(np.float64)
        if a.shape != b.shape:
            out[n] = dict(shape_a=list(a.shape), shape_b=list(b.shape))
            continue
        d = np.abs(a - b)
        out[n] = {"n": int(a.size), "max_abs_diff": float(d.max()) if d.size else 0.0, "max_abs": float(np.abs(a).max()) if a.size else 0.0,
                  "n_above_1e-5": int((d > 1e-5).sum())}
    return dict(arrays=out, missing=missing)


if __name__ == "__main__":
    print(json.dumps(compare(sys.argv[1], sys.argv[2])))
