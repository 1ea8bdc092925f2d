#!/usr/bin/env python
"""The case matrix of tests/test_render_route_gpu.py as a driver: its launch records and its tensors, under any copy of the package.

  run      every case forward + backward twice; the second run's launch record (entry point + tag, launches; order of first appearance)
           goes to --routes as JSON -- tests/golden/render_routes.json is this, taken under the PARENT commit's package -- and every
           output and gradient of it to --tensors.  --package DIR: import 3danimals_amd from DIR (a `git archive` of another commit; the
           built library comes through A3D_LIB) instead of this tree.  One process, the cases in the order of the matrix.
  compare  --parent A B [more] --this C: every tensor the parent reproduces bit for bit across its two runs must be bit-equal under this commit;
           the others (they receive float atomics) within the bounds of test_every_launch_folding_switch_off_gives_the_same_frames_and_gradients:
           5e-7 on images, rtol 2e-4 and atol 2e-5 of the max-abs on gradients.  Prints the counts; exit status 1 when a tensor misses.

Usage:  A3D_LIB=$PWD/3danimals_amd/lib/liba3d_hip.so python tools/render_routes.py run --package parent_tree --routes routes.json --tensors a.pt
        python tools/render_routes.py compare --parent a.pt b.pt --this c.pt
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(args):
    sys.path.insert(0, os.path.abspath(args.package) if args.package else ROOT)
    pkg = importlib.import_module("3danimals_amd")  # (first: the test modules below put this tree on the path for their own imports)
    assert os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__))) == os.path.abspath(args.package or ROOT), pkg.__file__
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    T = importlib.import_module("test_render_route_gpu")
    L, R = (importlib.import_module("3danimals_amd" + m) for m in ("._lib", ".model.render.render"))
    dev = torch.device("cuda:0")
    scene = T.make_scene(dev)
    routes, tensors = {}, {}
    for name, case in T.CASES.items():
        routes[name], outs, grads = T.launch_record(L, R, scene, case, dev)
        tensors[name] = {"out": {k: v.cpu() for k, v in outs.items()}, "grad": {k: v.cpu() for k, v in grads.items()}}
        print(name, len(routes[name]), "entry points,", sum(n for _, n in routes[name]), "launches", flush=True)
    if args.routes:
        with open(args.routes, "w") as f:
            lines = ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in routes.items())  # (a case per line)
            f.write('{"commit": %s,\n"routes": {\n%s\n}}\n' % (json.dumps(args.commit), lines))
    if args.tensors:
        torch.save(tensors, args.tensors)


def compare(args):
    a, b, *more = (torch.load(p) for p in args.parent)
    c = torch.load(args.this)
    n = dict(compared=0, bit_equal=0, within_bound=0, missed=0)
    for case in a:
        for kind in ("out", "grad"):
            assert a[case][kind].keys() == b[case][kind].keys() == c[case][kind].keys(), (case, kind)
            for key, x in a[case][kind].items():
                y, z = b[case][kind][key], c[case][kind][key]
                n["compared"] += 1
                if torch.equal(x, z) or torch.equal(y, z):
                    n["bit_equal"] += 1
                    continue
                err = float((x - z).abs().max())
                if torch.equal(x, y) and all(torch.equal(x, m[case][kind][key]) for m in more):  # the parent reproduces it: so must this commit
                    ok = False
                elif kind == "out":
                    ok = err <= 5e-7
                else:
                    scale = float(x.abs().max())
                    ok = scale > 0 and bool(((x - z).abs() <= 2e-5 * scale + 2e-4 * x.abs()).all())
                n["within_bound" if ok else "missed"] += 1
                print(f"{'within bound' if ok else 'MISSED'}: {case} {kind} {key}: max abs {err:.3e}; parent against itself "
                      f"{max(float((x - m[case][kind][key]).abs().max()) for m in [b] + more):.3e}")
    print("tensors " + ", ".join(f"{k} {v}" for k, v in n.items()))
    return 1 if n["missed"] else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("run")
    p.add_argument("--package", default=None)
    p.add_argument("--routes", default=None)
    p.add_argument("--tensors", default=None)
    p.add_argument("--commit", default=None, help="what to call the package's commit in the JSON")
    p = sub.add_parser("compare")
    p.add_argument("--parent", nargs="+", required=True, help="two runs of the parent (the rule); further ones narrow what counts as reproduced")
    p.add_argument("--this", required=True)
    a = ap.parse_args()
    sys.exit(run(a) if a.cmd == "run" else compare(a))
