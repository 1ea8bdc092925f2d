"""Named, seeded cases of the keypoint-transfer evaluation, shared by tests/test_keypoints_cpu.py, tests/test_keypoints_gpu.py and
tests/golden/make_golden_keypoints.py.  Every array is float32 (the boxes float64), so what is recorded of the reference is a function
of float32-representable inputs.

Nearest-vertex cases: dict(uv [N,V,2], vis [N,V], kp [N,K,2]), N = 3.
  lattice_*   every coordinate a multiple of 2^-10 in [-2, 2]: the float32 d2 is exact up to 16 (a multiple of 2^-20 below 2^24 of
              them), that is for every vertex that can be the nearest one here; the float32 rule and the float64 reference must
              agree on every index.  coarse_*: multiples of 2^-3 -- thousands of exact ties and duplicate vertices.
  random_*    float32 normals; the seeds are ones for which the float32 rule and the float64 reference choose the same indices
              (checked when the fixture is made and again in the CPU test: a float32 near-tie picking another vertex would be a
              property of the precision, and no fixture may rest on it).
  the named special cases below.
"""
import numpy as np

N = 3
SLAB = 256  # vertices per work-group at N = 3 and every V here (a3d_nearest_visible_vertex_slab; the CPU test asks the library)
VS = (1, 63, 64, 65, 257, 5000)  # 5000: twenty slabs per image
KS = (1, 16, 17)  # 17: a second keypoint tile

LATTICE = [f"{kind}_V{v}_K{k}" for kind in ("lattice", "coarse") for v in VS for k in KS]
RANDOM = ["random_V257_K16", "random_V5000_K17", "random_V65_K1"]
RANDOM_SEEDS = {"random_V257_K16": 1, "random_V5000_K17": 2, "random_V65_K1": 3}
SPECIAL_FINITE = ["duplicates_across_slabs", "only_last_visible", "none_visible", "invisible_is_nearest"]
SPECIAL_NONFINITE = ["nan_keypoint", "nan_vertex", "inf_coordinates"]
FINITE = LATTICE + RANDOM + SPECIAL_FINITE
ALL = FINITE + SPECIAL_NONFINITE


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 32)


def _lattice(rng, shape, step_log2):
    span = 2 << step_log2  # [-2, 2] in steps of 2^-step_log2
    return (rng.integers(-span, span + 1, size=shape) / float(1 << step_log2)).astype(np.float32)


def make_case(name):
    rng = np.random.default_rng(_seed(name))
    if name in LATTICE or name in RANDOM:
        kind, v, k = name.split("_")
        v, k = int(v[1:]), int(k[1:])
        if kind == "random":
            rng = np.random.default_rng(RANDOM_SEEDS[name])
            uv = (0.5 * rng.standard_normal((N, v, 2))).astype(np.float32)
            kp = (0.5 * rng.standard_normal((N, k, 2))).astype(np.float32)
        else:
            bits = 10 if kind == "lattice" else 3
            uv, kp = _lattice(rng, (N, v, 2), bits), _lattice(rng, (N, k, 2), bits)
        vis = (rng.random((N, v)) < 0.6).astype(np.float32)
        if v > 1:
            vis[0, 0] = 0  # (the answer 0 is not the default)
        return dict(uv=uv, vis=vis, kp=kp)
    v, k = 5000, 16
    uv, kp = _lattice(rng, (N, v, 2), 10), _lattice(rng, (N, k, 2), 10)
    vis = np.ones((N, v), np.float32)
    if name == "duplicates_across_slabs":
        # image 0: keypoint j sits ON a vertex that exists twice, in two work-groups' slabs -- the lower index wins; image 1: three
        # copies inside one slab and one wave; image 2: the lower copy is invisible -- the higher one wins
        for j in range(k):
            lo, hi = 10 + j, 10 + j + (1 + j) * SLAB
            uv[0, lo] = uv[0, hi] = kp[0, j]
            uv[1, 300 + 3 * j: 303 + 3 * j] = kp[1, j]
            uv[2, lo] = uv[2, hi] = kp[2, j]
            vis[2, lo] = 0
    elif name == "only_last_visible":
        vis[:] = 0
        vis[:, -1] = 1
    elif name == "none_visible":
        vis[:] = 0
        vis[1, 4000] = 1  # (one image has a visible vertex: nothing leaks between images)
    elif name == "invisible_is_nearest":
        for j in range(k):
            uv[:, 7 + 300 * j] = kp[:, j]  # exactly on the keypoint, and invisible
            vis[:, 7 + 300 * j] = 0
    elif name == "nan_keypoint":
        vis[:, 0] = 0  # even with vertex 0 invisible: inf - NaN is a NaN in every row, argmin gives 0
        kp[0, 3] = np.nan
        kp[1, 5, 1] = np.nan
        kp[2, :, 0] = np.nan
    elif name == "nan_vertex":
        uv[0, 4321, 0] = np.nan
        uv[0, 4700] = np.nan
        uv[1, 100, 1] = np.nan
        vis[1, 100] = 0  # an invisible vertex's coordinates are never read
        uv[2, 300] = np.nan
        uv[2, 255, 1] = np.nan  # the last vertex of the first slab, before the other one
    elif name == "inf_coordinates":
        uv[0, 17] = np.inf  # d2 = +inf: like an invisible vertex
        uv[0, 18, 0] = -np.inf
        kp[1, 2] = np.inf  # inf - x = inf for every finite vertex: all equal, the first VISIBLE vertex ... and inf - inf = NaN for the invisible ones
        vis[1, :5] = 0
        uv[2, 2000] = np.inf
        kp[2, 4] = np.inf  # inf - inf = NaN at vertex 2000
    else:
        raise KeyError(name)
    return dict(uv=uv, vis=vis, kp=kp)


# ---- slabs of more than one trip per thread: the slab grows with N * V (2048 work-groups of 256 threads are aimed at), so these need
# many images.  name -> (N, V, K, trips); lattice coordinates.
TRIPS = {"trips2_N256_V4100_K16": (256, 4100, 16, 2), "trips5_N256_V10300_K17": (256, 10300, 17, 5), "trips32_N1024_V16500_K3": (1024, 16500, 3, 32)}


def make_trips_case(name):
    n, v, k, _ = TRIPS[name]
    rng = np.random.default_rng(_seed(name))
    uv, kp = _lattice(rng, (n, v, 2), 10), _lattice(rng, (n, k, 2), 10)
    vis = (rng.random((n, v)) < 0.6).astype(np.float32)
    # image 0: every keypoint ON two vertices, one per trip of the same thread (the lower index wins); image 1: on the slab's last vertex
    slab = 256 * TRIPS[name][3]
    for j in range(k):
        uv[0, 5 + j] = uv[0, 5 + j + 256] = kp[0, j]
        vis[0, 5 + j] = vis[0, 5 + j + 256] = 1
    uv[1, min(slab, v) - 1] = kp[1, 0]
    vis[1, min(slab, v) - 1] = 1
    return dict(uv=uv, vis=vis, kp=kp)


# ---- the pair stage: N = 6 images, P = 40 pairs (a pair (s, s) among them), K = 16, lattice coordinates
PCK_N, PCK_V, PCK_K, PCK_P = 6, 300, 16, 40
PCK_PAD = 0.05  # the second box_pad_frac recorded (the first is the default 0)


def make_pck_case():
    rng = np.random.default_rng(20261019)
    uv = _lattice(rng, (PCK_N, PCK_V, 2), 10) / 2  # in [-1, 1]
    kp = _lattice(rng, (PCK_N, PCK_K, 2), 10) / 2
    # keypoints near vertices of a common layout, so that a fair share of the transfers lands below the threshold
    layout = rng.integers(0, PCK_V, size=PCK_K)
    for n in range(PCK_N):
        kp[n] = uv[n, layout] + _lattice(rng, (PCK_K, 2), 3) / 32  # (multiples of 2^-8 up to 1/16)
    vis = (rng.random((PCK_N, PCK_V)) < 0.7).astype(np.float32)
    kp_visible = (rng.random((PCK_N, PCK_K)) < 0.8).astype(np.float32)
    kp_visible[:, 0] = 1
    boxes = np.stack([rng.integers(0, 200, PCK_N), rng.integers(0, 200, PCK_N), rng.integers(60, 400, PCK_N), rng.integers(60, 400, PCK_N)], -1).astype(np.float64)
    boxes[1] += 0.5
    pairs = np.stack([rng.integers(0, PCK_N, PCK_P), rng.integers(0, PCK_N, PCK_P)], -1).astype(np.int64)
    pairs[0] = (2, 2)
    pairs[1] = (0, 5)
    return dict(uv=uv.astype(np.float32), vis=vis, kp=kp.astype(np.float32), kp_visible=kp_visible, boxes=boxes, pairs=pairs)
