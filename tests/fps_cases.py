"""Inputs of the farthest-point-sampling tests (tests/test_fps_cpu.py, test_fps_gpu.py, golden/make_fps_golden.py): built once per process
from seeds, never modified by a test.

cloud(V, seed)     a random anisotropic cloud [V,3] float32: seeded uniform in [-1, 1]^3 scaled by ANISOTROPY
starts(N, V, seed) the first picks int64 [N] of a batch
batch(V, N)        (clouds [N,V,3], starts [N]) of the shape sweep: cloud n of a given V is the same for every N
lattice()          8 x 6 x 5 integer points (coordinates < 64), shuffled: every distance is exact and ties are everywhere
identical(V)       V copies of one point
quadruped()        two noisy V = 386 quadrupeds [1,2,V,3] (tests/bones_wide_cases.py: base), the input of estimate_bones(resample=True)

EQUALITY: the named equality clouds (name -> (V, seed, start)): random clouds with V <= about 1,000 whose float64 greedy run leaves a
relative gap >= GAP_BOUND = 32 eps32 between the best and the second-best candidate at EVERY one of its V picks, so that float32 rounding
(1.75 eps32 per distance, tests/test_fps_gpu.py derives it) cannot decide a pick.  The seeds were chosen so; tests/test_fps_cpu.py
asserts it.  The shape sweep demands equality of every (cloud, k) whose float64 gaps over the first k picks clear the same bound, and
validity of every pick of the others.
"""
import functools

import numpy as np
import torch

from conftest import seeded

EPS32 = float(np.finfo(np.float32).eps)
GAP_BOUND = 32 * EPS32  # 3.8e-6
ANISOTROPY = (1.0, 0.5, 1.6)

# the sweep: wave and work-group edges, then one below, at and one above every size at which csrc/fps.hip changes kernel or points per
# thread (FPS_SMALL_MAX_V = 256; 1024 x {1, 2, 3, 4, 6, 8, 12, 16} points per thread; A3D_FPS_REG_MAX_V = 16384, beyond it the workspace regime)
SWEEP_V = [1, 2, 63, 64, 65, 1023, 1024, 1025]
BOUNDARY_V = [255, 256, 257] + [1024 * p + d for p in (2, 3, 4, 6, 8, 12, 16) for d in (-1, 0, 1)]
BOUNDARY_K_MAX = 256  # (V alone decides the regime; k only lengthens the loop)
SWEEP_N = [1, 3, 40]
VALIDITY = (20000, 5000, 77)  # V, k, seed

EQUALITY = {"v300a": (300, 3000, 160), "v300b": (300, 3001, 180), "v1000a": (1000, 10001, 385), "v1000b": (1000, 10010, 626),
            "v1025a": (1025, 10273, 844), "v1025b": (1025, 10275, 261)}


@functools.lru_cache(maxsize=None)
def cloud(V, seed):
    return (seeded((V, 3), seed, -1, 1) * torch.tensor(ANISOTROPY)).contiguous()


@functools.lru_cache(maxsize=None)
def starts(N, V, seed=5):
    return torch.randint(V, [N], generator=torch.Generator().manual_seed(seed + V), dtype=torch.int64)


def cloud_seed(V, n):
    return 100 * V + n


@functools.lru_cache(maxsize=None)
def batch(V, N):
    return torch.stack([cloud(V, cloud_seed(V, n)) for n in range(N)]), starts(max(SWEEP_N), V)[:N].clone()


def sweep_combos(V):
    """(N, k) of the sweep at V: k in {1, V // 4, V} (those that are >= 1) x N in SWEEP_N; the 40-cloud batches of the large V leave out
    k = V (their float64 references cost seconds otherwise)."""
    ks = sorted({k for k in (1, V // 4, V) if k >= 1})
    out = [(N, k) for N in SWEEP_N for k in ks if k == 1 or N < 40 or V <= 65 or k == V // 4]
    return out


@functools.lru_cache(maxsize=None)
def lattice():
    g = torch.stack(torch.meshgrid(torch.arange(8), torch.arange(6), torch.arange(5), indexing="ij"), -1).reshape(-1, 3).float()
    return g[torch.randperm(g.shape[0], generator=torch.Generator().manual_seed(11))].contiguous()


LATTICE_START = 17


@functools.lru_cache(maxsize=None)
def near_ties(N=4096, seed=31):
    """[N,3,3] float32: cloud n = (origin point, A, B) with B = A moved up by 0, 1 or 2 float32 steps in one coordinate (n % 3 steps, in
    coordinate (n // 3) % 3).  From the start 0 the squared distances of A and B are equal or a few units in the last place apart:
    whether their square roots tie -- and so whether the second pick is A (index 1, the lower) or B -- is decided by the LAST BIT of a
    square root.  A square root that is off by one unit in the last place picks differently in a share of the clouds."""
    p = seeded((N, 3, 3), seed, -1, 1) * torch.tensor(ANISOTROPY)
    a = p[:, 1].numpy().copy()
    n = np.arange(N)
    c = (n // 3) % 3
    for _ in range(2):
        step = np.nextafter(a[n, c], np.float32(4.0))
        a[n, c] = np.where((n % 3) > _, step, a[n, c])
    p[:, 2] = torch.from_numpy(a)
    return p.contiguous()


def identical(V):
    return torch.tensor([0.25, -1.5, 3.0]).repeat(V, 1)


@functools.lru_cache(maxsize=None)
def quadruped():
    import bones_wide_cases as C

    return C.base(1, 2)


QUADRUPED_START = (100, 7)
