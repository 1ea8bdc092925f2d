"""Inputs of the wide estimate_bones tests (tests/test_bones_wide_gpu.py, test_bones_wide_cpu.py, golden/make_golden_bones_wide.py): built
once per process from seeds, never modified by a test (every user clones).

base(B, F)       the V = 386 quadruped of tests/test_gpu_parity.py (quadruped_mesh(16, 0.3)) + 0.02 * seeded((B, F, V, 3), 9, -1, 1)
cloud(N, V)      a seeded point cloud of five clusters per instance, vertex v in cluster v % 5: a body around the z axis and four legs
                 below it, one per top-view quadrant, reaching from next to the axes to well inside the quadrant; the legs of five
                 consecutive vertices share their height, so that the medians of x and z among the low vertices sit between the legs
ties(N, V)       cloud(N, V) with, in every instance, two vertices that share the largest z, two that share the smallest z and two of
                 quadrant 0 that share the lowest y -- the members of a pair differ in their other coordinates and lie a slab of the
                 kernel apart (TIE_PAIRS), so that the first-index rule is settled between work-groups
empty(B, F, n)   base(B, F) with instance n pushed to the +x side: its two -x quadrants hold no vertex
"""
import functools
import importlib

import torch

from conftest import kuhn, seeded

L = importlib.import_module("3danimals_amd._lib")
SLAB = L.EB_WIDE_SLAB
KW = dict(n_body_bones=8, n_legs=4)
MODES = [("z_minmax", None), ("z_minmax_y+", None), ("z_minmax_y+", 0.4)]
SHAPES = [(3, 11), (5, 8), (20, 10)]  # N = 33 is the first size on the wide path
EDGE_V = [1, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 1]
N_EDGE = 33
TIE_V = 2 * SLAB + 1
# (lower index, higher index) of the tied pairs: spine maximum, spine minimum, foot of quadrant 0
TIE_PAIRS = {"z_max": (5, SLAB + 5), "z_min": (10, 2 * SLAB), "foot0": (16, SLAB + 21)}


@functools.lru_cache(maxsize=None)
def quadruped():
    from oracle import dmtet_ref

    synthetic = importlib.import_module("3danimals_amd.synthetic")
    pos, tets = kuhn(16)
    verts, _, _, _ = dmtet_ref.marching_tets(pos, synthetic.quadruped_sdf(pos, leg_radius=0.3), tets)
    return verts


@functools.lru_cache(maxsize=None)
def base(B, F):
    verts = quadruped()
    return verts[None, None] + 0.02 * seeded((B, F, *verts.shape), 9, -1, 1)


@functools.lru_cache(maxsize=None)
def cloud(N, V, seed=21):
    u = seeded((N, 1, V, 3), seed, 0, 1)
    k = (torch.arange(V) % 5)[None, None, :]
    sx = torch.where((k == 1) | (k == 2), 1.0, -1.0)  # legs 1, 2: +x, legs 3, 4: -x
    sz = torch.where((k == 1) | (k == 4), 1.0, -1.0)  # legs 1, 4: +z
    ux, uz = u[..., 0] ** 0.5, u[..., 2] ** 0.5  # (denser towards the outside: a dozen vertices per leg still populate its quadrant)
    uy = u[:, :, (torch.arange(V) // 5) * 5, 1]  # the four legs of a group of five vertices share y: the low vertices are balanced in x and z
    leg = torch.stack([sx * (0.02 + 0.58 * ux), -1.4 + 0.8 * uy, sz * (0.02 + 0.78 * uz)], -1)
    body = torch.stack([-0.1 + 0.2 * u[..., 0], 0.2 + 0.4 * u[..., 1], -1.0 + 2.0 * u[..., 2]], -1)
    return torch.where((k == 0)[..., None], body, leg).contiguous()


@functools.lru_cache(maxsize=None)
def ties(N=N_EDGE, V=TIE_V):
    x = cloud(N, V).clone()
    for j, v in enumerate(TIE_PAIRS["z_max"]):
        x[:, :, v] = torch.tensor([0.05, 0.3 + 0.2 * j, 1.5])
    for j, v in enumerate(TIE_PAIRS["z_min"]):
        x[:, :, v] = torch.tensor([-0.05, 0.5 - 0.2 * j, -1.5])
    for j, v in enumerate(TIE_PAIRS["foot0"]):
        x[:, :, v] = torch.tensor([0.4 + 0.1 * j, -2.0, 0.5 + 0.2 * j])
    return x


@functools.lru_cache(maxsize=None)
def empty(B, F, n):
    x = base(B, F).clone().reshape(B * F, -1, 3)
    x[n, :, 0] = x[n, :, 0].abs() * 0.01 + 0.5
    return x.reshape(B, F, -1, 3)


def new_inputs():
    """(name, input, mode, threshold, n_leg_bones, permutable) of every input these tests construct themselves, for the check that none
    sits on a rounding edge (test_bones_wide_cpu.py).  The tied input is not permuted: the order of its vertices IS the case."""
    out = []
    for V in EDGE_V:
        for mode, thr in (MODES[1:] if V >= 65 else MODES[:2]):
            out.append((f"cloud_V{V}", cloud(N_EDGE, V), mode, thr, 3 if V >= 65 else 0, True))
    for mode, thr in MODES:
        out.append(("ties", ties(), mode, thr, 3, False))
    return out
