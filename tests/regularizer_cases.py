"""Meshes shared by tests/golden/make_golden_regularizer.py, tests/test_regularizer_cpu.py and tests/test_regularizer_gpu.py:
(v_pos float32 [B,V,3], faces int64 [F,3]) on the CPU.

The six meshes of tangent_cases (closed DMTet meshes with B = 1 and 4, one with an isolated vertex, a tetrahedron, a fan whose hub has
valence 70 and whose 70 rim edges are paired with face 0, a grid patch with 12 boundary edges), and the smallest meshes for what those
do not reach:

'nonmanifold'  three faces on the edge (0,1), two of them running it the same way, and a face flipped against its neighbour across
               (1,2): duplicates in one column of compute_edge_to_face_mapping (the last write wins) and empty second columns.
'repeated'     one face (3,3,4) that lists a vertex twice (a self edge, a zero normal) and one face of three collinear vertices with
               exactly representable coordinates (a zero cross product: the 1e-20 clamp of safe_normalize and its gradient).
'multi_group'  an icosphere, V = 642 (no multiple of 64), F = 1280, B = 2: sums cross work-groups.
'emit_lists'   the marching-tets mesh of the committed dmtet_sphere_r8 fixture, B = 2: on the GPU the same extraction hands the
               kernels its fixed-stride vertex -> face lists.
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tangent_cases as TC  # noqa: E402
import regularizer_ref as R  # noqa: E402

EXTRA_NAMES = ("nonmanifold", "repeated", "multi_group", "emit_lists")
NAMES = TC.MESH_NAMES + EXTRA_NAMES
LOSS_NAMES = ("laplace", "normal_consistency", "avg_edge_length")
EMIT_FIXTURE = "dmtet_sphere_r8.npz"


def icosphere(levels):
    """(unit vertices float64 [V,3], faces int64 [F,3]) of an icosahedron subdivided ``levels`` times, outward winding."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
             (-t, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
             (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(v, dtype=np.float64) / np.linalg.norm(v) for v in verts]
    for _ in range(levels):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]

        nxt = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    return torch.from_numpy(np.stack(verts)), torch.tensor(faces, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """-> dict(v_pos float32 [B,V,3], faces int64 [F,3]); the same tensors on every call (do not modify them)."""
    if name in TC.MESH_NAMES:
        case = TC.make_mesh_case(name)
        return dict(v_pos=case["v_pos"], faces=case["faces"])
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "nonmanifold":
        faces = torch.tensor([[0, 1, 2], [0, 1, 3], [1, 0, 4], [1, 2, 5]])
        return dict(v_pos=torch.randn(2, 6, 3, generator=g), faces=faces)
    if name == "repeated":
        faces = torch.tensor([[0, 1, 2], [2, 1, 3], [3, 3, 4], [4, 5, 6]])
        v_pos = torch.randn(2, 7, 3, generator=g)
        v_pos[:, 4:] = torch.tensor([[2.0, 0.5, -1.0], [3.0, 0.5, -1.0], [4.5, 0.5, -1.0]])  # collinear, exactly
        return dict(v_pos=v_pos, faces=faces)
    if name == "multi_group":
        verts, faces = icosphere(3)
        v_pos = (verts[None] * (1.0 + 0.05 * torch.randn(2, verts.shape[0], 1, generator=g, dtype=torch.float64))).float()
        return dict(v_pos=v_pos, faces=faces)
    assert name == "emit_lists"
    m = TC._golden(EMIT_FIXTURE)
    verts, faces = torch.from_numpy(m["verts"]), torch.from_numpy(m["faces"])
    return dict(v_pos=verts[None] + 0.02 * (torch.rand(2, verts.shape[0], 3, generator=g) - 0.5), faces=faces)


@functools.lru_cache(maxsize=None)
def tables(name):
    """the restatement's (edges, tris_per_edge) of a case"""
    return R.edge_tables(make_case(name)["faces"])


def isolated_vertices(case):
    used = torch.zeros(case["v_pos"].shape[1], dtype=torch.bool)
    used[case["faces"].reshape(-1)] = True
    return ~used


def value_and_grad(fn, v_pos):
    """(loss, d loss / d v_pos) of a scalar loss, detached, on the CPU"""
    v = v_pos.detach().clone().requires_grad_(True)
    loss = fn(v)
    (g,) = torch.autograd.grad(loss, v)
    return loss.detach().cpu(), g.cpu()


@functools.lru_cache(maxsize=None)
def x64(name, loss):
    """(value, gradient) of the float64 restatement; computed once per (case, loss)"""
    case = make_case(name)
    return value_and_grad(lambda v: R.LOSSES[loss](v, case["faces"], tables(name)), case["v_pos"].double())
