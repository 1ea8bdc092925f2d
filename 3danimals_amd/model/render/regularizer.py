"""Mesh and texture smoothness losses -- public API of the reference's model/render/regularizer.py (same five names and signatures).

``laplace_regularizer_const``, ``normal_consistency`` and ``avg_edge_length`` of a CUDA float32 mesh run in csrc/regularizer.hip
(ops.laplace_regularizer / ops.normal_consistency / ops.avg_edge_length): atomics-free gathers over the vertex -> face lists the
project already keeps per triangle list, double sums in a fixed order (the same bits on every run), no torch.unique and no host
synchronisation.  CPU, float64 and switched-off (``HIP_REGULARIZERS = False``) inputs take the torch statements below, which are the
reference's, with two differences:

* ``laplace_regularizer_const`` of the reference raises for every input: it scatters an index of shape [B,F,3] into its normaliser
  ``norm`` [B,V,1], which torch refuses.  The evident intent is norm[b,v] = 2 x (number of face corners at v), a [B,F,1] index; that is
  what the statements here and the kernels compute.
* ``device=`` is taken from the input instead of the literal "cuda".

``compute_edge_to_face_mapping`` leaves 0 in a column no face wrote (a boundary edge is paired with face 0) and writes duplicates with
an index put whose winner torch defines on the CPU only (the last write: the highest directed-edge slot 3f + c).  The kernels define
the winner as the CPU's, so the statements on a GPU may differ from them on a non-manifold or inconsistently wound mesh; on the CPU
they agree.  ``get_edge_length`` (per-edge values in torch.unique's order) and ``image_grad`` (one dr.texture call) stay torch
statements.  This module is not part of overlay.MODULES; import it directly.
"""
from __future__ import annotations

import importlib

import torch

from ... import ops
from . import mesh, util

HIP_REGULARIZERS = True  # CUDA float32 inputs through csrc/regularizer.hip (False: always the torch statements)


def _hip_ok(v_pos, t_pos_idx):
    return (HIP_REGULARIZERS and torch.is_tensor(v_pos) and v_pos.is_cuda and v_pos.dtype == torch.float32 and v_pos.dim() == 3
            and torch.is_tensor(t_pos_idx) and t_pos_idx.is_cuda and t_pos_idx.dim() == 3)


def image_grad(buf, std=0.01):
    """The image gradient, useful for kd / ks smoothness losses (reference :19-25)."""
    dr = importlib.import_module(__package__.rsplit(".", 2)[0] + ".shims.nvdiffrast.torch")  # (dr.texture: ops.texture on the GPU)
    dev = buf.device
    t, s = torch.meshgrid(torch.linspace(-1.0 + 1.0 / buf.shape[1], 1.0 - 1.0 / buf.shape[1], buf.shape[1], device=dev),
                          torch.linspace(-1.0 + 1.0 / buf.shape[2], 1.0 - 1.0 / buf.shape[2], buf.shape[2], device=dev), indexing="ij")
    tc = torch.normal(mean=0, std=std, size=(buf.shape[0], buf.shape[1], buf.shape[2], 2), device=dev) + torch.stack((s, t), dim=-1)[None, ...]
    tap = dr.texture(buf, tc, filter_mode="linear", boundary_mode="clamp")
    return torch.abs(tap[..., :-1] - buf[..., :-1]) * tap[..., -1:] * buf[..., -1:]


def _avg_edge_length_torch(v_pos, t_pos_idx):
    return torch.mean(get_edge_length(v_pos, t_pos_idx))


def avg_edge_length(v_pos, t_pos_idx):
    """The average edge length of a mesh: a rough estimate of its tessellation (reference :31-34)."""
    if _hip_ok(v_pos, t_pos_idx):
        return ops.avg_edge_length(v_pos, t_pos_idx)
    return _avg_edge_length_torch(v_pos, t_pos_idx)


def _laplace_regularizer_const_torch(v_pos, t_pos_idx):
    batch_size = v_pos.shape[0]

    term = torch.zeros_like(v_pos)
    norm = torch.zeros_like(v_pos[..., 0:1])

    v0 = v_pos[:, t_pos_idx[0, :, 0], :]
    v1 = v_pos[:, t_pos_idx[0, :, 1], :]
    v2 = v_pos[:, t_pos_idx[0, :, 2], :]

    term.scatter_add_(1, t_pos_idx[..., 0:1].repeat(batch_size, 1, 3), (v1 - v0) + (v2 - v0))
    term.scatter_add_(1, t_pos_idx[..., 1:2].repeat(batch_size, 1, 3), (v0 - v1) + (v2 - v1))
    term.scatter_add_(1, t_pos_idx[..., 2:3].repeat(batch_size, 1, 3), (v0 - v2) + (v1 - v2))

    two = torch.ones_like(v0[..., 0:1]) * 2.0  # ([B,F,1] index and source: the reference's [B,F,3] does not fit norm [B,V,1])
    norm.scatter_add_(1, t_pos_idx[..., 0:1].repeat(batch_size, 1, 1), two)
    norm.scatter_add_(1, t_pos_idx[..., 1:2].repeat(batch_size, 1, 1), two)
    norm.scatter_add_(1, t_pos_idx[..., 2:3].repeat(batch_size, 1, 1), two)

    term = term / torch.clamp(norm, min=1.0)

    return torch.mean(term ** 2)


def laplace_regularizer_const(v_pos, t_pos_idx):
    """Laplacian regularisation with the umbrella operator (reference :40-61; see the module's docstring for the index correction)."""
    if _hip_ok(v_pos, t_pos_idx):
        return ops.laplace_regularizer(v_pos, t_pos_idx)
    return _laplace_regularizer_const_torch(v_pos, t_pos_idx)


def _normal_consistency_torch(v_pos, t_pos_idx):
    v0 = v_pos[:, t_pos_idx[0, :, 0]]
    v1 = v_pos[:, t_pos_idx[0, :, 1]]
    v2 = v_pos[:, t_pos_idx[0, :, 2]]

    face_normals = util.safe_normalize(torch.cross(v1 - v0, v2 - v0, dim=-1))

    tris_per_edge = mesh.compute_edge_to_face_mapping(t_pos_idx)

    n0 = face_normals[:, tris_per_edge[:, 0], :]
    n1 = face_normals[:, tris_per_edge[:, 1], :]

    term = torch.clamp(util.dot(n0, n1), min=-1.0, max=1.0)
    term = (1.0 - term) * 0.5

    return torch.mean(torch.abs(term))


def normal_consistency(v_pos, t_pos_idx):
    """Smooth face normals across the unique edges (reference :66-84)."""
    if _hip_ok(v_pos, t_pos_idx):
        return ops.normal_consistency(v_pos, t_pos_idx)
    return _normal_consistency_torch(v_pos, t_pos_idx)


def get_edge_length(v_pos, t_pos_idx):
    """Per-edge lengths [B,E,1] in torch.unique's order (reference :87-90)."""
    e_pos_idx = mesh.compute_edges(t_pos_idx)
    return util.length(v_pos[:, e_pos_idx[:, 0]] - v_pos[:, e_pos_idx[:, 1]])
