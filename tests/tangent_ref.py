"""The tangent frame restated for the tests, in whatever dtype the inputs have (the tests call it in float64): the shading normal with
a tangent-space perturbation (reference renderutils/bsdf.py:30-51) and the per-vertex tangents (reference mesh.py:310-350).  Plain
torch, differentiable by autograd; independent of the package.  tests/test_tangent_cpu.py holds it to the reference's recorded float64
outputs and gradients."""
import torch

NORMAL_THRESHOLD = 0.1


def _dot(a, b):
    return (a * b).sum(-1, keepdim=True)


def _normalize(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def shading_normal(pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm, two_sided_shading=True, opengl=True):
    n, t, view = _normalize(smooth_nrm), _normalize(smooth_tng), _normalize(view_pos - pos)
    bt = _normalize(torch.cross(t.expand_as(n + t), n.expand_as(n + t), dim=-1))
    px, py, pz = perturbed_nrm[..., 0:1], perturbed_nrm[..., 1:2], perturbed_nrm[..., 2:3].clamp(min=0.0)
    n = _normalize(t * px - bt * py + n * pz) if opengl else _normalize(t * px + bt * py + n * pz)
    g = geom_nrm
    if two_sided_shading:
        front = _dot(g, view) > 0
        n, g = torch.where(front, n, -n), torch.where(front, g, -g)
    w = (_dot(view, n) / NORMAL_THRESHOLD).clamp(0, 1)
    return g + w * (n - g)


def _safe_normalize(x):
    return x / torch.sqrt(_dot(x, x).clamp(min=1e-20))


def vertex_tangents(v_pos, v_tex, v_nrm, faces, uv_idx, nrm_idx=None):
    """v_pos [B,V,3], v_tex [1|B,Nuv,2], v_nrm [B,V,3], faces / uv_idx / nrm_idx [F,3] int64 -> [B,V,3]."""
    nrm_idx = faces if nrm_idx is None else nrm_idx
    p0, p1, p2 = (v_pos[:, faces[:, i]] for i in range(3))
    t0, t1, t2 = (v_tex[:, uv_idx[:, i]] for i in range(3))
    e1, e2, a, b = t1 - t0, t2 - t0, p1 - p0, p2 - p0
    nom = a * e2[..., 1:2] - b * e1[..., 1:2]
    denom = e1[..., 0:1] * e2[..., 1:2] - e1[..., 1:2] * e2[..., 0:1]
    tang = nom / torch.where(denom > 0, denom.clamp(min=1e-6), denom.clamp(max=-1e-6))
    tang = tang.expand(v_pos.shape[0], -1, -1)
    total, count = torch.zeros_like(v_nrm), torch.zeros_like(v_nrm)
    for i in range(3):
        total = total.index_add(1, nrm_idx[:, i], tang)
        count = count.index_add(1, nrm_idx[:, i], torch.ones_like(tang))
    t = _safe_normalize(total / count)
    return _safe_normalize(t - _dot(t, v_nrm) * v_nrm)
