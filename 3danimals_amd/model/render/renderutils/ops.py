"""``use_python`` is accepted for signature parity (reference default False = its JIT CUDA plugin, which does not exist on this
platform); both values take the torch path below -- the one every config of the reference selects (render.py:72,278).
The two cube-map prefilters (diffuse_cubemap, specular_cubemap) exist in the reference ONLY inside that plugin (its use_python
branch is ``assert False``): here both values of ``use_python`` run the HIP kernels of csrc/envlight.hip."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from ...._lib import fp32_region

NORMAL_THRESHOLD = 0.1  # reference renderutils/bsdf.py:13
HIP_XFM_POINTS = True  # xfm_points on the GPU as a3d_xfm_points_fwd / _bwd (False: the padded torch matmul, e.g. for double precision)


def _dot(x, y):
    return torch.sum(x * y, -1, keepdim=True)


def _hip_xfm_ok(points, matrix):
    if not (HIP_XFM_POINTS and points.is_cuda and matrix.is_cuda and points.dtype == torch.float32 and matrix.dtype == torch.float32):
        return False
    if points.dim() != 3 or matrix.dim() != 3 or points.shape[2] != 3 or tuple(matrix.shape[1:]) != (4, 4):
        return False
    b = max(points.shape[0], matrix.shape[0])
    return points.shape[0] in (1, b) and matrix.shape[0] in (1, b)


@fp32_region
def xfm_points(points, matrix, use_python=False):
    """[B|1,V,3] x [B,4,4] -> homogeneous [B,V,4] = [p,1] . M^T (reference ops.py:524-525).

    One padded batched matmul (rocBLAS); autograd reaches both the points and the matrix (camera pose).
    """
    if _hip_xfm_ok(points, matrix):
        from .... import ops  # one launch each way (csrc/xfm.hip) instead of pad + bmm, and two more bmm + a slice backward

        out = ops.xfm_points(points, matrix)
    else:
        out = torch.matmul(F.pad(points, pad=(0, 1), mode="constant", value=1.0), torch.transpose(matrix, 1, 2))
    if torch.is_anomaly_enabled():
        assert torch.all(torch.isfinite(out)), "Output of xfm_points contains inf or NaN"
    return out


@fp32_region
def xfm_vectors(vectors, matrix, use_python=False):
    """Direction transform (w = 0), reference ops.py:533-549."""
    out = torch.matmul(F.pad(vectors, pad=(0, 1), mode="constant", value=0.0), torch.transpose(matrix, 1, 2))[..., 0:3].contiguous()
    if torch.is_anomaly_enabled():
        assert torch.all(torch.isfinite(out)), "Output of xfm_vectors contains inf or NaN"
    return out


def prepare_shading_normal(pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm, two_sided_shading=True, opengl=True,
                           use_python=False):
    """Final shading normal (reference ops.py:194-227 -> bsdf.py:46-51): optional tangent-space perturbation,
    two-sided flip by the geometric normal, bend toward the geometric normal at grazing view angles.

    The hot path passes perturbed_nrm=None (render.py:71), for which the tangent frame cancels exactly and
    ``smooth_tng`` is not touched (so it may be None).
    """
    n = F.normalize(smooth_nrm, dim=-1)
    view = F.normalize(view_pos - pos, dim=-1)
    if perturbed_nrm is not None:
        t = F.normalize(smooth_tng, dim=-1)
        bt = F.normalize(torch.cross(t, n, dim=-1), dim=-1)
        sign = -1.0 if opengl else 1.0
        n = F.normalize(t * perturbed_nrm[..., 0:1] + sign * bt * perturbed_nrm[..., 1:2] + n * torch.clamp(perturbed_nrm[..., 2:3], min=0.0),
                        dim=-1)
    else:
        n = F.normalize(n, dim=-1)  # (0,0,1) perturbation: n*1, re-normalised (bsdf.py:38-44)
    g = geom_nrm
    if two_sided_shading:
        front = _dot(g, view) > 0
        n = torch.where(front, n, -n)
        g = torch.where(front, g, -g)
    t = torch.clamp(_dot(view, n) / NORMAL_THRESHOLD, min=0, max=1)
    out = torch.lerp(g, n, t)
    if torch.is_anomaly_enabled():
        assert torch.all(torch.isfinite(out)), "Output of prepare_shading_normal contains inf or NaN"
    return out


def diffuse_cubemap(cubemap, use_python=False):
    """Cosine-lobe irradiance map of a [6,N,N,3] cube map (reference ops.py:404-411); ops.diffuse_cubemap states the arithmetic."""
    from .... import ops

    out = ops.diffuse_cubemap(cubemap)
    if torch.is_anomaly_enabled():
        assert torch.all(torch.isfinite(out)), "Output of diffuse_cubemap contains inf or NaN"
    return out


NDF_SAMPLES = 1000000
NDF_CACHE_SIZE = 32  # entries kept (least recently used dropped): a 512-base light holds 6, a table at N = 512 is 75 MB of device memory
_ndf_cutoff_cache = OrderedDict()  # (roughness, cutoff) -> cosine
_ndf_bounds_cache = OrderedDict()  # (N, roughness, cutoff, device) -> (cosine, bounds table)


def clear_specular_cache():
    """Drop the cached cutoff cosines and bounds tables (they are rebuilt on the next use)."""
    _ndf_cutoff_cache.clear()
    _ndf_bounds_cache.clear()


def _lru(cache, key, make):
    if key in cache:
        cache.move_to_end(key)
        return cache[key]
    cache[key] = make()
    while len(cache) > NDF_CACHE_SIZE:
        cache.popitem(last=False)
    return cache[key]


def ndf_cutoff_cosine(roughness, cutoff):
    """Cosine of the cone that holds ``cutoff`` of the GGX lobe, by the reference's rule (ops.py:428-443): D(roughness^4, cos t) summed
    over 1,000,000 equally spaced angles t in [0, pi/2]; the first angle whose running sum reaches ``cutoff`` of the total."""
    def make():
        a2 = float(roughness) ** 4
        cos_t = np.clip(np.cos(np.linspace(0.0, np.pi / 2.0, NDF_SAMPLES)), 0.0, 1.0)
        den = (cos_t * a2 - cos_t) * cos_t + 1.0
        running = np.cumsum(a2 / (den * den * np.pi))
        return float(cos_t[int(np.argmax(running >= running[-1] * cutoff))])

    return _lru(_ndf_cutoff_cache, (float(roughness), float(cutoff)), make)


def specular_bounds(res, roughness, cutoff, device):
    """(cutoff cosine, bounds table of ops.specular_bounds) for a face size, cached per (N, roughness, cutoff, device); the cache keeps
    the NDF_CACHE_SIZE most recently used entries (clear_specular_cache() empties it)."""
    from .... import ops

    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    def make():
        c = ndf_cutoff_cosine(roughness, cutoff)
        return c, ops.specular_bounds(res, c, device)

    return _lru(_ndf_bounds_cache, (int(res), float(roughness), float(cutoff), str(device)), make)


def specular_cubemap(cubemap, roughness, cutoff=0.99, use_python=False):
    """GGX-prefiltered cube map (reference ops.py:446-458): colour sum / weight sum of ops.specular_cubemap_raw over the cone that
    keeps ``cutoff`` of the lobe's energy."""
    from .... import ops

    assert cubemap.shape[0] == 6 and cubemap.shape[1] == cubemap.shape[2], "Bad shape for cubemap tensor: %s" % str(cubemap.shape)
    ops.require_device(cubemap, what="specular_cubemap")
    c, bounds = specular_bounds(cubemap.shape[1], roughness, cutoff, cubemap.device)
    out = ops.specular_cubemap_raw(cubemap, roughness, c, bounds)
    if torch.is_anomaly_enabled():
        assert torch.all(torch.isfinite(out)), "Output of specular_cubemap contains inf or NaN"
    return out[..., 0:3] / out[..., 3:]
