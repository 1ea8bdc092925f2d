"""``use_python`` is accepted for signature parity (reference default False = its JIT CUDA plugin, which does not exist on this
platform); both values take the torch path below -- the one every config of the reference selects (render.py:72,278).
The two cube-map prefilters (diffuse_cubemap, specular_cubemap) exist in the reference ONLY inside that plugin (its use_python
branch is ``assert False``): here both values of ``use_python`` run the HIP kernels of csrc/envlight.hip.
The shading BSDFs (lambert, frostbite_diffuse, pbr_specular, pbr_bsdf) and image_loss: ``use_python=True`` is the torch twin below (any
device, any dtype), ``use_python=False`` runs CUDA float32 inputs through the fused kernels of csrc/bsdf.hip (ops.bsdf / ops.image_loss) and
takes the twin for anything else.  The four terms _fresnel_shlick, _ndf_ggx, _lambda_ggx, _masking_smith are the twin for both values."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from ...._lib import fp32_region

NORMAL_THRESHOLD = 0.1  # reference renderutils/bsdf.py:13
HIP_XFM_POINTS = True  # xfm_points on the GPU as a3d_xfm_points_fwd / _bwd (False: the padded torch matmul, e.g. for double precision)
HIP_SHADING_NORMAL = True  # prepare_shading_normal WITH a perturbed normal as a3d_shading_normal_fwd / _bwd (False: always the torch statements)


def _dot(x, y):
    return torch.sum(x * y, -1, keepdim=True)


def _on_gpu_f32(t):
    return t.is_cuda and t.dtype == torch.float32


def _hip_xfm_ok(points, matrix, on_gpu_f32=_on_gpu_f32):
    """The clip transform's kernel takes these operands.  ``on_gpu_f32``: the caller's form of the device question (render._plan_route's)."""
    if not (HIP_XFM_POINTS and on_gpu_f32(points) and on_gpu_f32(matrix)):
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
    ``smooth_tng`` is not touched (so it may be None).  With a perturbed normal, ``use_python=False`` and CUDA float32 tensors the
    statements below run as one launch each way (ops.shading_normal, csrc/tangent.hip); they are its specification.
    """
    if (not use_python and perturbed_nrm is not None and HIP_SHADING_NORMAL
            and all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() >= 1 and t.shape[-1] == 3
                    for t in (pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm))):
        from .... import ops

        out = ops.shading_normal(pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm, two_sided_shading, opengl)
        if torch.is_anomaly_enabled():
            assert torch.all(torch.isfinite(out)), "Output of prepare_shading_normal contains inf or NaN"
        return out
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


# ---------------------------------------------------------------------------------------------- shading BSDFs and the HDR image loss
# The torch twins restate reference renderutils/bsdf.py:57-151 and loss.py:16-41 operation by operation; they are the specification of
# the kernels in csrc/bsdf.hip (values, and through autograd the subgradients at every clamp / where / abs).
SPECULAR_EPSILON = 1e-4
HIP_BSDF = True  # the BSDFs and image_loss as a3d_bsdf_* / a3d_image_loss_* (False: always the torch twin)


def _clamp_cos(cos_theta):
    return torch.clamp(cos_theta, min=SPECULAR_EPSILON, max=1.0 - SPECULAR_EPSILON)


def _twin_fresnel_shlick(f0, f90, cos_theta):
    return f0 + (f90 - f0) * (1.0 - _clamp_cos(cos_theta)) ** 5.0


def _twin_ndf_ggx(alpha_sqr, cos_theta):
    c = _clamp_cos(cos_theta)
    d = (c * alpha_sqr - c) * c + 1
    return alpha_sqr / (d * d * np.pi)


def _twin_lambda_ggx(alpha_sqr, cos_theta):
    c = _clamp_cos(cos_theta)
    c2 = c * c
    tan2 = (1.0 - c2) / c2
    return 0.5 * (torch.sqrt(1 + alpha_sqr * tan2) - 1.0)


def _twin_masking_smith(alpha_sqr, cos_i, cos_o):
    return 1 / (1 + _twin_lambda_ggx(alpha_sqr, cos_i) + _twin_lambda_ggx(alpha_sqr, cos_o))


def _twin_lambert(nrm, wi):
    return torch.clamp(_dot(nrm, wi), min=0.0) / np.pi


def _twin_frostbite(nrm, wi, wo, linear_roughness):
    wi_n, wo_n = _dot(wi, nrm), _dot(wo, nrm)
    wi_h = _dot(wi, F.normalize(wo + wi, dim=-1))
    bias = 0.5 * linear_roughness
    factor = 1.0 - (0.51 / 1.51) * linear_roughness
    f90 = bias + 2.0 * wi_h * wi_h * linear_roughness
    res = _twin_fresnel_shlick(1.0, f90, wi_n) * _twin_fresnel_shlick(1.0, f90, wo_n) * factor
    return torch.where((wi_n > 0.0) & (wo_n > 0.0), res, torch.zeros_like(res))


def _twin_pbr_specular(col, nrm, wo, wi, alpha, min_roughness=0.08):
    a = torch.clamp(alpha, min=min_roughness * min_roughness, max=1.0)
    a2 = a * a
    h = F.normalize(wo + wi, dim=-1)
    wo_n, wi_n, wo_h, n_h = _dot(wo, nrm), _dot(wi, nrm), _dot(wo, h), _dot(nrm, h)
    w = _twin_fresnel_shlick(col, 1, wo_h) * _twin_ndf_ggx(a2, n_h) * _twin_masking_smith(a2, wo_n, wi_n) * 0.25 \
        / torch.clamp(wo_n, min=SPECULAR_EPSILON)
    return torch.where((wo_n > SPECULAR_EPSILON) & (wi_n > SPECULAR_EPSILON), w, torch.zeros_like(w))


def _twin_pbr_bsdf(kd, arm, pos, nrm, view_pos, light_pos, min_roughness, lobe):
    wo = F.normalize(view_pos - pos, dim=-1)
    wi = F.normalize(light_pos - pos, dim=-1)
    spec_str, roughness, metallic = arm[..., 0:1], arm[..., 1:2], arm[..., 2:3]
    ks = (0.04 * (1.0 - metallic) + kd * metallic) * (1 - spec_str)
    kd = kd * (1.0 - metallic)
    diffuse = kd * (_twin_lambert(nrm, wi) if lobe == 0 else _twin_frostbite(nrm, wi, wo, roughness))
    return diffuse + _twin_pbr_specular(ks, nrm, wo, wi, roughness * roughness, min_roughness=min_roughness)


def _twin_tonemap(x):
    f = torch.log(torch.clamp(x, min=0, max=65535) + 1)
    return torch.where(f > 0.0031308, torch.pow(torch.clamp(f, min=0.0031308), 1.0 / 2.4) * 1.055 - 0.055, 12.92 * f)


def _twin_image_loss(img, target, loss, tonemapper):
    if tonemapper == "log_srgb":
        img, target = _twin_tonemap(img), _twin_tonemap(target)
    if loss == "mse":
        return F.mse_loss(img, target)
    if loss == "smape":
        return torch.mean(torch.abs(img - target) / (torch.abs(img) + torch.abs(target) + 0.01))
    if loss == "relmse":
        return torch.mean((img - target) * (img - target) / (img * img + target * target + 0.1))
    return F.l1_loss(img, target)


def _hip_bsdf_ok(*tensors):
    return HIP_BSDF and all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() >= 1 for t in tensors)


def _finite(out, name):
    if torch.is_anomaly_enabled():
        assert torch.all(torch.isfinite(out)), "Output of %s contains inf or NaN" % name
    return out


def _fresnel_shlick(f0, f90, cosTheta, use_python=False):
    """f0 + (f90 - f0) (1 - clamp(cosTheta, 1e-4, 1 - 1e-4))^5 (reference ops.py:101-109).  The torch twin for both values of
    ``use_python``: the term exists in the reference's plugin only to test it; inside pbr_specular / frostbite_diffuse it is fused."""
    return _finite(_twin_fresnel_shlick(f0, f90, cosTheta), "_fresnel_shlick")


def _ndf_ggx(alphaSqr, cosTheta, use_python=False):
    """GGX normal distribution (reference ops.py:124-132); the torch twin for both values of ``use_python`` (see _fresnel_shlick)."""
    return _finite(_twin_ndf_ggx(alphaSqr, cosTheta), "_ndf_ggx")


def _lambda_ggx(alphaSqr, cosTheta, use_python=False):
    """GGX Lambda (reference ops.py:146-154); the torch twin for both values of ``use_python`` (see _fresnel_shlick)."""
    return _finite(_twin_lambda_ggx(alphaSqr, cosTheta), "_lambda_ggx")


def _masking_smith(alphaSqr, cosThetaI, cosThetaO, use_python=False):
    """Height-correlated Smith masking (reference ops.py:168-176); the torch twin for both values of ``use_python``."""
    return _finite(_twin_masking_smith(alphaSqr, cosThetaI, cosThetaO), "_masking_smith")


def lambert(nrm, wi, use_python=False):
    """max(nrm . wi, 0) / pi -> [..., 1] (reference ops.py:244-264).  Inputs [minibatch, height, width, 3] or broadcastable."""
    if not use_python and _hip_bsdf_ok(nrm, wi):
        from .... import ops

        out = ops.bsdf("lambert", (nrm, wi))
    else:
        out = _twin_lambert(nrm, wi)
    return _finite(out, "lambert")


def frostbite_diffuse(nrm, wi, wo, linearRoughness, use_python=False):
    """Frostbite's normalised Disney diffuse lobe -> [..., 1] (reference ops.py:278-300); linearRoughness is [..., 1]."""
    if not use_python and _hip_bsdf_ok(nrm, wi, wo, linearRoughness):
        from .... import ops

        out = ops.bsdf("frostbite_diffuse", (nrm, wi, wo, linearRoughness))
    else:
        out = _twin_frostbite(nrm, wi, wo, linearRoughness)
    return _finite(out, "frostbite_diffuse")


def pbr_specular(col, nrm, wo, wi, alpha, min_roughness=0.08, use_python=False):
    """GGX specular lobe -> [..., 3] (reference ops.py:315-339); alpha is [..., 1], clamped to [min_roughness^2, 1]."""
    if not use_python and _hip_bsdf_ok(col, nrm, wo, wi, alpha):
        from .... import ops

        out = ops.bsdf("pbr_specular", (col, nrm, wo, wi, alpha), min_roughness=min_roughness)
    else:
        out = _twin_pbr_specular(col, nrm, wo, wi, alpha, min_roughness=min_roughness)
    return _finite(out, "pbr_specular")


def pbr_bsdf(kd, arm, pos, nrm, view_pos, light_pos, min_roughness=0.08, bsdf="lambert", use_python=False):
    """Diffuse + GGX specular response to a point light -> [..., 3] (reference ops.py:355-386): arm = (specular strength, linear
    roughness, metalness); bsdf 'lambert' or 'frostbite' picks the diffuse lobe; view_pos / light_pos typically broadcast."""
    lobe = 1 if bsdf == "frostbite" else 0
    if not use_python and _hip_bsdf_ok(kd, arm, pos, nrm, view_pos, light_pos):
        from .... import ops

        out = ops.bsdf("pbr_bsdf", (kd, arm, pos, nrm, view_pos, light_pos), min_roughness=min_roughness, lobe=lobe)
    else:
        out = _twin_pbr_bsdf(kd, arm, pos, nrm, view_pos, light_pos, min_roughness, lobe)
    return _finite(out, "pbr_bsdf")


def image_loss(img, target, loss="l1", tonemapper="none", use_python=False):
    """HDR image loss, a scalar: the mean over all elements of 'l1' | 'mse' | 'smape' | 'relmse' (anything else is l1, as in the
    reference), after the optional 'log_srgb' tone map srgb(log(clamp(x, 0, 65535) + 1)) (reference ops.py:476-498)."""
    if not use_python and _hip_bsdf_ok(img, target):
        from .... import ops

        out = ops.image_loss(img, target, loss, tonemapper)
    else:
        out = _twin_image_loss(img, target, loss, tonemapper)
    return _finite(out, "image_loss")
