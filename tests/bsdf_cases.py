"""Input builders and the parity rule shared by tests/golden/make_golden_bsdf.py, tests/test_bsdf_cpu.py and tests/test_bsdf_gpu.py.

Two kinds of inputs.  'cond': conditioned BY CONSTRUCTION so that nothing sits on a kink -- unit normals, view and light directions placed
in the normal's hemisphere with cosines in [0.05, 0.95] and azimuths 0.2 .. pi/2 apart (so woDotN, wiDotN >= 0.05, nDotH <= 0.975, woDotH
<= 0.9996), roughness in [0.1, 0.99] (alpha inside its clamp).  'wild': the reference's own test pattern, torch.rand everything
(renderutils/tests/test_bsdf.py).  'bcast': a conditioned planar patch [2,16,16] lit and seen from fixed points, view_pos / light_pos
[B,1,1,3] resp. [1,1,1,3].
"""
import math

import torch

GOLDEN_PIXELS = 512
LOSSES = ("l1", "mse", "smape", "relmse")
TONEMAPS = ("none", "log_srgb")
GOLDEN_CASES = [(n, k, s) for s, (n, k) in enumerate(
    [("lambert", "cond"), ("lambert", "wild"), ("frostbite_diffuse", "cond"), ("frostbite_diffuse", "wild"), ("pbr_specular", "cond"),
     ("pbr_specular", "wild"), ("pbr_bsdf_lambert", "cond"), ("pbr_bsdf_lambert", "wild"), ("pbr_bsdf_lambert", "bcast"),
     ("pbr_bsdf_frostbite", "cond"), ("pbr_bsdf_frostbite", "wild"), ("pbr_bsdf_frostbite", "bcast"), ("_fresnel_shlick", "wild"),
     ("_ndf_ggx", "wild"), ("_lambda_ggx", "wild"), ("_masking_smith", "wild")])]
KINK_EPS = 1e-5
SPEC_EPS = 1e-4


def _unit(g, n):
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)


def _frame(nrm, g):
    """nrm plus two directions in its hemisphere: cosines in [0.05, 0.95], azimuths 0.2 .. pi/2 apart."""
    n = nrm.shape[0]
    helper = torch.where(nrm[:, 0:1].abs() < 0.9, torch.tensor([1.0, 0.0, 0.0]), torch.tensor([0.0, 1.0, 0.0])).expand(n, 3)
    t = torch.nn.functional.normalize(torch.cross(nrm, helper, dim=-1), dim=-1)
    b = torch.cross(nrm, t, dim=-1)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, 1, generator=g)
    phi_o = u(0.0, 2 * math.pi)
    phi_i = phi_o + u(0.2, math.pi / 2) * torch.where(torch.rand(n, 1, generator=g) < 0.5, -1.0, 1.0)
    out = []
    for phi in (phi_o, phi_i):
        c = u(0.05, 0.95)
        s = torch.sqrt(1 - c * c)
        out.append(nrm * c + (t * torch.cos(phi) + b * torch.sin(phi)) * s)
    return out


def make_inputs(name, kind, n, seed):
    """float32 CPU inputs of one case, in the public function's argument order."""
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)
    if name.startswith("_"):
        k = {"_fresnel_shlick": 3, "_ndf_ggx": 2, "_lambda_ggx": 2, "_masking_smith": 3}[name]
        return [rand(n, 1) for _ in range(k)]
    if kind == "wild":
        k = {"lambert": (3, 3), "frostbite_diffuse": (3, 3, 3, 1), "pbr_specular": (3, 3, 3, 3, 1)}.get(name, (3,) * 6)
        return [rand(n, c) for c in k]
    if kind == "bcast":
        B, H, W = 2, 16, 16
        assert n == B * H * W
        ys, xs = torch.meshgrid(torch.linspace(-0.5, 0.5, H), torch.linspace(-0.5, 0.5, W), indexing="ij")
        pos = torch.stack([xs, ys, torch.zeros_like(xs)], -1)[None].repeat(B, 1, 1, 1) + 0.02 * (rand(B, H, W, 3) - 0.5)
        nrm = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.1 * (rand(B, H, W, 3) - 0.5), dim=-1)
        view = torch.tensor([[2.0, 0.5, 2.0], [1.8, -0.4, 2.2]]).view(B, 1, 1, 3)
        light = torch.tensor([2.5, -0.5, 1.5]).view(1, 1, 1, 3)
        arm = torch.stack([rand(B, H, W), 0.1 + 0.89 * rand(B, H, W), rand(B, H, W)], -1)
        return [rand(1, 1, 1, 3) * 0.8 + 0.1, arm, pos, nrm, view, light]
    nrm = _unit(g, n)
    wo, wi = _frame(nrm, g)
    rough = 0.1 + 0.89 * rand(n, 1)
    if name == "lambert":
        return [nrm, wi]
    if name == "frostbite_diffuse":
        return [nrm, wi, wo, rough]
    if name == "pbr_specular":
        return [rand(n, 3), nrm, wo, wi, rough * rough]
    pos = torch.randn(n, 3, generator=g)
    view = pos + wo * (1 + 3 * rand(n, 1))
    light = pos + wi * (1 + 3 * rand(n, 1))
    return [rand(n, 3), torch.cat([rand(n, 1), rough, rand(n, 1)], -1), pos, nrm, view, light]


def out_shape(name, inputs):
    lead = torch.broadcast_shapes(*[t.shape[:-1] for t in inputs])
    return (*lead, 3 if name.startswith("pbr") else 1)


def make_images(n, seed):
    """HDR image pairs for image_loss, conditioned: values in [0.05, 8], |img - target| >= 1e-3 per element, tone-mapped values away
    from the sRGB knee (log(x + 1) >= log(1.05) = 0.049 >> 0.0031308)."""
    g = torch.Generator().manual_seed(seed)
    img = 0.05 + 7.95 * torch.rand(n // 4, 4, generator=g) ** 2
    delta = (1e-3 + torch.rand(n // 4, 4, generator=g)) * torch.where(torch.rand(n // 4, 4, generator=g) < 0.5, -1.0, 1.0)
    target = torch.where(img + delta < 0.05, img - delta, img + delta)
    return img, target


def call_public(ru, name, inputs, **kw):
    if name.startswith("pbr_bsdf"):
        return ru.pbr_bsdf(*inputs, min_roughness=0.08, bsdf=name.split("_")[-1], **kw)
    return getattr(ru, name)(*inputs, **kw)


def near_kink(name, inputs):
    """[pixels] bool: elements within KINK_EPS of a kink of the BSDF (cosTheta at either clamp, woDotN / wiDotN at specular_epsilon or
    0, alpha at a clamp), evaluated in float64 from the inputs."""
    x = [t.double() for t in inputs]
    dot = lambda a, b: (a * b).sum(-1)
    nz = torch.nn.functional.normalize
    near = lambda v, *ks: torch.stack([(v - k).abs() <= KINK_EPS for k in ks]).any(0)
    cos_k = (SPEC_EPS, 1 - SPEC_EPS)
    if name == "lambert":
        return near(dot(x[0], x[1]), 0.0)
    if name == "frostbite_diffuse":
        return near(dot(x[1], x[0]), 0.0, *cos_k) | near(dot(x[2], x[0]), 0.0, *cos_k)
    if name == "pbr_specular":
        col, nrm, wo, wi, alpha = x
        rough = None
    else:
        kd, arm, pos, nrm, view, light = x
        wo, wi = nz(view - pos, dim=-1), nz(light - pos, dim=-1)
        rough, alpha = arm[..., 1], (arm[..., 1:2] ** 2)
    h = nz(wo + wi, dim=-1)
    bad = near(dot(wo, nrm), 0.0, *cos_k) | near(dot(wi, nrm), 0.0, *cos_k) | near(dot(wo, h), *cos_k) | near(dot(nrm, h), *cos_k)
    bad = bad | near(alpha[..., 0], 0.08 * 0.08, 1.0)
    return bad


def rel_err(x, x64):
    """e(x) = |x - x64| / (|x64| + s), s the median of |x64| over the tensor.  Where more than half of a tensor is exactly 0 (unlit
    pixels of the wild sets) s is 0: an element that is exactly right has e = 0 there (not 0 / 0), one that is not has e = inf."""
    x64 = x64.double()
    s = x64.abs().median()
    err = (x.double().cpu() - x64).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / (x64.abs() + s))


def parity(what, hip, twin32, x64, keep=None):
    """The parity rule: max e(hip) <= 4 max e(twin32) and mean e(hip) <= 2 mean e(twin32), per tensor; prints both sides.  ``keep``:
    bool mask over the leading shape of elements that take part (None: all)."""
    eh, et = rel_err(hip, x64), rel_err(twin32, x64)
    if keep is not None:
        keep = keep.reshape(*keep.shape, *([1] * (eh.dim() - keep.dim()))).expand_as(eh)
        eh, et = eh[keep], et[keep]
    mh, mt, ah, at = float(eh.max()), float(et.max()), float(eh.mean()), float(et.mean())
    print(f"{what}: max e(hip) {mh:.3e} / max e(twin32) {mt:.3e} = {mh / max(mt, 1e-300):.3f}; "
          f"mean e(hip) {ah:.3e} / mean e(twin32) {at:.3e} = {ah / max(at, 1e-300):.3f}")
    assert mh <= 4 * mt and ah <= 2 * at, (what, mh, mt, ah, at)
