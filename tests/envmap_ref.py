"""The two environment-probe resamplers restated from include/a3d.h ("Texture sampling", generated coordinates), with a dtype argument:
in float64 the truth the kernels are held to, in float32 on the CPU the yardstick e_ref (what one rounding per statement costs).  The
taps are the texture restatement's (tests/texture_ref.py: bilinear wrap, seamless cube)."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_ref as R  # noqa: E402


def lin(a, b, n, dtype):
    """torch.linspace's two-sided rule, statement by statement in ``dtype``; a, b: Python doubles, rounded to ``dtype`` once."""
    a, b = torch.tensor(a, dtype=dtype), torch.tensor(b, dtype=dtype)
    if n == 1:
        return a.reshape(1)
    step = (b - a) / torch.tensor(n - 1, dtype=dtype)
    i = torch.arange(n)
    return torch.where(i < n // 2, a + step * i.to(dtype), b - step * (n - 1 - i).to(dtype))


def latlong_coords(res, dtype):
    """-> uv [6,h,w,2] and the unit directions v [6,h,w,3] of latlong_to_cubemap's lookups."""
    h, w = res
    gy, gx = torch.meshgrid(lin(-1.0 + 1.0 / h, 1.0 - 1.0 / h, h, dtype), lin(-1.0 + 1.0 / w, 1.0 - 1.0 / w, w, dtype), indexing="ij")
    face = torch.arange(6)[:, None, None].expand(6, h, w)
    d = R.cube_to_dir(face, gx[None].expand(6, h, w), gy[None].expand(6, h, w))
    dd = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    v = d / torch.sqrt(torch.clamp(dd, min=1e-20))[..., None]
    two_pi, pi = torch.tensor(2 * math.pi, dtype=dtype), torch.tensor(math.pi, dtype=dtype)
    tu = torch.atan2(v[..., 0], -v[..., 2]) / two_pi + 0.5
    tv = torch.acos(torch.clamp(v[..., 1], min=-1, max=1)) / pi
    return torch.stack((tu, tv), -1), v


def latlong_to_cubemap(latlong, res, dtype=torch.float64):
    """[H,W,C] -> [6,h,w,C]; differentiable in the map."""
    uv, _ = latlong_coords(res, dtype)
    return R.texture(latlong.to(dtype)[None], uv, filter_mode="linear", boundary_mode="wrap")


def cube_dirs(res, dtype):
    """The directions [1,h,w,3] of cubemap_to_latlong's lookups."""
    h, w = res
    gy, gx = torch.meshgrid(lin(0.0 + 1.0 / h, 1.0 - 1.0 / h, h, dtype), lin(-1.0 + 1.0 / w, 1.0 - 1.0 / w, w, dtype), indexing="ij")
    pi = torch.tensor(math.pi, dtype=dtype)
    theta, phi = gy * pi, gx * pi
    st, ct, sp, cp = torch.sin(theta), torch.cos(theta), torch.sin(phi), torch.cos(phi)
    return torch.stack((st * sp, ct, -(st * cp)), -1)[None]


def cubemap_to_latlong(cubemap, res, dtype=torch.float64):
    """[6,S,S,C] -> [h,w,C]; differentiable in the cube."""
    return R.texture(cubemap.to(dtype)[None], cube_dirs(res, dtype), filter_mode="linear", boundary_mode="cube")[0]


def pole_mask(res):
    """[6,h,w] bool: the lookups of latlong_to_cubemap whose direction has x^2 + z^2 < 1e-12 (tu is undefined there)."""
    _, v = latlong_coords(res, torch.float64)
    return v[..., 0] ** 2 + v[..., 2] ** 2 < 1e-12
