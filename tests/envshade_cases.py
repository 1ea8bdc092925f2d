"""Named cases of the environment-shade tests (tests/test_envshade_cpu.py, tests/test_envshade_gpu.py), in one place: the lights, the
frames, the operand layouts, the kink measure and a float64 restatement of EnvironmentLight.shade whose backward can be broken one
piece at a time.  Every value is float32-representable, so the float64 reference, the float32 statements and the kernel start from the
same numbers.  The yardstick itself is tests/envlight_ref.shade with the lookups of tests/texture_ref.py."""
import math

import torch

import envlight_ref as R
import texture_ref as T

F64 = torch.float64
LO, HI = R.MIN_ROUGHNESS, R.MAX_ROUGHNESS
LO32, HI32 = float(torch.tensor(LO, dtype=torch.float32)), float(torch.tensor(HI, dtype=torch.float32))

# name -> (specular level sizes, diffuse size)
LIGHTS = {
    "a_8_4_2": ((8, 4, 2), 2),            # nearly every tap walks an edge or hits a corner; every gradient map is summed in LDS
    "b_64_32_16": ((64, 32, 16), 16),     # both scatter routes: 64 and 32 merge in the wave, 16 and the diffuse map live in LDS
    "c_64_to_4": ((64, 32, 16, 8, 4), 4),  # five levels: get_mip's upper branch reaches the top level
}
FRAMES = {"2x16x16": (2, 16, 16), "3x5x7": (3, 5, 7), "1x9x8": (1, 9, 8)}
FRAMES.update({f"list{p}": (1, 1, p) for p in (1, 63, 64, 65, 257, 1000)})
VIEWS = ("image", "full")  # [B,1,1,3] | [B,H,W,3] (on a point list: one row per point)
TRANSFORMS = ("none", "one", "per_image")  # None | [1,4,4] | [B,4,4]

SEED = 13  # of every random case below (the first from 11 on with which no frame under 100 pixels has a pixel near a kink: one of 72 is 1.4 %)


def random_cases():
    """(light, frame, view_pos form, transform, specular) of the random cases the kernel is held to float64 on: every frame under
    every light; the operand forms and both values of ``specular`` spread over them."""
    cases = []
    for i, frame_name in enumerate(FRAMES):
        for j, light_name in enumerate(LIGHTS):
            k = i * 3 + j
            xfm = TRANSFORMS[(k // 2) % 3]
            if xfm == "per_image" and FRAMES[frame_name][0] == 1:
                xfm = "one"
            cases.append((light_name, frame_name, VIEWS[k % 2], xfm, k % 5 != 3))
    return cases


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _r32(t):
    return t.float().double()


def light(name, seed=0):
    """-> (specular levels [6,S,S,3], diffuse [6,S,S,3]) in float64: independent random maps in [0, 4] (no prefilter: a lookup does not
    care where its texels came from)."""
    sizes, dsize = LIGHTS[name]
    g = _gen(1000 + seed)
    spec = [_r32(torch.rand(6, s, s, 3, generator=g, dtype=F64) * 4) for s in sizes]
    return spec, _r32(torch.rand(6, dsize, dsize, 3, generator=g, dtype=F64) * 4)


_fg = []


def fg_table():
    """the FG table as the light holds it: evaluated in float64, rounded to float32 once."""
    if not _fg:
        _fg.append(_r32(R.fg_table()))
    return _fg[0]


def frame(shape, seed, view="image"):
    """-> [gb_pos, gb_normal, kd, ks, view_pos]: positions around the origin, unit normals, albedo in [0, 1], ks = (occlusion in [0, 1],
    roughness in [0, 1.2]: below lo, both branches of get_mip, above 1; metalness in [0, 1]), the camera near (0.3, 0.2, 2.5)."""
    B, H, W = shape
    g = _gen(seed)
    pos = torch.randn(B, H, W, 3, generator=g, dtype=F64) * 0.3
    n = torch.randn(B, H, W, 3, generator=g, dtype=F64)
    n = n / n.norm(dim=-1, keepdim=True)
    kd = torch.rand(B, H, W, 3, generator=g, dtype=F64)
    ks = torch.rand(B, H, W, 3, generator=g, dtype=F64) * torch.tensor([1.0, 1.2, 1.0], dtype=F64)
    v = torch.tensor([0.3, 0.2, 2.5], dtype=F64) + 0.2 * torch.randn(B, 1, 1, 3, generator=g, dtype=F64)
    if view == "full":
        v = v + 0.05 * torch.randn(B, H, W, 3, generator=g, dtype=F64)
    else:
        assert view == "image"
    return [_r32(t) for t in (pos, n, kd, ks, v)]


def transform(kind, B, seed=0):
    """None | [1,4,4] | [B,4,4]: proper rotations (QR of a random matrix) with a translation column, which a direction must not see."""
    if kind == "none":
        return None
    n = 1 if kind == "one" else B
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=_gen(77 + seed), dtype=F64))
    q = q * torch.linalg.det(q).sign()[:, None, None]
    m = torch.eye(4, dtype=F64).repeat(n, 1, 1)
    m[:, :3, :3] = q
    m[:, :3, 3] = torch.tensor([5.0, -7.0, 11.0], dtype=F64)
    return _r32(m)


def reference(spec, diff, fg, leaves, specular=True, mtx=None):
    """tests/envlight_ref.shade, image by image where the transform is per image."""
    pos, n, kd, ks, view = leaves
    if mtx is None or mtx.shape[0] == 1:
        return R.shade(spec, diff, fg, pos, n, kd, ks, view, specular=specular, mtx=None if mtx is None else mtx[0])
    B = pos.shape[0]
    assert mtx.shape[0] == B
    rows = []
    for b in range(B):
        one = [t[b:b + 1] if t.shape[0] == B else t for t in leaves]
        rows.append(R.shade(spec, diff, fg, *one, specular=specular, mtx=mtx[b]))
    return torch.cat(rows)


# ---------------------------------------------------------------------------------------------- kinks
def _cube_coords(d, S):
    """-> (distance of the direction from a face boundary in face coordinates, distance of its texel coordinates from an integer)."""
    a = d.abs()
    major = a.amax(-1, keepdim=True).clamp(min=1e-300)
    st = a / major  # the major component is 1, the other two |s|, |t|
    second = st.sort(-1).values[..., 1]
    x = (d / major + 1) * 0.5 * S - 0.5  # (the sign conventions of a face mirror x into S - 1 - x: the same distance from an integer)
    frac = (x - x.round()).abs()
    frac = torch.where(st >= 1.0, torch.ones_like(frac), frac)  # (the major axis itself is no texel coordinate)
    return 1.0 - second, frac.amin(-1)


def directions(leaves, mtx=None):
    """-> (n . wo, lookup direction of the diffuse map, of the specular stack) in the dtype of the leaves."""
    pos, n, kd, ks, view = leaves
    wo = R.safe_normalize(view - pos)
    dn = (wo * n).sum(-1, keepdim=True)
    refl = R.safe_normalize(2 * dn * n - wo)
    nrm = n
    if mtx is not None:
        rot = mtx[:, :3, :3].to(pos.dtype).expand(pos.shape[0], 3, 3)
        refl, nrm = torch.einsum("bij,bhwj->bhwi", rot, refl), torch.einsum("bij,bhwj->bhwi", rot, nrm)
    return dn, nrm, refl


def near_kink(spec_sizes, diffuse_size, leaves, specular=True, mtx=None, fg_res=256, texel=1e-4, other=1e-5):
    """bool [B,H,W], on float64 inputs alone: the pixel lies within ``texel`` texel units of a texel boundary of a lookup it makes, or
    within ``other`` of a cube-face boundary, an integer level, roughness = lo / hi / 1 or n.v = 1e-4 -- where a gradient is
    discontinuous and float32 may legitimately stand on the other side."""
    pos, n, kd, ks, view = leaves
    dn, nd, rd = directions(leaves, mtx)
    face, tex = _cube_coords(nd, diffuse_size)
    near = (face < other) | (tex < texel)
    if specular:
        rough = ks[..., 1]
        L = len(spec_sizes)
        mip = R.get_mip(rough, L)
        level = mip.clamp(0, L - 1)
        l0 = level.floor().clamp(max=L - 1).long()
        sizes = torch.tensor(spec_sizes, dtype=F64)
        for l in (l0, (l0 + 1).clamp(max=L - 1)):
            face, tex = _cube_coords(rd, sizes[l][..., None])
            near |= (face < other) | (tex < texel)
        near |= ((mip - mip.round()).abs() < other) & (rough > LO) & (rough < 1.0)  # (below lo and above 1 the level is constant: no kink there)
        for r in (LO, HI, 1.0):
            near |= (rough - r).abs() < other
        near |= (dn[..., 0] - 1e-4).abs() < other
        for c in (dn[..., 0].clamp(min=1e-4), rough):
            x = c * fg_res - 0.5
            near |= (x - x.round()).abs() < texel
    return near


# ---------------------------------------------------------------------------------------------- a restatement whose backward can be broken
MUTATIONS = ("no_bias_grad", "no_fg_roughness_grad", "no_fg_ndv_grad", "no_visibility_factor", "rotation_not_transposed",
             "no_coarse_slot_scatter")


class _RotateWrongAdjoint(torch.autograd.Function):
    """v -> R v whose backward applies R again instead of its transpose."""

    @staticmethod
    def forward(ctx, v, rot):
        ctx.save_for_backward(rot)
        return torch.einsum("bij,bhwj->bhwi", rot, v)

    @staticmethod
    def backward(ctx, g):
        rot, = ctx.saved_tensors
        return torch.einsum("bij,bhwj->bhwi", rot, g), None


def shade_restated(spec, diff, fg, leaves, specular=True, mtx=None, mutate=None):
    """EnvironmentLight.shade again, statement by statement, with the specular lookup written as two linear lookups blended by the
    level's fraction, so that each piece of the backward can be named.  ``mutate`` breaks one piece of the BACKWARD (the values stay)."""
    assert mutate is None or mutate in MUTATIONS
    pos, n, kd, ks, view = leaves
    wo = R.safe_normalize(view - pos)
    dn = (wo * n).sum(-1, keepdim=True)
    refl = R.safe_normalize(2 * dn * n - wo)
    nrm = n
    if mtx is not None:
        rot = mtx[:, :3, :3].to(pos.dtype).expand(pos.shape[0], 3, 3)
        if mutate == "rotation_not_transposed":
            refl, nrm = _RotateWrongAdjoint.apply(refl, rot), _RotateWrongAdjoint.apply(nrm, rot)
        else:
            refl, nrm = torch.einsum("bij,bhwj->bhwi", rot, refl), torch.einsum("bij,bhwj->bhwi", rot, nrm)
    cube = dict(filter_mode="linear", boundary_mode="cube")
    col = T.texture(diff[None], nrm, **cube) * (kd * (1 - ks[..., 2:3]) if specular else kd)
    if specular:
        rough, metal = ks[..., 1:2], ks[..., 2:3]
        ndv = dn.clamp(min=1e-4)
        uv = torch.cat((ndv.detach() if mutate == "no_fg_ndv_grad" else ndv, rough.detach() if mutate == "no_fg_roughness_grad" else rough), -1)
        lut = T.texture(fg, uv, filter_mode="linear", boundary_mode="clamp")
        L = len(spec)
        level = R.get_mip(rough.detach() if mutate == "no_bias_grad" else rough, L)
        inside = (level >= 0) & (level <= L - 1)
        level = torch.where(inside, level, level.detach()).clamp(0, L - 1)  # (the clamped level has no gradient)
        l0 = level.detach().floor().clamp(max=L - 1)
        f = level - l0
        s = torch.zeros_like(col)
        for l in range(L):
            fine = T.texture(spec[l][None], refl, **cube)
            coarse = T.texture((spec[l].detach() if mutate == "no_coarse_slot_scatter" else spec[l])[None], refl, **cube)
            s = s + torch.where(l0 == l, (1 - f) * fine, torch.zeros_like(s)) + torch.where((l0 + 1).clamp(max=L - 1) == l, f * coarse, torch.zeros_like(s))
        col = col + s * (((1 - metal) * 0.04 + kd * metal) * lut[..., 0:1] + lut[..., 1:2])
    vis = 1 - ks[..., 0:1]
    if mutate == "no_visibility_factor":
        return col.detach() * vis + (col - col.detach())
    return col * vis


def tolerance(x32, x64):
    """the bound this chain is held to (tests/test_envlight_gpu.py): four times the float32 statements' own error, and never less than
    four float32 roundings of the tensor's largest magnitude."""
    return 4 * max(float((x32.double() - x64).abs().max()), 2.0 ** -22 * float(x64.abs().max()))
