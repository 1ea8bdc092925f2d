"""Float64 torch restatement of the texture specification (ops.texture's docstring; csrc/texture.hip), differentiable by autograd.

Written for this project from the specification, lookup-parallel and unoptimised: every level is sampled at every lookup and the
lookup's one or two levels are selected afterwards.  The level of detail reads ``uv`` detached (the specification treats the level as a
constant for uv's gradient).  Lives in tests/ because oracle/ is frozen.
"""
import torch

FACES = 6


def mip_sizes(h, w, max_mip_level=None, max_levels=16):
    sizes = [(h, w)]
    top = max_levels - 1 if max_mip_level is None else min(max_mip_level, max_levels - 1)
    while len(sizes) - 1 < top:
        h, w = sizes[-1]
        if (h == 1 and w == 1) or (h > 1 and h % 2) or (w > 1 and w % 2):
            break
        sizes.append((max(h // 2, 1), max(w // 2, 1)))
    return sizes


def box_down(t):
    """One level of the box-filter chain: [..., H, W, C] -> [..., H/2 | 1, W/2 | 1, C]."""
    H, W, C = t.shape[-3:]
    sh, sw = (2 if H > 1 else 1), (2 if W > 1 else 1)
    return t.reshape(*t.shape[:-3], H // sh, sh, W // sw, sw, C).mean(dim=(-4, -2))


def mip_chain(tex, max_mip_level=None):
    H, W = tex.shape[-3], tex.shape[-2]
    levels = [tex]
    for _ in mip_sizes(H, W, max_mip_level)[1:]:
        levels.append(box_down(levels[-1]))
    return levels


def cube_to_dir(face, s, t):
    """The reference's cube_to_dir (model/render/util.py:96-103), face a tensor."""
    one = torch.ones_like(s)
    table = torch.stack([torch.stack(v, -1) for v in (
        (one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one))], 0)  # [6, ..., 3]
    return table.gather(0, face[None, ..., None].expand(1, *face.shape, 3))[0]


def cube_face(d):
    """-> face, s, t, |major| of directions d [..., 3] (ties x before y before z)."""
    x, y, z = d.unbind(-1)
    ax, ay, az = x.abs(), y.abs(), z.abs()
    isx = (ax >= ay) & (ax >= az)
    isy = ~isx & (ay >= az)
    face = torch.where(isx, torch.where(x >= 0, 0, 1), torch.where(isy, torch.where(y >= 0, 2, 3), torch.where(z >= 0, 4, 5)))
    m = torch.where(isx, ax, torch.where(isy, ay, az))
    num_s = torch.stack([-z, z, x, x, x, -x], -1).gather(-1, face[..., None])[..., 0]
    num_t = torch.stack([-y, -y, z, -z, -y, -y], -1).gather(-1, face[..., None])[..., 0]
    return face, num_s / m, num_t / m, m


def _cube_rows(b, face, ix, iy, S):
    """Flat texel row of cube taps (after the edge walk) and the corner mask."""
    inx, iny = (ix >= 0) & (ix < S), (iy >= 0) & (iy < S)
    sv = -1.0 + (2 * ix + 1).double() / S
    tv = -1.0 + (2 * iy + 1).double() / S
    f2, s2, t2, _ = cube_face(cube_to_dir(face, sv, tv))
    jx = torch.floor((s2 + 1) * 0.5 * S).long().clamp(0, S - 1)
    jy = torch.floor((t2 + 1) * 0.5 * S).long().clamp(0, S - 1)
    inside = inx & iny
    f = torch.where(inside, face, f2)
    jx, jy = torch.where(inside, ix, jx), torch.where(inside, iy, jy)
    return ((b * FACES + f) * S + jy) * S + jx, ~inx & ~iny


def sample_level(level, b, x, y, nearest, boundary, face=None, unit=False):
    """[N, C] samples of one level at texel coordinates x, y [N] (texel i centred at i); b = texture image per lookup.  unit: every tap
    weighs 1 (a cube corner, the mean of the other three, 1/3 each) -- see ``terms``."""
    C = level.shape[-1]
    flat = level.reshape(-1, C)
    if face is not None:  # cube
        S = level.shape[-2]
        if nearest:
            ix = torch.floor(x + 0.5).long().clamp(0, S - 1)
            iy = torch.floor(y + 0.5).long().clamp(0, S - 1)
            return flat[((b * FACES + face) * S + iy) * S + ix]
        x0, y0 = torch.floor(x), torch.floor(y)
        fx, fy = (x - x0)[:, None], (y - y0)[:, None]
        x0, y0 = x0.long(), y0.long()
        rows, corner = zip(*[_cube_rows(b, face, x0 + dx, y0 + dy, S) for dy in (0, 1) for dx in (0, 1)])
        T = torch.stack([flat[r.clamp(min=0)] for r in rows], 1)  # [N, 4, C]
        corner = torch.stack(corner, 1)[..., None]
        mean3 = (T * (~corner)).sum(1, keepdim=True) / 3.0
        T = torch.where(corner, mean3, T)
        if unit:
            return T.sum(1)
        top = T[:, 0] * (1 - fx) + T[:, 1] * fx
        bot = T[:, 2] * (1 - fx) + T[:, 3] * fx
        return top * (1 - fy) + bot * fy
    H, W = level.shape[-3], level.shape[-2]

    def tap(ix, iy):
        if boundary == "wrap":
            ok, ix, iy = None, ix % W, iy % H
        else:
            ok = ((ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)) if boundary == "zero" else None
            ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
        v = flat[(b * H + iy) * W + ix]
        return v if ok is None else v * ok[:, None].to(v.dtype)

    if nearest:
        return tap(torch.floor(x + 0.5).long(), torch.floor(y + 0.5).long())
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    x0, y0 = x0.long(), y0.long()
    if unit:
        return tap(x0, y0) + tap(x0 + 1, y0) + tap(x0, y0 + 1) + tap(x0 + 1, y0 + 1)
    top = tap(x0, y0) * (1 - fx) + tap(x0 + 1, y0) * fx
    bot = tap(x0, y0 + 1) * (1 - fx) + tap(x0 + 1, y0 + 1) * fx
    return top * (1 - fy) + bot * fy


def lod_from_jacobian(J00, J01, J10, J11):
    """0.5 log2(lambda_max(J J^T)); -inf for a zero J (no NaN, no gradient)."""
    a, c, b = J00 * J00 + J01 * J01, J10 * J10 + J11 * J11, J00 * J10 + J01 * J11
    lam = 0.5 * (a + c) + torch.sqrt((0.5 * (a - c)) ** 2 + b * b)
    ok = lam > 0
    return torch.where(ok, 0.5 * torch.log2(torch.where(ok, lam, torch.ones_like(lam))), torch.full_like(lam, -float("inf")))


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode="auto", boundary_mode="wrap", max_mip_level=None, unit=False):
    """The specification, float64.  ``mip``: None (the box chain of ``tex``, differentiable) or a list of levels 1..  ``unit``: every
    tap and level slot weighs 1 (for ``terms``; not a sampling mode)."""
    if filter_mode == "auto":
        filter_mode = "linear-mipmap-linear" if (uv_da is not None or mip_level_bias is not None) else "linear"
    cube = boundary_mode == "cube"
    lead = uv.shape[:-1]
    N = uv[..., 0].numel()
    B, Bt = uv.shape[0], tex.shape[0]
    b = (torch.arange(N, device=uv.device) // (N // B)) if Bt > 1 else torch.zeros(N, dtype=torch.long, device=uv.device)
    u = uv.reshape(N, uv.shape[-1])
    mipmap = filter_mode in ("linear-mipmap-nearest", "linear-mipmap-linear")
    if mipmap:
        levels = mip_chain(tex, max_mip_level) if mip is None else [tex] + list(mip)[: (None if max_mip_level is None else max_mip_level)]
    else:
        levels = [tex]
    L = len(levels)
    face = s = t = None
    if cube:  # (a zero direction samples 0 with no gradient: it is swapped for a finite one so that no NaN enters autograd)
        live = u.detach().abs().amax(-1) > 0
        u = torch.where(live[:, None], u, torch.ones_like(u))
        face, s, t, m = cube_face(u)
    # level of detail
    level = torch.zeros(N, dtype=uv.dtype, device=uv.device)
    if mipmap:
        if uv_da is not None:
            da = uv_da.reshape(N, -1)
            if cube:
                ud = u.detach()
                fd, sd, td, md = cube_face(ud)
                half = 0.5 * tex.shape[-2]
                idx = lambda tbl: torch.tensor(tbl, device=uv.device)[fd]
                ia, ib, im = idx([2, 2, 0, 0, 0, 0]), idx([1, 1, 2, 2, 1, 1]), idx([0, 0, 1, 1, 2, 2])
                sa, sb = idx([-1.0, 1, 1, 1, 1, -1]).double(), idx([-1.0, -1, 1, -1, -1, -1]).double()
                sm = torch.where(ud.gather(1, im[:, None])[:, 0] >= 0, 1.0, -1.0).double()
                g = lambda comp, k: da.gather(1, (2 * comp + k)[:, None])[:, 0]
                J00 = half * (sa * g(ia, 0) - sd * sm * g(im, 0)) / md
                J01 = half * (sa * g(ia, 1) - sd * sm * g(im, 1)) / md
                J10 = half * (sb * g(ib, 0) - td * sm * g(im, 0)) / md
                J11 = half * (sb * g(ib, 1) - td * sm * g(im, 1)) / md
            else:
                Th, Tw = tex.shape[1], tex.shape[2]
                J00, J01, J10, J11 = da[:, 0] * Tw, da[:, 1] * Tw, da[:, 2] * Th, da[:, 3] * Th
            level = lod_from_jacobian(J00, J01, J10, J11)
        if mip_level_bias is not None:
            level = level + mip_level_bias.reshape(N)
        level = torch.where(torch.isinf(level) & (level < 0), torch.zeros_like(level), level)
        level = torch.clamp(level, 0.0, float(L - 1))
    if filter_mode == "linear-mipmap-nearest":
        l0 = torch.floor(level.detach() + 0.5).long().clamp(max=L - 1)
        slots = [(l0, torch.ones_like(level))]
    elif filter_mode == "linear-mipmap-linear":
        l0 = torch.floor(level.detach()).long().clamp(max=L - 1)
        f = level - l0.to(level.dtype)
        slots = [(l0, 1 - f), ((l0 + 1).clamp(max=L - 1), f)]
    else:
        slots = [(torch.zeros(N, dtype=torch.long, device=uv.device), torch.ones_like(level))]
    nearest = filter_mode == "nearest"
    out = 0
    for li, lev in enumerate(levels):
        if cube:
            S = lev.shape[-2]
            x, y = (s + 1) * 0.5 * S - 0.5, (t + 1) * 0.5 * S - 0.5
        else:
            x, y = u[:, 0] * lev.shape[2] - 0.5, u[:, 1] * lev.shape[1] - 0.5
        val = sample_level(lev, b, x, y, nearest, boundary_mode, face, unit)
        wsum = sum(torch.where(lv == li, torch.ones_like(w) if unit else w, torch.zeros_like(w)) for lv, w in slots)
        out = out + wsum[:, None] * val
    if cube:
        out = torch.where(live[:, None], out, torch.zeros_like(out))
    return out.reshape(*lead, tex.shape[-1])


def terms(tex, uv, g_out, uv_da=None, mip_level_bias=None, mip=None, unit=False, **kw):
    """The texel scatter of the backward, per level and before any box-filter adjoint: [g of level 0, level 1, ..] (float64) for the
    per-lookup weights ``g_out`` [..., C] >= 0.  unit=False: sum over lookups and taps of w * g_out, with the specification's tap and
    level weights -- all non-negative, so g_out = |g| gives the magnitude sum |w g| a float sum of those terms rounds against.
    unit=True: every tap weighs 1, so g_out = 1 counts the terms (an upper bound: taps of weight 0 count too)."""
    mipmap = kw.get("filter_mode", "auto") in ("linear-mipmap-nearest", "linear-mipmap-linear") or (
        kw.get("filter_mode", "auto") == "auto" and (uv_da is not None or mip_level_bias is not None))
    stack = [tex] + (list(mip) if mip is not None else (mip_chain(tex, kw.get("max_mip_level"))[1:] if mipmap else []))
    leaves = [t.detach().double().clone().requires_grad_(True) for t in stack]
    dbl = lambda t: None if t is None else t.detach().double()
    out = texture(leaves[0], dbl(uv), dbl(uv_da), dbl(mip_level_bias), mip=leaves[1:] if mipmap else None, unit=unit, **kw)
    grads = torch.autograd.grad(out, leaves, g_out.double().expand(out.shape), allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for t, g in zip(leaves, grads)]


# ------------------------------------------------------------------------------------------------ test fields and error bounds
# (tests/test_texture_backward_gpu.py and its CPU premise / self-checks in tests/test_texture_cpu.py)
EPS = 2.0 ** -24
MAG = tuple(f"mag{kx}{ky}" for kx in range(4) for ky in range(4))
PATTERNS = MAG + ("alt", "run3", "distinct")
FRACTIONS = (0.0, 0.25, 0.75)  # mip_level_bias = k + one of these (0.5 would tie under linear-mipmap-nearest)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def dyadic(shape, seed):
    """Texels: multiples of 1/16 in [-4, 4]."""
    return torch.randint(-64, 65, tuple(shape), generator=_gen(seed)).double() / 16


def small_ints(shape, seed):
    """g_out: integers in [-3, 3]."""
    return torch.randint(-3, 4, tuple(shape), generator=_gen(seed)).double()


def frame_xy(B, H, W):
    """(px, py) [B, H, W] of every lookup of a [B, H, W] frame: in the 8 x 8 wave block lane bits 0..2 are px & 7, bits 3..5 py & 7."""
    py, px = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return px.expand(B, H, W), py.expand(B, H, W)


def pattern_texels(name, px, py):
    """Texel (tx, ty) (before the modulo of the level size) each lookup's quad starts at, for a merge pattern of the backward:
    magKXKY -- lookup (px, py) magnifies texel (px >> kx, py >> ky) (mag33: a whole 8 x 8 wave on one quad); alt -- keys equal at lane
    distance 2, different at distance 1 (and 8); run3 -- runs of 3, off the power-of-two alignment; distinct -- every key differs."""
    if name.startswith("mag"):
        return px >> int(name[3]), py >> int(name[4])
    if name == "alt":
        return (px & 1) * 3 + 1, (py & 1) * 5 + 2
    if name == "run3":
        return px // 3, py // 3
    if name == "distinct":
        return 2 * px, 2 * py
    raise ValueError(name)


def exact_uv(tx, ty, ax, ay, w, h):
    """uv = (t + 0.5 + a/8) / size: texel coordinate t + a/8 (a in 0..7) on a level of size (h, w), exact in fp32 for power-of-two sizes."""
    return torch.stack([(tx.double() + 0.5 + ax.double() / 8) / w, (ty.double() + 0.5 + ay.double() / 8) / h], -1)


def exact_field(pattern, B, H, W, size, C, mode, seed, k=0, tex_batch=1, levels=None):
    """A 2-D case in which every fp32 operation of the kernel is exact: power-of-two texture ``size`` (h, w) with a dyadic custom stack
    of ``levels`` levels (mipmap modes), uv on texel centres + a/8 of level k (so that level k + 1 sees sixteenths), bias k + FRACTIONS,
    small-integer g_out.  -> dict(tex, mip, uv, bias, g), float64."""
    mipmap = mode in ("linear-mipmap-nearest", "linear-mipmap-linear")
    sizes = mip_sizes(*size)[: levels] if mipmap else [size]
    tex = dyadic((tex_batch,) + tuple(size) + (C,), seed)
    mip = [dyadic((tex_batch, h, w, C), seed + 1 + l) for l, (h, w) in enumerate(sizes[1:])] if mipmap else None
    k = min(k, len(sizes) - 1)
    h, w = sizes[k]
    px, py = frame_xy(B, H, W)
    tx, ty = pattern_texels(pattern, px, py)
    a = torch.randint(0, 8, (2, B, H, W), generator=_gen(seed + 50))
    uv = exact_uv(tx % w, ty % h, a[0], a[1], w, h)
    bias = None
    if mipmap:
        fr = torch.tensor(FRACTIONS, dtype=torch.float64)[(px + 2 * py) % 3]
        bias = torch.where(torch.tensor(k + 1 < len(sizes)), k + fr, torch.full_like(fr, float(k)))
    return dict(tex=tex, mip=mip, uv=uv, bias=bias, g=small_ints((B, H, W, C), seed + 60))


def coord_scale(uv, tex, cube):
    """Per lookup: a bound on |texel coordinate| of level 0, the scale of the fp32 rounding of the coordinate and so of the weights."""
    if cube:
        return torch.full(uv.shape[:-1], 2.0 * tex.shape[-2], dtype=torch.float64, device=uv.device)
    return uv[..., 0].double().abs() * tex.shape[-2] + uv[..., 1].double().abs() * tex.shape[-3] + 2.0


def g_tex_bounds(tex, uv, g, uv_da=None, mip_level_bias=None, mip=None, A=64.0, **kw):
    """Per-texel bounds on |fp32 g_tex - float64 g_tex|: 2 EPS ((n + 8) |g|-weighted magnitude + sum over terms |g| (A + X)), with n the
    number of terms a texel receives (R.terms unit pass), X the lookup's coordinate scale (the weights are computed from fp32
    coordinates: their error is ~ |x| EPS) and A for the level fraction and the products.  One tensor per level of a custom stack;
    with the internal chain (mipmap modes, mip=None) one tensor for ``tex`` that also carries the box-filter adjoint's pushes."""
    cube = kw.get("boundary_mode") == "cube"
    absg = g.double().abs()
    mag = terms(tex, uv, absg, uv_da, mip_level_bias, mip, **kw)
    cnt = terms(tex, uv, torch.ones_like(absg), uv_da, mip_level_bias, mip, unit=True, **kw)
    crd = terms(tex, uv, absg * (A + coord_scale(uv, tex, cube))[..., None], uv_da, mip_level_bias, mip, unit=True, **kw)
    per = [2 * EPS * ((n + 8) * m + c) for m, n, c in zip(mag, cnt, crd)]
    mode = kw.get("filter_mode", "auto")
    if mip is None and len(per) > 1 and mode != "linear" and mode != "nearest":
        leaf = tex.detach().double().clone().requires_grad_(True)
        chain = mip_chain(leaf, kw.get("max_mip_level"))
        Lc = len(chain)
        return [torch.autograd.grad(chain, leaf, [b + 2 * EPS * (Lc + 2) * m for b, m in zip(per, mag)])[0]]
    return per
