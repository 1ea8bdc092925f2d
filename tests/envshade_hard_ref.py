"""EnvironmentLight.shade with its reverse mode written out by hand, statement by statement as csrc/envshade.hip takes them, in any
dtype -- the yardstick of tests/test_envshade_adversarial_cpu.py and tests/test_envshade_adversarial_gpu.py -- and the named hard cases.

``evaluate(case, dtype)`` returns, per quantity (``quantities``: the values, the five per-pixel gradients, g_diffuse, every g_specular[l]),
the value and its MAGNITUDE: the same chain with the absolute value of every term and an addition for every subtraction, seeded with
|g_out|.  For a texel gradient that is the scatter of |w lw g_sample|, for a per-pixel gradient the adjoint chain with every coefficient
(weights, texels, directions, 1 / length) at its absolute value.  Errors are measured in units of 2^-24 x magnitude (tests/deriv_ref.py).

Constants.  The kinks of the chain -- lo and hi of the level rule, its 1.0, the 1e-4 under n.v, the 1e-20 under a squared length -- are
decided by the kernel and by the float32 statements on the FLOAT32 values of these numbers (CONST32).  The float64 evaluation the kernel
is held to uses the same float32 values, so a pixel placed exactly on a kink stands on the same side in both.  tests/envshade_cases.reference
holds the float64 values (0.08 is not a float32 number, and a roughness of float32(0.08) lies below it); the hand reverse mode equals
its autograd to 1e-12 with CONST64, the same code on the other set of constants.  0.04 is no kink: both sets hold the double.

Where the hand reverse mode follows the kernel and not autograd of the reference: a tap of weight 0 is not scattered (autograd sends
0 x g there, a NaN if g is one), and a level the lookup does not select receives nothing (tests/texture_ref.texture multiplies every level
by its slot weight, 0 for the others: a NaN g_out reaches every level's quad there).  Only the non-finite cases see either.

MEASURED holds, per case and quantity, what the float32 evaluation of this restatement reaches against its float64 evaluation;
tests/test_envshade_adversarial_cpu.py measures it afresh.  The kernel's bound is 4 x that figure in these units plus 4 ulp of the
float64 value, per element, no element left out.
"""
import functools
import types

import torch

import envshade_cases as C
import texture_ref as T
from deriv_ref import EPS

F64, F32 = torch.float64, torch.float32
FACTOR, FLOOR_ULP = 4.0, 4.0


def f32(v):
    return float(torch.tensor(v, dtype=F32))


CONST32 = types.SimpleNamespace(lo=f32(0.08), hi=f32(0.5), one=1.0, ndv=f32(1e-4), eps=f32(1e-20))
CONST64 = types.SimpleNamespace(lo=0.08, hi=0.5, one=1.0, ndv=1e-4, eps=1e-20)
PIXEL_KEYS = ("g_pos", "g_normal", "g_kd", "g_ks", "g_view")
MUTATIONS = ("drop_one_tap", "corner_third_kept", "level_lost_for_a_work_group", "wrong_side_at_a_kink", "g_view_not_negated")


def quantities(n_levels):
    return ("values",) + PIXEL_KEYS + ("g_diffuse",) + tuple(f"g_specular[{l}]" for l in range(n_levels))


def nextafter32(v, up):
    t = torch.tensor(v, dtype=F32)
    return float(torch.nextafter(t, torch.tensor(float("inf") if up else -float("inf"), dtype=F32)))


# ---------------------------------------------------------------------------------------------- lookups
def _cube_lookup(d):
    """csrc/tex_lookup.h make_lookup on directions [P,3]: the face of the largest |component| (ties x before y before z; a comparison
    with NaN is false), s = sa d[ia] / m, t = sb d[ib] / m."""
    dt = d.dtype
    x, y, z = d.unbind(-1)
    ax, ay, az = x.abs(), y.abs(), z.abs()
    isx = (ax >= ay) & (ax >= az)
    isy = ~isx & (ay >= az)
    face = torch.where(isx, torch.where(x >= 0, 0, 1), torch.where(isy, torch.where(y >= 0, 2, 3), torch.where(z >= 0, 4, 5)))
    tbl = lambda v: torch.tensor(v)[face]
    L = types.SimpleNamespace(face=face, ia=tbl([2, 2, 0, 0, 0, 0]), ib=tbl([1, 1, 2, 2, 1, 1]), im=tbl([0, 0, 1, 1, 2, 2]))
    L.sa, L.sb, L.sm = tbl([-1.0, 1, 1, 1, 1, -1]).to(dt), tbl([-1.0, -1, 1, -1, -1, -1]).to(dt), tbl([1.0, -1, 1, -1, 1, -1]).to(dt)
    g = lambda i: d.gather(1, i[:, None])[:, 0]
    m = g(L.im).abs()
    L.valid = (m > 0) & (m < float("inf"))
    ms = torch.where(L.valid, m, torch.ones_like(m))
    zero = torch.zeros_like(m)
    L.inv_m = torch.where(L.valid, 1 / ms, zero)
    L.s = torch.where(L.valid, L.sa * g(L.ia) / ms, zero)
    L.t = torch.where(L.valid, L.sb * g(L.ib) / ms, zero)
    return L


def _cube_quad(L, S):
    """level_quad on a cube level of size S: rows [P,4] (-1: no tap), w, wx, wy [P,4] with the corner tap's share handed to the other
    three in thirds; w_raw: the same without that share."""
    dt = L.s.dtype
    x, y = (L.s + 1) * 0.5 * S - 0.5, (L.t + 1) * 0.5 * S - 0.5
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    ix, iy = x0.long(), y0.long()
    w = torch.stack(((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy), 1)
    wx = torch.stack((-(1 - fy), 1 - fy, -fy, fy), 1)
    wy = torch.stack((-(1 - fx), -fx, 1 - fx, fx), 1)
    b = torch.zeros_like(ix)
    rows, corner = zip(*[T._cube_rows(b, L.face, ix + dx, iy + dy, S) for dy in (0, 1) for dx in (0, 1)])
    rows, corner = torch.stack(rows, 1), torch.stack(corner, 1)
    dead = corner | ~L.valid[:, None]
    third = torch.tensor(1.0 / 3.0, dtype=dt)
    q = types.SimpleNamespace(rows=torch.where(dead, -1, rows), corner=corner & L.valid[:, None])
    out = []
    for v in (w, wx, wy):
        c = (v * corner).sum(1, keepdim=True)
        out.append(torch.where(dead, torch.zeros_like(v), v + c * third))
    q.w, q.wx, q.wy = out
    q.w_raw = torch.where(dead, torch.zeros_like(w), w)
    return q


def _flat_quad(u, v, H, W):
    """level_quad on a 2-D level under the clamp rule: every tap has a row."""
    x, y = u * W - 0.5, v * H - 0.5
    fin = lambda t: torch.where(torch.isfinite(t), t, torch.zeros_like(t))
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    ix, iy = torch.floor(fin(x)).long(), torch.floor(fin(y)).long()
    cx, cy = (lambda i: i.clamp(0, W - 1)), (lambda i: i.clamp(0, H - 1))
    q = types.SimpleNamespace(rows=torch.stack([cy(iy + dy) * W + cx(ix + dx) for dy in (0, 1) for dx in (0, 1)], 1))
    q.w = torch.stack(((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy), 1)
    q.fx, q.fy = fx, fy
    return q


def _taps(flat, q):
    """[P,4,C] texels of a quad's taps (a tap without a row reads 0 and weighs 0)."""
    return flat[q.rows.clamp(min=0)] * (q.rows >= 0)[..., None].to(flat.dtype)


def _sample(tex, w, lw=None):
    acc = 0
    for t in range(4):
        wt = w[:, t] if lw is None else w[:, t] * lw
        acc = acc + wt[:, None] * tex[:, t]
    return acc


def _normalize(v, eps):
    d = (v * v).sum(-1, keepdim=True)
    ln = torch.sqrt(d.clamp(min=eps))
    return v / ln, d, ln


# ---------------------------------------------------------------------------------------------- the forward
def _forward(case, dt, K):
    B, H, W = case["shape"]
    P = B * H * W
    full = lambda t: t.to(dt).expand(B, H, W, 3).reshape(P, 3)
    pos, n, kd, ks, view = (full(t) for t in case["leaves"])
    f = types.SimpleNamespace(P=P, n=n, kd=kd, ks=ks, K=K, dt=dt, specular=case.get("specular", True))
    f.dif_map = case["dif"].to(dt).reshape(-1, 3)
    f.spec_maps = [m.to(dt).reshape(-1, 3) for m in case["spec"]]
    f.sizes, f.dsize = [m.shape[1] for m in case["spec"]], case["dif"].shape[1]
    f.wo, f.d1, f.len1 = _normalize(view - pos, K.eps)
    f.dn = (f.wo * n).sum(-1, keepdim=True)
    f.refl, f.d2, f.len2 = _normalize(2 * f.dn * n - f.wo, K.eps)
    f.rot = None
    rd, nd = f.refl, n
    if case["mtx"] is not None:
        m = case["mtx"][:, :3, :3].to(dt)
        f.rot = m.expand(B, 3, 3)[:, None].expand(B, H * W, 3, 3).reshape(P, 3, 3)
        per = lambda v: torch.cat([v.reshape(B, H * W, 3)[b] @ m[b if m.shape[0] > 1 else 0].T for b in range(B)])  # (the statement is a matmul)
        rd, nd = per(f.refl), per(n)
    f.Ld = _cube_lookup(nd)
    f.qd = _cube_quad(f.Ld, f.dsize)
    f.Td = _taps(f.dif_map, f.qd)
    f.dif = _sample(f.Td, f.qd.w)
    f.vis = 1 - ks[:, 0:1]
    if not f.specular:
        f.diff_col = kd
        f.shaded = f.dif * kd
        return f
    rough, metal = ks[:, 1], ks[:, 2:3]
    f.omm = 1 - metal
    f.spec_col = f.omm * 0.04 + kd * metal
    f.diff_col = kd * f.omm
    f.shaded = f.dif * f.diff_col
    f.ndv = f.dn[:, 0].clamp(min=K.ndv)
    fg = C.fg_table().to(dt)
    f.fg_h, f.fg_w = fg.shape[1], fg.shape[2]
    f.qf = _flat_quad(f.ndv, rough, f.fg_h, f.fg_w)
    f.Tf = fg.reshape(-1, 2)[f.qf.rows]
    lut = _sample(f.Tf, f.qf.w)
    f.fgA, f.fgB = lut[:, 0:1], lut[:, 1:2]
    Ln = len(f.sizes)
    lo, hi, one = (torch.tensor(v, dtype=dt) for v in (K.lo, K.hi, K.one))
    f.mip = torch.where(rough < hi, (rough.clamp(lo, hi) - lo) / (hi - lo) * (Ln - 2), (rough.clamp(hi, one) - hi) / (one - hi) + Ln - 2)
    f.live = (f.mip >= 0) & (f.mip <= Ln - 1)
    level = torch.where(torch.isnan(f.mip), torch.zeros_like(f.mip), f.mip).clamp(0, Ln - 1)
    l0 = torch.floor(level).clamp(max=Ln - 1)
    fr = level - l0
    f.lv = (l0.long(), (l0.long() + 1).clamp(max=Ln - 1))
    f.lw = (1 - fr, fr)
    f.in1 = (rough < hi) & (rough >= lo) & (rough <= hi)
    f.in2 = ~(rough < hi) & (rough >= hi) & (rough <= one)
    f.slope1, f.slope2 = (Ln - 2) / (hi - lo), 1 / (one - hi)
    f.Ls = _cube_lookup(rd)
    f.qs, f.Ts, f.lwl = [], [], []
    spec = 0
    for l, S in enumerate(f.sizes):
        q = _cube_quad(f.Ls, S)
        tex = _taps(f.spec_maps[l], q)
        zero = torch.zeros_like(fr)
        lwl = torch.where(f.lv[0] == l, f.lw[0], zero) + torch.where((f.lv[1] == l) & (f.lv[0] != l), f.lw[1], zero)
        spec = spec + _sample(tex, q.w, lwl)
        f.qs.append(q); f.Ts.append(tex); f.lwl.append(lwl)
    f.spec = spec
    f.reflectance = f.spec_col * f.fgA + f.fgB
    f.shaded = f.shaded + f.spec * f.reflectance
    return f


# ---------------------------------------------------------------------------------------------- the backward, signed or in magnitudes
def _backward(f, go, mag, mutate=None, at=None):
    """-> dict of per-pixel gradients [P,3] and map gradients [6 S S,3].  mag: every coefficient at its absolute value, every
    subtraction an addition.  ``mutate`` (signed only) breaks one piece; ``at`` names the pixel(s) it breaks it at."""
    a = torch.abs if mag else (lambda x: x)
    sg = 1.0 if mag else -1.0
    dt, P = f.dt, f.P
    z3 = lambda: torch.zeros(P, 3, dtype=dt)
    pix = torch.arange(P)

    def quad_grad(q, tex, g):
        v = (g[:, None, :] * a(tex)).sum(-1)  # [P,4]
        return (a(q.wx) * v).sum(1), (a(q.wy) * v).sum(1), (a(q.w) * v).sum(1)

    def dir_grad(L, gu, gv):
        gsu, gtv = gu * L.inv_m, gv * L.inv_m
        d = z3()
        d.scatter_add_(1, L.ia[:, None], (gsu * a(L.sa))[:, None])
        d.scatter_add_(1, L.ib[:, None], (gtv * a(L.sb))[:, None])
        d.scatter_add_(1, L.im[:, None], (sg * (gsu * a(L.s) + gtv * a(L.t)) * a(L.sm))[:, None])
        return d * L.valid[:, None].to(dt)

    def scatter(n_rows, q, lw, g, w=None, skip=None):
        out = torch.zeros(n_rows, 3, dtype=dt)
        w = q.w if w is None else w
        for t in range(4):
            wt = a(w[:, t]) if lw is None else a(w[:, t] * lw)
            on = (q.rows[:, t] >= 0) & (wt != 0)
            if skip is not None:
                on = on & ~skip(t)
            out.index_add_(0, q.rows[on, t], (wt[:, None] * g)[on])
        return out

    def normalize_bwd(y, d, ln, g):
        r = g / ln
        s = (a(y) * g).sum(-1, keepdim=True) / ln
        return torch.where(d >= f.K.eps, r + sg * a(y) * s, r)

    go = a(go)
    gsh = go * a(f.vis)
    g_ksx = sg * (go * a(f.shaded)).sum(-1)
    gdv = gsh * a(f.diff_col)
    g_dc = gsh * a(f.dif)
    gx, gy, _ = quad_grad(f.qd, f.Td, gdv)
    half = 0.5 * f.dsize
    g_nd = dir_grad(f.Ld, gx * half, gy * half)
    out = {"g_diffuse": scatter(f.dif_map.shape[0], f.qd, None, gdv, w=f.qd.w_raw if mutate == "corner_third_kept" else None)}
    g_kd, g_rd = g_dc, z3()
    g_rough = g_metal = g_dn = torch.zeros(P, dtype=dt)
    if f.specular:
        gsv = gsh * a(f.reflectance)
        g_R = gsh * a(f.spec)
        g_sc = g_R * a(f.fgA)
        g_fgA, g_fgB = (g_R * a(f.spec_col)).sum(-1), g_R.sum(-1)
        g_kd = g_sc * a(f.ks[:, 2:3]) + g_dc * a(f.omm)
        g_metal = ((g_sc * a(f.kd)).sum(-1) + sg * 0.04 * g_sc.sum(-1)) + sg * (g_dc * a(f.kd)).sum(-1)
        v = g_fgA[:, None] * a(f.Tf[:, :, 0]) + g_fgB[:, None] * a(f.Tf[:, :, 1])
        fx, fy = f.qf.fx, f.qf.fy
        gxf = a(1 - fy) * (v[:, 1] + sg * v[:, 0]) + a(fy) * (v[:, 3] + sg * v[:, 2])
        gyf = a(1 - fx) * (v[:, 2] + sg * v[:, 0]) + a(fx) * (v[:, 3] + sg * v[:, 1])
        g_dn = torch.where(f.dn[:, 0] >= f.K.ndv, gxf * f.fg_w, torch.zeros_like(gxf))
        g_rough = gyf * f.fg_h
        gu = gv = glev = 0
        for l, S in enumerate(f.sizes):
            q, tex, lwl = f.qs[l], f.Ts[l], f.lwl[l]
            gxl, gyl, gsl = quad_grad(q, tex, gsv)
            fac = a(lwl) * 0.5 * S
            gu, gv = gu + gxl * fac, gv + gyl * fac
            hi_slot, lo_slot = (f.lv[1] == l).to(dt), (f.lv[0] == l).to(dt)
            glev = glev + (hi_slot + sg * lo_slot) * gsl * (f.lv[0] != f.lv[1]).to(dt)
            skip, lw = None, lwl
            if mutate == "drop_one_tap" and l == at[1]:
                skip = lambda t: (pix == at[0]) & (t == at[2])
            if mutate == "level_lost_for_a_work_group" and l == at[1]:
                lw = torch.where((pix >= at[0]) & (pix < at[0] + 256), torch.zeros_like(lwl), lwl)
            out[f"g_specular[{l}]"] = scatter(f.spec_maps[l].shape[0], q, lw, gsv, skip=skip,
                                              w=q.w_raw if mutate == "corner_third_kept" else None)
        g_rd = dir_grad(f.Ls, gu, gv)
        slope = f.in1.to(dt) * f.slope1 + f.in2.to(dt) * f.slope2
        if mutate == "wrong_side_at_a_kink":
            slope = torch.where(pix == at[0], torch.zeros_like(slope), slope)
        g_rough = g_rough + torch.where(f.live, glev * slope, torch.zeros_like(glev))
    rot_t = (lambda g: g) if f.rot is None else (lambda g: torch.einsum("pji,pj->pi", a(f.rot), g))
    g_refl, g_n = rot_t(g_rd), rot_t(g_nd)
    g_rr = normalize_bwd(f.refl, f.d2, f.len2, g_refl)
    g_dn = g_dn + 2 * (g_rr * a(f.n)).sum(-1)
    g_wo = g_dn[:, None] * a(f.n) + sg * g_rr
    g_n = g_n + a(2 * f.dn) * g_rr + g_dn[:, None] * a(f.wo)
    g_wr = normalize_bwd(f.wo, f.d1, f.len1, g_wo)
    out.update(g_pos=sg * g_wr, g_normal=g_n, g_kd=g_kd, g_ks=torch.stack((g_ksx, g_rough, g_metal), -1), g_view=g_wr)
    return out


def _value_magnitude(f):
    m = _sample(f.Td.abs(), f.qd.w.abs()) * f.diff_col.abs()
    if f.specular:
        ms = sum(_sample(tex.abs(), q.w.abs(), lwl.abs()) for q, tex, lwl in zip(f.qs, f.Ts, f.lwl))
        m = m + ms * (f.spec_col.abs() * f.fgA.abs() + f.fgB.abs())
    return m * f.vis.abs()


def evaluate(case, dtype=F64, consts=CONST32, mutate=None, at=None, magnitudes=True):
    """-> (values: quantity -> tensor in the shapes autograd returns, magnitudes: the same keys or None)."""
    B, H, W = case["shape"]
    f = _forward(case, dtype, consts)
    go = case["go"].to(dtype).reshape(f.P, 3)
    res = []
    for mag in ((False, True) if magnitudes else (False,)):
        g = _backward(f, go, mag, None if mag else mutate, at)
        o = {"values": (_value_magnitude(f) if mag else f.shaded * f.vis).reshape(B, H, W, 3)}
        for key, leaf in zip(PIXEL_KEYS, case["leaves"]):
            t = g[key].reshape(B, H, W, 3)
            if mutate == "g_view_not_negated" and key == "g_view" and not mag:
                t = t.clone()
                t[0] = -t[0]
            o[key] = t.sum_to_size(leaf.shape)
        o["g_diffuse"] = g["g_diffuse"].reshape(case["dif"].shape)
        for l, m in enumerate(case["spec"]):
            o[f"g_specular[{l}]"] = g[f"g_specular[{l}]"].reshape(m.shape) if f.specular else torch.zeros(m.shape, dtype=dtype)
        res.append(o)
    f.quads = {"g_diffuse": f.qd.rows}
    if f.specular:
        for l in range(len(f.sizes)):
            f.quads[f"g_specular[{l}]"] = torch.where((f.lwl[l] != 0)[:, None], f.qs[l].rows, -1)
    evaluate.last_forward = f
    return res[0], (res[1] if magnitudes else None)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 values, magnitudes, the forward) of a case on the float32 constants: computed once per process, never written to."""
    val, mag = evaluate(build(name))
    return val, mag, evaluate.last_forward


def autograd(case):
    """quantity -> autograd of tests/envshade_cases.reference in float64 (on its own, float64, constants)."""
    leaves = [t.clone().requires_grad_(True) for t in case["leaves"]]
    spec, dif = [t.clone().requires_grad_(True) for t in case["spec"]], case["dif"].clone().requires_grad_(True)
    B, H, W = case["shape"]
    out = C.reference(spec, dif, C.fg_table(), [t.expand(B, H, W, 3) for t in leaves], case.get("specular", True), case["mtx"])
    wrt = leaves + [dif] + spec
    gs = torch.autograd.grad((out * case["go"]).sum(), wrt, allow_unused=True)
    res = {"values": out.detach()}
    for key, g, t in zip(PIXEL_KEYS + ("g_diffuse",) + tuple(f"g_specular[{l}]" for l in range(len(spec))), gs, wrt):
        res[key] = torch.zeros_like(t) if g is None else g
    return res


# ---------------------------------------------------------------------------------------------- the unit and the bound
def units(got, ref, mag):
    """max |got - ref| / (2^-24 magnitude) over the elements with a finite float64 value; an element nothing feeds must be exactly 0."""
    got = got.double()
    fin = torch.isfinite(ref) & torch.isfinite(mag)
    dead = fin & (mag == 0)
    assert bool((got[dead] == 0).all()), "an element nothing feeds is not zero"
    use = fin & ~dead
    if not bool(use.any()):
        return 0.0
    return float(((got - ref).abs()[use] / (EPS * mag[use])).max())


def violations(got, ref, mag, figure, where=None):
    """indices where |got - ref| > 2^-24 (4 figure magnitude + 4 |ref|) among the elements with a finite float64 value (all of them
    outside the non-finite cases); a non-finite ``got`` there violates.  ``where``: only these elements."""
    got = got.double()
    fin = torch.isfinite(ref) & torch.isfinite(mag)
    if where is not None:
        fin = fin & where
    ok = (got - ref).abs() <= EPS * (FACTOR * figure * mag + FLOOR_ULP * ref.abs())
    return torch.nonzero(fin & ~ok)


def measure(name):
    """quantity -> units of the float32 evaluation of the restatement against its float64 evaluation."""
    case = build(name)
    ref, mag, _ = reference(name)
    x32, _ = evaluate(case, F32, magnitudes=False)
    return {k: units(x32[k], ref[k], mag[k]) for k in ref}


# ---------------------------------------------------------------------------------------------- cases
def _r32(t):
    return t.float().double()


def maps(sizes, dsize, seed=0, scale=4.0):
    g = C._gen(2000 + seed)
    spec = [_r32(torch.rand(6, s, s, 3, generator=g, dtype=F64) * scale) for s in sizes]
    return spec, _r32(torch.rand(6, dsize, dsize, 3, generator=g, dtype=F64) * scale)


LIGHTS = dict(C.LIGHTS)
LIGHTS.update({
    "d_64_32_16_dif32": ((64, 32, 16), 32),  # the diffuse map on the merge route
    "e_4_2_1_dif1": ((4, 2, 1), 1),
    "f_2_1_1_dif2": ((2, 1, 1), 2),
    "g_16_to_1_1": ((16, 8, 4, 2, 1, 1), 16),
    "h_16_levels": ((16, 8, 4, 2) + (1,) * 12, 16),
})


@functools.lru_cache(maxsize=None)
def _filler_seed(light, shape, view, xfm_kind):
    """the first seed from C.SEED on for which tests/envshade_cases.near_kink finds no pixel of the random frame near a kink."""
    sizes, dsize = LIGHTS[light]
    for seed in range(C.SEED, C.SEED + 400):
        leaves = C.frame(shape, seed, view)
        if not bool(C.near_kink(sizes, dsize, leaves, True, C.transform(xfm_kind, shape[0], seed)).any()):
            return seed
    raise AssertionError("no seed without a pixel near a kink")


def base(light, shape, view="full", xfm="none", go_seed=0):
    """A random case: the light's maps, a frame whose pixels all stand clear of every kink, a random g_out."""
    sizes, dsize = LIGHTS[light]
    seed = _filler_seed(light, tuple(shape), view, xfm)
    spec, dif = maps(sizes, dsize)
    go = _r32(torch.randn(*shape, 3, generator=C._gen(seed + 500 + go_seed), dtype=F64))
    B, H, W = shape
    return dict(light=light, shape=tuple(shape), spec=spec, dif=dif, leaves=C.frame(shape, seed, view), mtx=C.transform(xfm, shape[0], seed),
                go=go, filler=torch.ones(B, H, W, dtype=torch.bool), wants=None, holds="", specular=True)


def place(case, rows, pos=None, n=None, view=None, rough=None, ks=None, kd=None):
    """Overwrite pixels ``rows`` (indices into the flat frame) of a full-form case; they stop being filler."""
    B, H, W = case["shape"]
    flat = lambda i: case["leaves"][i].reshape(B * H * W, 3)
    for i, v in ((0, pos), (1, n), (2, kd), (3, ks), (4, view)):
        if v is not None:
            flat(i)[rows] = _r32(torch.as_tensor(v, dtype=F64))
    if rough is not None:
        flat(3)[rows, 1] = _r32(torch.as_tensor(rough, dtype=F64))
    case["filler"].reshape(-1)[rows] = False


def look_along(case, rows, d):
    """Both lookup directions of pixels ``rows`` along d [len(rows),3]: the point at the origin, the camera at 2 d, the normal
    float32(d / |d|).  Every operation treats the components alike, so ties between |components| and exact zeros survive in float32 and
    in float64: the reflection is (2 n.wo) n - wo with n and wo both along d."""
    d = torch.as_tensor(d, dtype=F64)
    place(case, rows, pos=torch.zeros_like(d), view=2 * d, n=_r32(d / d.norm(dim=-1, keepdim=True)))


AXES = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
EDGES = [[sx, sy, 0] for sx in (1, -1) for sy in (1, -1)] + [[sx, 0, sz] for sx in (1, -1) for sz in (1, -1)] + \
        [[0, sy, sz] for sy in (1, -1) for sz in (1, -1)]
CORNERS = [[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
UP, DN = nextafter32(1.0, True), nextafter32(1.0, False)
BESIDE = [[1, UP, 0.3], [1, DN, 0.3], [-0.2, DN, -1], [0.6, -1, -UP]]  # one float32 step to either side of a face boundary
GEOMETRY = AXES + EDGES + CORNERS + BESIDE

ROUGH_KINKS = [CONST32.lo, CONST32.hi, 1.0, 0.0, 1.5]
ROUGH_BESIDE = [nextafter32(v, up) for v in (CONST32.lo, CONST32.hi, 1.0) for up in (False, True)]
NDV_KINKS = [CONST32.ndv, nextafter32(CONST32.ndv, False), nextafter32(CONST32.ndv, True), 0.0, f32(-0.3), 1.0]


def _lights(name):
    light = name[len("light_"):]
    c = base(light, (1, 1, 130), "full", "one" if light[0] in "bdg" else "none")
    c["holds"] = f"sizes {LIGHTS[light]}"
    return c


def _wanted(name):
    c = base("b_64_32_16", (1, 9, 8), "full", "none")
    n = len(c["spec"])
    spec_keys = [f"g_specular[{l}]" for l in range(n)]
    c["wants"] = {"wanted_no_diffuse": list(PIXEL_KEYS) + spec_keys,
                  "wanted_no_level0": list(PIXEL_KEYS) + ["g_diffuse"] + spec_keys[1:],
                  "wanted_only_maps": ["g_diffuse"] + spec_keys,
                  "wanted_only_view": ["g_view"]}[name]
    c["holds"] = "wants " + ", ".join(c["wants"])
    return c


def _concentration(name):
    """Every pixel looks along one of a few directions: all lanes of all waves add into the same quads."""
    kind = name[len("conc_"):]
    light = "a_8_4_2" if kind.endswith("lds") else "d_64_32_16_dif32"
    shape = (2, 16, 16) if kind.startswith("frame") else (1, 1, 1024)
    c = base(light, shape, "full", "none")
    P = shape[0] * shape[1] * shape[2]
    g = C._gen(31)
    dirs = _r32(torch.randn(16, 3, generator=g, dtype=F64))
    dirs[1] = -dirs[0] * torch.tensor([1.0, 0.5, 2.0], dtype=F64)  # (another face than dirs[0])
    which = {"two_quads": torch.arange(P) % 2, "quad_per_wave": torch.arange(P) // 64}.get(kind, torch.zeros(P, dtype=torch.long))
    look_along(c, torch.arange(P), dirs[which])
    # roughness inside (lo, hi): levels 0 and 1 of a three-level light, both slots live
    place(c, torch.arange(P), rough=0.12 + 0.3 * torch.rand(P, generator=g, dtype=F64))
    c["which"], c["n_dirs"] = which, int(which.max()) + 1
    c["holds"] = f"every pixel of direction group k has the quads of the group's first pixel, {c['n_dirs']} groups, levels 0 and 1"
    return c


def _geometry(name):
    light = {"geo_S1": "e_4_2_1_dif1", "geo_S2": "a_8_4_2", "geo_S16": "b_64_32_16", "geo_S32": "d_64_32_16_dif32"}[name]
    c = base(light, (1, 1, 65), "full", "none")
    rows = torch.arange(len(GEOMETRY))
    look_along(c, rows, GEOMETRY)
    place(c, rows[-len(BESIDE):], n=BESIDE)  # (the normal itself one step beside the boundary: the diffuse lookup does not normalise it)
    place(c, rows, rough=0.75)  # the upper branch: level L - 1.5, the two smallest levels
    c["holds"] = "rows 0..5 on the axes, 6..17 on the face boundaries, 18..25 on the corners, 26..29 one float32 step beside a boundary"
    return c


def _kinks(name):
    if name.startswith("kink_roughness"):
        c = base("c_64_to_4", (1, 1, 65), "full", "none")
        c["rough"] = ROUGH_KINKS if name == "kink_roughness" else ROUGH_BESIDE
        for i, r in enumerate(c["rough"]):
            place(c, torch.arange(4 * i, 4 * i + 4), rough=r)
        c["holds"] = "rows 4i..4i+3 have roughness c['rough'][i]; the level is exactly 0 at lo, L - 2 at hi, L - 1 at 1"
    else:
        c = base("b_64_32_16", (1, 1, 65), "full", "none")
        for i, v in enumerate(NDV_KINKS):
            rows = torch.arange(4 * i, 4 * i + 4)
            nxy = _r32(torch.rand(4, 2, generator=C._gen(41 + i), dtype=F64) - 0.5)
            place(c, rows, pos=torch.zeros(4, 3), view=torch.tensor([[0.0, 0.0, 2.0]]).expand(4, 3),
                  n=torch.cat((nxy, torch.full((4, 1), v, dtype=F64)), -1))
        c["holds"] = "rows 4i..4i+3 have n.v exactly NDV_KINKS[i]: wo is (0, 0, 1) exactly and n.z the value"
    return c


DEGENERATE = ("zero normal", "view == pos", "|view - pos| = 1e-11", "|view - pos| = 1e-9", "|n| = 1e-3", "|n| = 1e3")


def _degenerate(name):
    c = base("b_64_32_16", (1, 1, 65), "full", "none")
    B, H, W = c["shape"]
    pos, n = c["leaves"][0].reshape(-1, 3), c["leaves"][1].reshape(-1, 3)
    r = lambda i: torch.arange(4 * i, 4 * i + 4)
    place(c, r(0), n=torch.zeros(4, 3))
    place(c, r(1), view=pos[r(1)].clone())
    for i, d in ((2, 1e-11), (3, 1e-9)):
        u = _r32(torch.randn(4, 3, generator=C._gen(50 + i), dtype=F64))
        place(c, r(i), pos=torch.zeros(4, 3), view=_r32(u / u.norm(dim=-1, keepdim=True) * d))
    place(c, r(4), n=_r32(n[r(4)] * 1e-3))
    place(c, r(5), n=_r32(n[r(5)] * 1e3))
    c["holds"] = "rows 4i..4i+3: " + "; ".join(DEGENERATE)
    return c


def _transforms(name):
    kind = name[len("xfm_"):]
    shape = (3, 5, 7) if kind == "three" else (1, 1, 65)
    c = base("b_64_32_16", shape, "full", "none")
    m = torch.eye(4, dtype=F64).repeat(shape[0], 1, 1)
    g = C._gen(61)
    if kind == "zero":
        m[:, :3, :3] = 0
    elif kind == "reflection":
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))
        m[0, :3, :3] = q * -torch.linalg.det(q).sign()
    elif kind == "shear":
        m[0, :3, :3] = torch.tensor([[1.0, 0.75, -0.5], [0.0, 1.0, 1.5], [0.0, 0.0, 1.0]], dtype=F64)
    elif kind in ("scale_1e-20", "scale_1e20"):
        m[0, :3, :3] = torch.eye(3, dtype=F64) * float(kind[len("scale_"):])
    else:  # three different matrices: a rotation, a reflection with a shear, a scaled rotation
        q, _ = torch.linalg.qr(torch.randn(3, 3, 3, generator=g, dtype=F64))
        m[:, :3, :3] = q
        m[1, :3, :3] = m[1, :3, :3] @ torch.tensor([[1.0, 0.5, 0.0], [0.0, -1.0, 0.0], [0.0, 0.25, 1.0]], dtype=F64)
        m[2, :3, :3] *= 7.0
    m[:, :3, 3] = torch.tensor([5.0, -7.0, 11.0], dtype=F64)  # a translation column, which a direction must not see
    c["mtx"] = _r32(m)
    c["holds"] = f"{kind}; the translation column is (5, -7, 11)"
    return c


FRAME_SHAPES = {"frame_1x8x8": (1, 8, 8), "frame_1x8x9": (1, 8, 9), "frame_1x7x64": (1, 7, 64), "frame_3x16x8": (3, 16, 8),
                "frame_list255": (1, 1, 255), "frame_list256": (1, 1, 256)}


def _frames(name):
    shape = FRAME_SHAPES[name]
    c = base("b_64_32_16", shape, "image", "per_image" if shape[0] > 1 else "one")
    c["holds"] = f"shape {shape}"
    return c


def _magnitudes(name):
    c = base("b_64_32_16", (1, 1, 130), "full", "none")
    g = C._gen(71)
    if name == "mag_hdr_maps":  # texels at 1e30, 1e-30 and 0 among ordinary ones
        for m in c["spec"] + [c["dif"]]:
            pick = torch.randint(0, 8, m.shape[:3], generator=g)
            for code, v in ((0, 1e30), (1, 1e-30), (2, 0.0)):
                m[pick == code] = _r32(m[pick == code] * v)
    elif name == "mag_g_out_1e20":
        e = torch.randint(-2, 21, c["go"].shape[:3], generator=g).double()
        c["go"] = _r32(c["go"] * 10.0 ** e[..., None])
    else:  # positions at 1e4, the camera 1e-2 away
        pos = _r32(c["leaves"][0] * 1e4 / 0.3)
        off = torch.randn(c["leaves"][0].shape, generator=g, dtype=F64)
        c["leaves"][0] = pos
        c["leaves"][4] = _r32(pos + 1e-2 * off / off.norm(dim=-1, keepdim=True))
        c["filler"][:] = False
    c["holds"] = name
    return c


def _operands(name):
    c = base("b_64_32_16", (2, 9, 8), "image", "none")
    pos, n, kd, ks, view = c["leaves"]
    if name == "operands_broadcast":  # kd [1,1,1,3], ks [B,1,1,3], gb_normal [1,H,W,3], an expanded view_pos
        c["leaves"] = [pos, n[:1].clone(), kd[:1, :1, :1].clone(), ks[:, :1, :1].clone(), view]
        c["expanded"] = (4,)  # the kernel is handed view_pos.expand(B, H, W, 3): strides (3, 0, 0, 1); the gradient goes to the [B,1,1,3] leaf
    else:  # gb_pos [B,H,1,3]: broadcast along W only, which the strides cannot say (the copy path of _EnvShadePlan)
        c["leaves"] = [pos[:, :, :1].clone(), n, kd, ks, view]
    c["filler"][:] = False  # (the broadcast frame is another frame than the seed was chosen for; test_no_filler... re-checks it)
    c["holds"] = "shapes " + ", ".join(str(list(t.shape)) for t in c["leaves"])
    return c


BAD_PIXEL = 37
NONFINITE = {"nonfinite_nan_normal": (1, float("nan")), "nonfinite_inf_pos": (0, float("inf")), "nonfinite_nan_kd": (2, float("nan")),
             "nonfinite_nan_g_out": (None, float("nan"))}


def _nonfinite(name):
    benign = name.endswith("_benign")
    c = base("b_64_32_16", (1, 1, 65), "full", "none")
    which, v = NONFINITE[name[:-len("_benign")] if benign else name]
    if not benign:
        (c["go"] if which is None else c["leaves"][which])[0, 0, BAD_PIXEL] = v
        c["filler"][0, 0, BAD_PIXEL] = False
    c["holds"] = f"pixel {BAD_PIXEL} alone is not finite" if not benign else "the same frame with every pixel finite"
    return c


HIDDEN_BIG, HIDDEN_KINK = (298, 299), 20


def _hidden(name):
    """The case the per-tensor bound is blind on: 300 pixels, more than a work-group; rows 0..7 look at the eight corners of the cube;
    row 20 has roughness float32(lo) exactly; the g_out of the last two pixels (one between levels 0 and 1, one between 1 and 2) is 2^24
    times the others', so every tensor's largest element is about 2^24 times an ordinary one."""
    c = base("b_64_32_16", (1, 1, 300), "full", "none")
    look_along(c, torch.arange(8), CORNERS)
    place(c, torch.arange(8), rough=0.3)
    place(c, torch.tensor([HIDDEN_KINK]), rough=CONST32.lo)
    place(c, torch.tensor(HIDDEN_BIG), rough=[0.3, 0.75])
    c["go"][0, 0, list(HIDDEN_BIG)] *= 2.0 ** 24
    c["holds"] = "rows 0..7 on the corners, row 20 at roughness lo, g_out of rows 298 and 299 scaled by 2^24"
    return c


FAMILIES = (
    (_lights, tuple("light_" + k for k in LIGHTS)),
    (_wanted, ("wanted_no_diffuse", "wanted_no_level0", "wanted_only_maps", "wanted_only_view")),
    (_concentration, ("conc_list_lds", "conc_list_merge", "conc_frame_lds", "conc_frame_merge", "conc_two_quads", "conc_quad_per_wave")),
    (_geometry, ("geo_S1", "geo_S2", "geo_S16", "geo_S32")),
    (_kinks, ("kink_roughness", "kink_roughness_one_ulp_beside", "kink_n_dot_v")),
    (_degenerate, ("degenerate_vectors",)),
    (_transforms, ("xfm_zero", "xfm_reflection", "xfm_shear", "xfm_scale_1e-20", "xfm_scale_1e20", "xfm_three")),
    (_frames, tuple(FRAME_SHAPES)),
    (_magnitudes, ("mag_hdr_maps", "mag_g_out_1e20", "mag_far_positions")),
    (_operands, ("operands_broadcast", "operands_pos_BH13")),
    (_nonfinite, tuple(NONFINITE)),
    (_hidden, ("hidden_under_the_largest",)),
)
CASES = tuple(n for _, names in FAMILIES for n in names)
_BUILDERS = {n: fn for fn, names in FAMILIES for n in names}
_BUILDERS.update({n + "_benign": _nonfinite for n in NONFINITE})


def build(name):
    c = _BUILDERS[name](name)
    c["name"] = name
    return c


def figure(name, key):
    return MEASURED[name][key]


MEASURED = {
    "light_a_8_4_2": {"values": 21.535, "g_pos": 1.834, "g_normal": 2.677, "g_kd": 19.182, "g_ks": 8.690, "g_view": 1.834, "g_diffuse": 3.850, "g_specular[0]": 766.575, "g_specular[1]": 82.296, "g_specular[2]": 15.983},
    "light_b_64_32_16": {"values": 230.527, "g_pos": 10.995, "g_normal": 16.815, "g_kd": 44.217, "g_ks": 44.185, "g_view": 10.995, "g_diffuse": 2188.060, "g_specular[0]": 5196.751, "g_specular[1]": 11389.232, "g_specular[2]": 13899.800},
    "light_c_64_to_4": {"values": 91.559, "g_pos": 5.428, "g_normal": 10.504, "g_kd": 42.569, "g_ks": 30.779, "g_view": 5.428, "g_diffuse": 69.397, "g_specular[0]": 1162.567, "g_specular[1]": 10554.222, "g_specular[2]": 287.201, "g_specular[3]": 2412.871, "g_specular[4]": 268.696},
    "light_d_64_32_16_dif32": {"values": 187.580, "g_pos": 10.995, "g_normal": 16.519, "g_kd": 42.235, "g_ks": 43.098, "g_view": 10.995, "g_diffuse": 3530.568, "g_specular[0]": 5196.751, "g_specular[1]": 11389.232, "g_specular[2]": 13899.800},
    "light_e_4_2_1_dif1": {"values": 4.718, "g_pos": 1.071, "g_normal": 1.863, "g_kd": 4.792, "g_ks": 3.769, "g_view": 1.071, "g_diffuse": 1.777, "g_specular[0]": 216.624, "g_specular[1]": 7.360, "g_specular[2]": 2.781},
    "light_f_2_1_1_dif2": {"values": 6.452, "g_pos": 1.363, "g_normal": 1.736, "g_kd": 4.701, "g_ks": 3.849, "g_view": 1.363, "g_diffuse": 3.850, "g_specular[0]": 33.530, "g_specular[1]": 2.260, "g_specular[2]": 2.781},
    "light_g_16_to_1_1": {"values": 24.045, "g_pos": 2.000, "g_normal": 4.475, "g_kd": 38.296, "g_ks": 11.037, "g_view": 2.000, "g_diffuse": 2188.060, "g_specular[0]": 403.750, "g_specular[1]": 200.777, "g_specular[2]": 44.425, "g_specular[3]": 73.732, "g_specular[4]": 7.317, "g_specular[5]": 2.338},
    "light_h_16_levels": {"values": 19.891, "g_pos": 5.815, "g_normal": 15.989, "g_kd": 21.300, "g_ks": 11.720, "g_view": 5.815, "g_diffuse": 4584.507, "g_specular[0]": 772.974, "g_specular[1]": 88.604, "g_specular[2]": 477.480, "g_specular[3]": 18.726, "g_specular[4]": 7.704, "g_specular[5]": 10.542, "g_specular[6]": 711.313, "g_specular[7]": 24.752, "g_specular[8]": 30.406, "g_specular[9]": 68.712, "g_specular[10]": 92.180, "g_specular[11]": 63.393, "g_specular[12]": 64.511, "g_specular[13]": 62.951, "g_specular[14]": 12.608, "g_specular[15]": 11.862},
    "wanted_no_diffuse": {"values": 40.169, "g_pos": 9.515, "g_normal": 12.640, "g_kd": 26.981, "g_ks": 32.691, "g_view": 9.515, "g_diffuse": 739.340, "g_specular[0]": 55914.842, "g_specular[1]": 3249.071, "g_specular[2]": 2670.326},
    "wanted_no_level0": {"values": 40.169, "g_pos": 9.515, "g_normal": 12.640, "g_kd": 26.981, "g_ks": 32.691, "g_view": 9.515, "g_diffuse": 739.340, "g_specular[0]": 55914.842, "g_specular[1]": 3249.071, "g_specular[2]": 2670.326},
    "wanted_only_maps": {"values": 40.169, "g_pos": 9.515, "g_normal": 12.640, "g_kd": 26.981, "g_ks": 32.691, "g_view": 9.515, "g_diffuse": 739.340, "g_specular[0]": 55914.842, "g_specular[1]": 3249.071, "g_specular[2]": 2670.326},
    "wanted_only_view": {"values": 40.169, "g_pos": 9.515, "g_normal": 12.640, "g_kd": 26.981, "g_ks": 32.691, "g_view": 9.515, "g_diffuse": 739.340, "g_specular[0]": 55914.842, "g_specular[1]": 3249.071, "g_specular[2]": 2670.326},
    "conc_list_lds": {"values": 4.580, "g_pos": 0.053, "g_normal": 0.309, "g_kd": 4.949, "g_ks": 3.437, "g_view": 0.053, "g_diffuse": 1.529, "g_specular[0]": 0.360, "g_specular[1]": 0.760, "g_specular[2]": 0.000},
    "conc_list_merge": {"values": 5.298, "g_pos": 0.179, "g_normal": 0.939, "g_kd": 4.533, "g_ks": 3.243, "g_view": 0.179, "g_diffuse": 1.593, "g_specular[0]": 4.494, "g_specular[1]": 0.675, "g_specular[2]": 0.000},
    "conc_frame_lds": {"values": 3.742, "g_pos": 0.043, "g_normal": 0.198, "g_kd": 3.969, "g_ks": 3.440, "g_view": 0.043, "g_diffuse": 0.756, "g_specular[0]": 1.292, "g_specular[1]": 0.519, "g_specular[2]": 0.000},
    "conc_frame_merge": {"values": 5.235, "g_pos": 0.190, "g_normal": 1.132, "g_kd": 4.841, "g_ks": 3.670, "g_view": 0.190, "g_diffuse": 2.066, "g_specular[0]": 10.115, "g_specular[1]": 1.780, "g_specular[2]": 0.000},
    "conc_two_quads": {"values": 41.360, "g_pos": 5.109, "g_normal": 9.005, "g_kd": 39.396, "g_ks": 21.647, "g_view": 5.109, "g_diffuse": 11.816, "g_specular[0]": 74.739, "g_specular[1]": 11.785, "g_specular[2]": 0.000},
    "conc_quad_per_wave": {"values": 78.706, "g_pos": 14.883, "g_normal": 25.591, "g_kd": 117.422, "g_ks": 41.194, "g_view": 14.883, "g_diffuse": 184.030, "g_specular[0]": 217.779, "g_specular[1]": 126.457, "g_specular[2]": 0.000},
    "geo_S1": {"values": 3.578, "g_pos": 0.950, "g_normal": 1.126, "g_kd": 3.562, "g_ks": 2.566, "g_view": 0.950, "g_diffuse": 1.898, "g_specular[0]": 68.518, "g_specular[1]": 3.921, "g_specular[2]": 3.052},
    "geo_S2": {"values": 5.131, "g_pos": 0.772, "g_normal": 1.079, "g_kd": 4.024, "g_ks": 2.809, "g_view": 0.772, "g_diffuse": 3.436, "g_specular[0]": 380.052, "g_specular[1]": 34.838, "g_specular[2]": 3.985},
    "geo_S16": {"values": 27.171, "g_pos": 4.728, "g_normal": 5.116, "g_kd": 23.190, "g_ks": 21.057, "g_view": 4.728, "g_diffuse": 548.123, "g_specular[0]": 7049.568, "g_specular[1]": 614.131, "g_specular[2]": 278.253},
    "geo_S32": {"values": 29.032, "g_pos": 4.728, "g_normal": 7.071, "g_kd": 30.400, "g_ks": 22.668, "g_view": 4.728, "g_diffuse": 795.535, "g_specular[0]": 7049.568, "g_specular[1]": 614.131, "g_specular[2]": 278.253},
    "kink_roughness": {"values": 80.312, "g_pos": 4.146, "g_normal": 11.526, "g_kd": 17.740, "g_ks": 32.133, "g_view": 4.146, "g_diffuse": 122.202, "g_specular[0]": 2185.489, "g_specular[1]": 363.428, "g_specular[2]": 304.151, "g_specular[3]": 609.206, "g_specular[4]": 141.836},
    "kink_roughness_one_ulp_beside": {"values": 50.804, "g_pos": 6.696, "g_normal": 12.517, "g_kd": 43.150, "g_ks": 39326.458, "g_view": 6.696, "g_diffuse": 122.202, "g_specular[0]": 2187.050, "g_specular[1]": 363.428, "g_specular[2]": 20803863.181, "g_specular[3]": 16777216.000, "g_specular[4]": 16777216.000},
    "kink_n_dot_v": {"values": 27.171, "g_pos": 8.678, "g_normal": 14.806, "g_kd": 26.432, "g_ks": 21.057, "g_view": 8.678, "g_diffuse": 561.529, "g_specular[0]": 7049.568, "g_specular[1]": 614.131, "g_specular[2]": 278.253},
    "degenerate_vectors": {"values": 107.993, "g_pos": 17.040, "g_normal": 22.353, "g_kd": 65.971, "g_ks": 74.333, "g_view": 17.040, "g_diffuse": 587.446, "g_specular[0]": 7049.568, "g_specular[1]": 1013.689, "g_specular[2]": 278.253},
    "xfm_zero": {"values": 0.000, "g_pos": 0.000, "g_normal": 0.000, "g_kd": 0.000, "g_ks": 0.000, "g_view": 0.000, "g_diffuse": 0.000, "g_specular[0]": 0.000, "g_specular[1]": 0.000, "g_specular[2]": 0.000},
    "xfm_reflection": {"values": 99.949, "g_pos": 7.783, "g_normal": 13.007, "g_kd": 34.100, "g_ks": 16.688, "g_view": 7.783, "g_diffuse": 2302.742, "g_specular[0]": 1791.051, "g_specular[1]": 1654.762, "g_specular[2]": 2469.488},
    "xfm_shear": {"values": 57.084, "g_pos": 3.537, "g_normal": 6.377, "g_kd": 54.863, "g_ks": 22.992, "g_view": 3.537, "g_diffuse": 462.899, "g_specular[0]": 3916.740, "g_specular[1]": 2046.374, "g_specular[2]": 403.775},
    "xfm_scale_1e-20": {"values": 30.579, "g_pos": 5.177, "g_normal": 7.346, "g_kd": 32.796, "g_ks": 21.057, "g_view": 5.177, "g_diffuse": 587.446, "g_specular[0]": 7049.568, "g_specular[1]": 1484.721, "g_specular[2]": 970.049},
    "xfm_scale_1e20": {"values": 30.214, "g_pos": 7.767, "g_normal": 11.040, "g_kd": 26.432, "g_ks": 21.377, "g_view": 7.767, "g_diffuse": 368.134, "g_specular[0]": 7049.568, "g_specular[1]": 1442.186, "g_specular[2]": 970.049},
    "xfm_three": {"values": 73.690, "g_pos": 9.783, "g_normal": 10.348, "g_kd": 62.606, "g_ks": 46.480, "g_view": 9.783, "g_diffuse": 816.896, "g_specular[0]": 12484.633, "g_specular[1]": 6930.028, "g_specular[2]": 476.237},
    "frame_1x8x8": {"values": 175.608, "g_pos": 5.431, "g_normal": 10.857, "g_kd": 30.513, "g_ks": 17.058, "g_view": 0.090, "g_diffuse": 2629.363, "g_specular[0]": 758.168, "g_specular[1]": 1343.384, "g_specular[2]": 1524.227},
    "frame_1x8x9": {"values": 118.473, "g_pos": 9.827, "g_normal": 10.588, "g_kd": 117.468, "g_ks": 53.233, "g_view": 0.619, "g_diffuse": 732.226, "g_specular[0]": 1813.033, "g_specular[1]": 2981.907, "g_specular[2]": 668.072},
    "frame_1x7x64": {"values": 250.229, "g_pos": 12.072, "g_normal": 21.660, "g_kd": 241.202, "g_ks": 85.049, "g_view": 0.168, "g_diffuse": 11581.404, "g_specular[0]": 201313.677, "g_specular[1]": 16784.051, "g_specular[2]": 7427.868},
    "frame_3x16x8": {"values": 127.259, "g_pos": 6.393, "g_normal": 9.759, "g_kd": 74.707, "g_ks": 51.878, "g_view": 0.307, "g_diffuse": 8909.964, "g_specular[0]": 18751.004, "g_specular[1]": 16746.301, "g_specular[2]": 1402.644},
    "frame_list255": {"values": 117.840, "g_pos": 15.210, "g_normal": 19.215, "g_kd": 94.897, "g_ks": 57.150, "g_view": 0.319, "g_diffuse": 2043.657, "g_specular[0]": 4911.699, "g_specular[1]": 19047.958, "g_specular[2]": 1342.563},
    "frame_list256": {"values": 73.619, "g_pos": 7.666, "g_normal": 13.048, "g_kd": 67.861, "g_ks": 63.960, "g_view": 0.160, "g_diffuse": 4836.028, "g_specular[0]": 15660.667, "g_specular[1]": 17244.580, "g_specular[2]": 7065.258},
    "mag_hdr_maps": {"values": 1018.606, "g_pos": 147.256, "g_normal": 358.532, "g_kd": 1019.003, "g_ks": 853.541, "g_view": 147.256, "g_diffuse": 42685.298, "g_specular[0]": 6243.897, "g_specular[1]": 4615.292, "g_specular[2]": 675.012},
    "mag_g_out_1e20": {"values": 103.338, "g_pos": 9.423, "g_normal": 19.775, "g_kd": 33.421, "g_ks": 42.913, "g_view": 9.423, "g_diffuse": 42685.956, "g_specular[0]": 6244.160, "g_specular[1]": 4615.864, "g_specular[2]": 674.237},
    "mag_far_positions": {"values": 93.843, "g_pos": 18.244, "g_normal": 22.746, "g_kd": 93.833, "g_ks": 56.176, "g_view": 18.244, "g_diffuse": 42685.298, "g_specular[0]": 8695.261, "g_specular[1]": 30055.481, "g_specular[2]": 1901.277},
    "operands_broadcast": {"values": 61.046, "g_pos": 11.267, "g_normal": 11.087, "g_kd": 0.731, "g_ks": 0.884, "g_view": 0.126, "g_diffuse": 898.752, "g_specular[0]": 11209.769, "g_specular[1]": 32724.678, "g_specular[2]": 724.433},
    "operands_pos_BH13": {"values": 70.933, "g_pos": 2.217, "g_normal": 14.532, "g_kd": 55.459, "g_ks": 33.199, "g_view": 0.369, "g_diffuse": 898.276, "g_specular[0]": 7886.777, "g_specular[1]": 136441.959, "g_specular[2]": 2796.574},
    "nonfinite_nan_normal": {"values": 27.171, "g_pos": 4.728, "g_normal": 7.346, "g_kd": 26.432, "g_ks": 21.377, "g_view": 4.728, "g_diffuse": 587.446, "g_specular[0]": 7049.568, "g_specular[1]": 614.131, "g_specular[2]": 970.049},
    "nonfinite_inf_pos": {"values": 27.171, "g_pos": 4.728, "g_normal": 7.346, "g_kd": 26.432, "g_ks": 21.377, "g_view": 4.728, "g_diffuse": 587.446, "g_specular[0]": 7049.568, "g_specular[1]": 614.131, "g_specular[2]": 970.049},
    "nonfinite_nan_kd": {"values": 27.171, "g_pos": 4.728, "g_normal": 7.346, "g_kd": 26.432, "g_ks": 21.377, "g_view": 4.728, "g_diffuse": 587.446, "g_specular[0]": 7049.568, "g_specular[1]": 614.131, "g_specular[2]": 970.049},
    "nonfinite_nan_g_out": {"values": 27.171, "g_pos": 4.728, "g_normal": 7.346, "g_kd": 26.432, "g_ks": 21.377, "g_view": 4.728, "g_diffuse": 587.446, "g_specular[0]": 7049.568, "g_specular[1]": 614.131, "g_specular[2]": 970.049},
    "hidden_under_the_largest": {"values": 102.090, "g_pos": 13.893, "g_normal": 15.995, "g_kd": 98.953, "g_ks": 49.139, "g_view": 13.893, "g_diffuse": 4067.969, "g_specular[0]": 84488.006, "g_specular[1]": 3272.906, "g_specular[2]": 2688.811},
}
