"""Float64 restatement of the image-space derivative operators (ops.rasterize_db, ops.interpolate_da), written from their definition:

    f = pixel centre in NDC,  q_i = p_i.xy - f p_i.w,  a_i = q_j x q_k,  s = a_0 + a_1 + a_2,  u = a_0 / s,  v = a_1 / s
    du/dX = (d a_0/d fx * s - a_0 * d s/d fx) / s^2 * 2 / W          (likewise du/dY, dv/dX, dv/dY; 2 / H for Y)
    dA/dX = du/dX (A_0 - A_2) + dv/dX (A_1 - A_2)

Plain torch in float64, so autograd gives every gradient.  Beside each value the module evaluates its MAGNITUDE: the same expression
with every input replaced by its absolute value and every subtraction by an addition (the denominators keep their true value).  An
fp32 evaluation in any order errs by a few 2^-24 of that magnitude per operation, so errors are measured in units of 2^-24 x magnitude:
the unit in which the torch fp32 path was measured and in which the kernels' bounds are stated (tests/test_deriv_gpu.py).  The
magnitude of a gradient is the gradient of the magnitude expression (all its terms are positive), summed per vertex for the scatters.

Scenes (``scene``) are soups of well-conditioned triangles: |cross| of the NDC edges >= ``min_cross`` and w in [0.6, 1.6], because the
derivatives scale as 1 / s and an edge-on triangle has unbounded fp32 error in any implementation.
"""
import numpy as np
import torch

EPS = 2.0 ** -24


def centres(n):
    """Pixel centres in NDC, float64: (i + 0.5) * 2 / n - 1."""
    return (torch.arange(n, dtype=torch.float64) + 0.5) * (2.0 / n) - 1.0


def _live(rast, F):
    ids = rast[..., 3].long() - 1
    return ids, (ids >= 0) & (ids < F)


def _no_term(t):
    """A float64 zero that depends on ``t`` (an image nothing covers still has a gradient: zeros) and hands back an exact zero for any
    upstream gradient -- 0.0 * t.sum() would turn a non-finite upstream value at a pixel without a triangle into NaN for every input."""
    return t.double().reshape(-1)[:0].sum()


def _rows(ids, live, tri, Bv, V):
    """Vertex rows [n,3] (image base included when the vertex array is per image) and the (b, y, x) of the live pixels."""
    b, y, x = torch.nonzero(live, as_tuple=True)
    t = tri.long()[ids[b, y, x]]
    return t + (b * V)[:, None] * int(Bv > 1), (b, y, x)


def _db_of(P, fx, fy, W, H, mag=False, s_true=None):
    """P [n,3,4] (x, y, z, w per corner), fx, fy [n] -> (du/dX, du/dY, dv/dX, dv/dY) [n,4] and s.  ``mag``: the magnitude expression
    (P, fx, fy already absolute; ``s_true`` the true |s|, its derivative replaced by that of the absolute sum)."""
    sub = (lambda p, q: p + q) if mag else (lambda p, q: p - q)
    x, y, w = P[..., 0], P[..., 1], P[..., 3]
    qx, qy = sub(x, fx[:, None] * w), sub(y, fy[:, None] * w)
    a, dax, day = [], [], []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        a.append(sub(qx[:, j] * qy[:, k], qy[:, j] * qx[:, k]))
        dax.append(sub(qy[:, j] * w[:, k], w[:, j] * qy[:, k]))
        day.append(sub(w[:, j] * qx[:, k], qx[:, j] * w[:, k]))
    s = a[0] + a[1] + a[2]
    sx, sy = dax[0] + dax[1] + dax[2], day[0] + day[1] + day[2]
    den = s if not mag else s_true.detach() - (s - s.detach())  # value |s|; d den = -d(abs sum): 1 / den^2 grows with every input
    d = lambda ai, dai, ds, k: sub(dai * s, ai * ds) / (den * den) * k
    return torch.stack([d(a[0], dax[0], sx, 2.0 / W), d(a[0], day[0], sy, 2.0 / H), d(a[1], dax[1], sx, 2.0 / W), d(a[1], day[1], sy, 2.0 / H)], -1), s


def barycentrics(P, fx, fy):
    """(u, v) of the perspective-correct barycentrics at NDC position (fx, fy): P [3,4] float64."""
    q = P[:, :2] - torch.stack([fx, fy]) * P[:, 3:4]
    cr = lambda p, r: p[0] * r[1] - p[1] * r[0]
    a0, a1, a2 = cr(q[1], q[2]), cr(q[2], q[0]), cr(q[0], q[1])
    s = a0 + a1 + a2
    return a0 / s, a1 / s


def barycentric_map(clip, tri, rast):
    """(u, v) [B,H,W,2] float64 of the stored triangles at the pixel centres, differentiable w.r.t. ``clip``; 0 where empty."""
    clip = clip if clip.dim() == 3 else clip[None]
    B, H, W, _ = rast.shape
    ids, live = _live(rast, tri.shape[0])
    rows, (b, y, x) = _rows(ids, live, tri, clip.shape[0], clip.shape[1])
    P = clip.double().reshape(-1, 4)[rows]
    fx, fy = centres(W)[x], centres(H)[y]
    qx, qy = P[..., 0] - fx[:, None] * P[..., 3], P[..., 1] - fy[:, None] * P[..., 3]
    a = [qx[:, (i + 1) % 3] * qy[:, (i + 2) % 3] - qy[:, (i + 1) % 3] * qx[:, (i + 2) % 3] for i in range(3)]
    s = a[0] + a[1] + a[2]
    return torch.zeros(B, H, W, 2, dtype=torch.float64).index_put((b, y, x), torch.stack([a[0] / s, a[1] / s], -1))


def interpolate(attr, rast, tri, uv):
    """u A0 + v A1 + (1 - u - v) A2 with the barycentrics ``uv`` [B,H,W,2] (float64, differentiable), 0 where empty."""
    attr = attr if attr.dim() == 3 else attr[None]
    B, H, W, _ = rast.shape
    ids, live = _live(rast, tri.shape[0])
    rows, (b, y, x) = _rows(ids, live, tri, attr.shape[0], attr.shape[1])
    A = attr.double().reshape(-1, attr.shape[2])[rows]
    u, v = uv[b, y, x, 0:1], uv[b, y, x, 1:2]
    return torch.zeros(B, H, W, attr.shape[2], dtype=torch.float64).index_put((b, y, x), u * A[:, 0] + v * A[:, 1] + (1 - u - v) * A[:, 2])


def rasterize_db(clip, tri, rast):
    """-> rast_db [B,H,W,4] float64, differentiable w.r.t. ``clip`` ([B|1,V,4] or [V,4], any float dtype)."""
    return rasterize_db_full(clip, tri, rast)["db"]


def rasterize_db_full(clip, tri, rast, g=None):
    """dict(db, mag [B,H,W,4]) and, with an upstream gradient ``g`` [B,H,W,4]: g_clip, g_clip_mag [Bc,V,4] (the float64 gradient and
    the summed magnitude of its terms), contrib [n,3,4] (per live pixel and corner), rows [n,3], feeds [Bc*V] (pixels per vertex row)."""
    clip = clip if clip.dim() == 3 else clip[None]
    B, H, W, _ = rast.shape
    Bc, V, F = clip.shape[0], clip.shape[1], tri.shape[0]
    ids, live = _live(rast, F)
    db = torch.zeros(B, H, W, 4, dtype=torch.float64)
    mag = torch.zeros(B, H, W, 4, dtype=torch.float64)
    out = dict(db=db, mag=mag)
    if F == 0 or not bool(live.any()):
        if g is not None:
            out.update(g_clip=torch.zeros(Bc, V, 4, dtype=torch.float64), g_clip_mag=torch.zeros(Bc, V, 4, dtype=torch.float64),
                       feeds=torch.zeros(Bc * V, dtype=torch.int64))
        out["db"] = db + _no_term(clip)
        return out
    rows, (b, y, x) = _rows(ids, live, tri, Bc, V)
    flat = clip.double().reshape(Bc * V, 4)
    P = flat[rows]
    fx, fy = centres(W)[x], centres(H)[y]
    val, s = _db_of(P, fx, fy, W, H)
    out["db"] = db.index_put((b, y, x), val)
    Pa = P.detach().abs().requires_grad_(g is not None)
    mval, _ = _db_of(Pa, fx.abs(), fy.abs(), W, H, mag=True, s_true=s.detach().abs())
    out["mag"] = mag.index_put((b, y, x), mval.detach())
    if g is not None:
        gl = g.double()[b, y, x]
        Pl = P.detach().requires_grad_(True)
        v2, _ = _db_of(Pl, fx, fy, W, H)
        (c,) = torch.autograd.grad((v2 * gl).sum(), Pl)
        (cm,) = torch.autograd.grad((mval * gl.abs()).sum(), Pa)
        c[..., 2], cm[..., 2] = 0.0, 0.0
        idx = rows.reshape(-1)
        out["g_clip"] = torch.zeros(Bc * V, 4, dtype=torch.float64).index_add_(0, idx, c.reshape(-1, 4)).reshape(Bc, V, 4)
        out["g_clip_mag"] = torch.zeros(Bc * V, 4, dtype=torch.float64).index_add_(0, idx, cm.reshape(-1, 4)).reshape(Bc, V, 4)
        out["feeds"] = torch.zeros(Bc * V, dtype=torch.int64).index_add_(0, idx, torch.ones_like(idx))
        out["contrib"], out["contrib_mag"], out["rows"] = c, cm, rows
    return out


def select(diff_attrs, C):
    return list(range(C)) if isinstance(diff_attrs, str) else [int(i) % C for i in diff_attrs]


def interpolate_da(attr, rast, tri, rast_db, diff_attrs="all"):
    """-> out_da [B,H,W,2S] float64, differentiable w.r.t. ``attr`` and ``rast_db``."""
    return interpolate_da_full(attr, rast, tri, rast_db, diff_attrs)["da"]


def interpolate_da_full(attr, rast, tri, rast_db, diff_attrs="all", g=None):
    """dict(da, mag [B,H,W,2S]) and, with an upstream gradient ``g`` [B,H,W,2S]: g_attr, g_attr_mag [Ba,V,C], g_db, g_db_mag
    [B,H,W,4], contrib [n,3,C] / contrib_mag, rows [n,3], feeds [Ba*V]."""
    attr = attr if attr.dim() == 3 else attr[None]
    B, H, W, _ = rast.shape
    Ba, V, C = attr.shape
    F = tri.shape[0]
    sel = select(diff_attrs, C)
    S = len(sel)
    ids, live = _live(rast, F)
    zeros = lambda *sh: torch.zeros(*sh, dtype=torch.float64)
    out = dict(da=zeros(B, H, W, 2 * S) + _no_term(attr) + _no_term(rast_db), mag=zeros(B, H, W, 2 * S))
    if g is not None:
        out.update(g_attr=zeros(Ba, V, C), g_attr_mag=zeros(Ba, V, C), g_db=zeros(B, H, W, 4), g_db_mag=zeros(B, H, W, 4),
                   feeds=torch.zeros(Ba * V, dtype=torch.int64))
    if F == 0 or not bool(live.any()):
        return out
    rows, (b, y, x) = _rows(ids, live, tri, Ba, V)

    def ev(A, db, mag):  # A [n,3,C], db [n,4] -> [n,2S]
        sub = (lambda p, q: p + q) if mag else (lambda p, q: p - q)
        As = A[..., sel]
        d0, d1 = sub(As[:, 0], As[:, 2]), sub(As[:, 1], As[:, 2])
        dx = db[:, 0:1] * d0 + db[:, 2:3] * d1
        dy = db[:, 1:2] * d0 + db[:, 3:4] * d1
        return torch.stack([dx, dy], -1).reshape(dx.shape[0], -1)

    A = attr.double().reshape(Ba * V, C)[rows]
    dbl = rast_db.double()[b, y, x]
    out["da"] = zeros(B, H, W, 2 * S).index_put((b, y, x), ev(A, dbl, False))
    out["mag"] = zeros(B, H, W, 2 * S).index_put((b, y, x), ev(A.detach().abs(), dbl.detach().abs(), True))
    if g is not None:
        gl = g.double()[b, y, x]
        Al, dl = A.detach().requires_grad_(True), dbl.detach().requires_grad_(True)
        c, gd = torch.autograd.grad((ev(Al, dl, False) * gl).sum(), [Al, dl])
        Am, dm = A.detach().abs().requires_grad_(True), dbl.detach().abs().requires_grad_(True)
        cm, gdm = torch.autograd.grad((ev(Am, dm, True) * gl.abs()).sum(), [Am, dm])
        idx = rows.reshape(-1)
        out["g_attr"] = zeros(Ba * V, C).index_add_(0, idx, c.reshape(-1, C)).reshape(Ba, V, C)
        out["g_attr_mag"] = zeros(Ba * V, C).index_add_(0, idx, cm.reshape(-1, C)).reshape(Ba, V, C)
        out["g_db"] = zeros(B, H, W, 4).index_put((b, y, x), gd)
        out["g_db_mag"] = zeros(B, H, W, 4).index_put((b, y, x), gdm)
        out["feeds"] = torch.zeros(Ba * V, dtype=torch.int64).index_add_(0, idx, torch.ones_like(idx))
        out["contrib"], out["contrib_mag"], out["rows"] = c, cm, rows
    return out


def units(got, ref, mag):
    """max |got - ref| / (2^-24 magnitude) over the elements with a magnitude; elements without one must be exactly zero."""
    got, dead = got.double(), mag == 0
    assert bool((got[dead] == 0).all()), "an element nothing feeds is not zero"
    if bool(dead.all()):
        return 0.0
    return float(((got - ref).abs()[~dead] / (EPS * mag[~dead])).max())


def violations(got, ref, mag, parent_units, factor=4.0, floor_ulp=4.0):
    """Elements where |got - ref| > 2^-24 (factor * parent_units * magnitude + floor_ulp * |ref|): the kernels' bound (factor 4 over the
    measured torch fp32 path, a floor of a few ulp of the float64 value).  Non-finite values violate."""
    got = got.double()
    bound = EPS * (factor * parent_units * mag + floor_ulp * ref.abs())
    return torch.nonzero(~((got - ref).abs() <= bound))


# ---------------------------------------------------------------------------------------------------------------- scenes
def soup(n, seed, min_cross=0.25, w_range=(0.6, 1.6), shared=False, B=1):
    """n well-conditioned triangles with private vertices, mixed winding, perspective w: clip [B|1, 3n, 4] float32, tri [n,3] int32.
    Triangles are resampled until |cross(p1 - p0, p2 - p0)| >= min_cross in NDC; depth separates them (z grows with the index)."""
    rng = np.random.default_rng(seed)
    Bc = 1 if shared else B
    xy = rng.uniform(-1.1, 1.1, (Bc, n, 3, 2))
    while True:
        e1, e2 = xy[:, :, 1] - xy[:, :, 0], xy[:, :, 2] - xy[:, :, 0]
        bad = np.abs(e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]) < min_cross
        if not bad.any():
            break
        xy[bad] = rng.uniform(-1.1, 1.1, (int(bad.sum()), 3, 2))
    w = rng.uniform(w_range[0], w_range[1], (Bc, n, 3, 1))
    z = (np.arange(n).reshape(1, n, 1, 1) + rng.uniform(0.1, 0.9, (Bc, n, 3, 1))) / (n + 1.0) * 1.6 - 0.8
    clip = np.concatenate([xy * w, z * w, w], -1).reshape(Bc, 3 * n, 4)
    return torch.from_numpy(clip).float(), torch.arange(3 * n, dtype=torch.int32).reshape(n, 3)


def attributes(Ba, V, C, seed):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-2.0, 2.0, (Ba, V, C))).float()


# name -> (B, H, W, triangles, shared clip, shared attr, C, diff_attrs).  B in {1, 3, 16}; non-square and odd frames, W < 8;
# C in {1, 2, 3, 8, 13, 24}; 'all', a subset, a permuted subset and a list with a repeated index.  S = 24 > 16 selected attributes is the
# size at which a3d_interp_da_bwd leaves the tile scatter for its per-pixel kernel.  (A scene's seed is its rank among the sorted names.)
SCENES = {
    "b1_square_uv": (1, 64, 64, 12, False, False, 2, "all"),
    "b3_odd_c3_subset": (3, 37, 53, 10, False, True, 3, [0, 2]),
    "b16_shared_c8_permuted": (16, 32, 48, 8, True, False, 8, [5, 1, 7, 2]),
    "b3_narrow_c13_repeat": (3, 45, 7, 6, True, True, 13, [3, 3, 12, 0, 3]),
    "b1_tall_c1": (1, 70, 5, 5, False, False, 1, "all"),
    "b3_c13_all": (3, 24, 40, 9, False, False, 13, "all"),
    "c24_all_b2": (2, 29, 35, 7, False, False, 24, "all"),
}


def scene(name):
    B, H, W, n, shared_clip, shared_attr, C, diff = SCENES[name]
    seed = sorted(SCENES).index(name)
    clip, tri = soup(n, seed, shared=shared_clip, B=B)
    attr = attributes(1 if shared_attr else B, clip.shape[1], C, seed + 100)
    return dict(B=B, H=H, W=W, clip=clip, tri=tri, attr=attr, diff_attrs=diff, seed=seed)


def range_scene():
    """Range mode: one shared vertex and attribute array, image b renders tri[first : first + count] (the last image nothing)."""
    clip, tri = soup(12, 21, shared=True)
    return dict(B=3, H=33, W=47, clip=clip, tri=tri, attr=attributes(1, clip.shape[1], 3, 22), diff_attrs=[2, 0], seed=23,
                ranges=torch.tensor([[0, 5], [3, 9], [7, 0]], dtype=torch.int32))


def empty_scene():
    """Every triangle off screen: an image nothing covers."""
    clip, tri = soup(4, 31, B=2)
    clip[..., 0] += 5.0 * clip[..., 3]
    return dict(B=2, H=19, W=23, clip=clip, tri=tri, attr=attributes(2, clip.shape[1], 3, 32), diff_attrs="all", seed=33)


def chain_scene():
    """The textured-mesh chain: a uv attribute in [0, 1] shared by three images and a 64 x 64 x 3 texture."""
    clip, tri = soup(10, 41, B=3)
    uv = torch.from_numpy(np.random.default_rng(42).uniform(0.0, 1.0, (1, clip.shape[1], 2))).float()
    tex = torch.from_numpy(np.random.default_rng(43).uniform(0.0, 1.0, (1, 64, 64, 3))).float()
    return dict(B=3, H=48, W=64, clip=clip, tri=tri, attr=uv, diff_attrs="all", seed=44, tex=tex)


def upstream(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed + 1000).normal(0.0, 1.0, tuple(shape))).float()
