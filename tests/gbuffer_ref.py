"""Float64 references, input makers and white-box list patterns for the fused G-buffer kernels (csrc/gbuffer.hip, gbuffer_common.h),
shared by tests/test_gbuffer_cpu.py and tests/test_gbuffer_adversarial_gpu.py.

The G-buffer backward has a scatter of its own (not tile_scatter.h): a work-group is 256 CONSECUTIVE entries of the covered-pixel list;
entries on one (image, triangle) merge with lane ^ 1, then lane ^ 8; every surviving (entry, corner) row is staged in LDS (640 or 768
entries), linked into the list of its vertex row in a 512- or 1024-slot table (16 linear probes from gb_hash) and flushed by 16-lane
groups; what finds no entry or no slot goes to the gradient rows with single-lane atomics.  The patterns below are therefore fabricated
by LIST POSITION and then laid out on a small frame; ``simulate`` replays the merge and the table on the CPU so that a test can assert the
stage it means to force.

Two input modes.  EXACT (``exact_tensors``): u, v multiples of 1/16 with 1 - u - v >= 1/16, every attribute an integer in [-8, 8],
upstream gradients non-zero integers in [-4, 4], face-normal gradient zero.  Every fp32 product is then exact; a term of a gradient row
is a multiple of 1/16 of magnitude <= 8 (g + g_tex), so with P <= 2^16 list entries every partial sum is below 2^19 and exact
(24 bits = 19 integer + 4 fractional + sign slack); forward values are multiples of 1/16 below 2^4; (gu, gv) are integers below 2^11.
Any summation order gives the same number: torch.equal.  NORMAL (``normal_tensors``): real positions and a random face-normal gradient;
columns 0..2 are held to ``vpos_bound``.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_scatter_backward_gpu import _tri_xy, make_pattern, rast_bwd_reference, raster_from_ids  # noqa: E402

EPS = 2.0 ** -24
WG, GB_PROBES, GB_ROW = 256, 16, 16  # csrc/gbuffer.hip
TABLES = {"small": (512, 640), "big": (1024, 768)}  # <GB_SLOTS, GB_ENTRIES>; big is chosen when P < 0.6 * B * F
SQRT_ULP, DIV_ULP = 2.0, 5.0  # sqrtf: 1 ulp, division: 2.5 ulp (HIP's documented bounds), in units of 2^-24 relative
PATTERNS = ("runs", "period8", "checker", "unique", "collide", "fan", "boundary", "holes")


def gb_hash(key, slots):
    """The slot gb_slot() starts probing at: ((key * 2654435761) mod 2^32) >> 23 (512 slots) or >> 22 (1024 slots)."""
    shift = 23 if slots == 512 else 22
    return ((np.asarray(key, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(shift)


# ------------------------------------------------------------------------------------------------ list patterns
def _image_of(P, B):
    """Image of each list entry: whole work-groups per image, non-decreasing."""
    nwg = -(-P // WG)
    return (np.arange(P) // WG) * B // max(nwg, 1)


def _pool(seed):
    """20 well-conditioned triangles over 12 shared vertices (the 'pool' of test_scatter_backward_gpu)."""
    _, tri, V, xy = make_pattern("pool", 1, 1, 1, False, seed)
    return tri, V, xy


def make_list(name, table, B, seed=0, P=None):
    """The named list pattern: dict(f [P] triangle of each list entry (-1 = a background pixel that is listed all the same, -2 = an id
    out of range, resolved by ``finish``), b [P] image, tri [F,3], V, xy [V,2] NDC positions with |cross| >= 0.3 per triangle).

    runs      runs of one triangle of length 1, 2, 3, 8, 9, 16, 17, 64, 257 (twice over, so every run starts at two alignments, and a run of 5:
              759 entries, an odd tail); neighbouring runs use different triangles of a pool with shared vertices
    period8   the same triangle at lanes L and L ^ 8 but not at L ^ 1: only the second merge round fires
    checker   two triangles sharing an edge, f = bit0(L) ^ bit3(L): no merge fires, 768 staged entries > 640 with 4 slots in use
    unique    every entry its own triangle with private vertices: 768 rows per work-group > 512 slots and 768 entries > 640
    collide   WHITE-BOX: per image 36 vertex rows (12 triangles) whose gb_hash for this table size is one value: > GB_PROBES rows on
              one probe sequence, so the probes run out with few rows.  A changed hash leaves the case a plain pool
    fan       one vertex shared by all 256 triangles of a work-group (at a rotating corner): one slot carries a list of 256 entries
    boundary  one triangle on every entry, the image changing at list position 129: lanes 128 / 129 (^ 1) and 128 / 136 (^ 8) carry
              the same f but another image and must not merge
    holes     pool with ~30 % background entries and ~5 % ids out of range, P entries (1, 255, 256, 257: partial work-groups)
    """
    rng = np.random.default_rng(seed)
    slots = TABLES[table][0]
    lane = lambda P: np.arange(P) % WG
    if name == "runs":
        tri, V, xy = _pool(seed)
        lengths = [1, 2, 3, 8, 9, 16, 17, 64, 257] * 2 + [5]
        f = np.concatenate([np.full(n, (7 * i) % len(tri)) for i, n in enumerate(lengths)])
        b = _image_of(len(f), B)
    elif name == "period8":
        P = 2 * WG
        L = lane(P)
        f = (L & 7) | ((L >> 4) << 3)
        tri = np.arange(3 * 128).reshape(-1, 3)
        V, xy, b = tri.size, _tri_xy(rng, 128).reshape(-1, 2), _image_of(P, B)
    elif name == "checker":
        P = 2 * WG
        L = lane(P)
        f = (L & 1) ^ ((L >> 3) & 1)
        tri = np.array([[0, 1, 2], [1, 3, 2]])
        V, xy, b = 4, np.array([[-0.9, -0.8], [0.85, -0.7], [-0.75, 0.9], [0.8, 0.85]]), _image_of(P, B)
    elif name == "unique":
        P = 2 * WG
        f = lane(P)
        tri = np.arange(3 * WG).reshape(-1, 3)
        V, xy, b = tri.size, _tri_xy(rng, WG).reshape(-1, 2), _image_of(P, B)
    elif name == "collide":
        P, V = 2 * WG, 60000
        b = _image_of(P, B)
        xy = rng.uniform(-1.0, 1.0, (V, 2))
        target = int(gb_hash(1, slots))
        tris = []
        for bi in range(B):
            idx = np.arange(V)
            hit = idx[gb_hash(bi * V + idx, slots) == target][:36]
            assert len(hit) == 36, "V is large enough for 36 rows on one hash value"
            xy[hit] = _tri_xy(rng, 12).reshape(-1, 2)
            tris.append(hit.reshape(12, 3))
        tri = np.concatenate(tris)
        f = 12 * b + rng.integers(0, 12, P)  # image b uses the triangles whose rows collide in image b
    elif name == "fan":
        P = 2 * WG
        f = lane(P)
        ring = np.zeros((WG, 2, 2))
        todo = np.ones(WG, bool)
        while todo.any():  # centre at the origin: |cross(p1, p2)| >= 0.3
            ring[todo] = rng.uniform(-1.0, 1.0, (int(todo.sum()), 2, 2))
            todo = np.abs(ring[:, 0, 0] * ring[:, 1, 1] - ring[:, 0, 1] * ring[:, 1, 0]) < 0.3
        k = np.arange(WG)
        tri = np.stack([np.zeros(WG, np.int64), 2 * k + 1, 2 * k + 2], -1)
        tri = np.stack([np.roll(t, i % 3) for i, t in enumerate(tri)])
        V, xy, b = 2 * WG + 1, np.concatenate([np.zeros((1, 2)), ring.reshape(-1, 2)]), _image_of(P, B)
    elif name == "boundary":
        assert B >= 2
        P = 300
        f = np.zeros(P, np.int64)
        tri, V, xy = np.array([[0, 1, 2]]), 3, np.array([[-0.95, -0.9], [0.9, -0.8], [-0.1, 0.95]])
        b = (np.arange(P) >= 129).astype(np.int64)
    elif name == "holes":
        tri, V, xy = _pool(seed)
        if table == "small":  # few entries: keep P >= 0.6 * B * F with fewer triangles
            tri = tri[: max(1, min(len(tri), int(P / (0.6 * B))))]
        f = rng.integers(0, len(tri), P)
        u = rng.random(P)
        if P > 1:
            f[u < 0.3] = -1
            f[u > 0.95] = -2
        b = _image_of(P, B)
    else:
        raise ValueError(name)
    return dict(name=name, table=table, f=np.asarray(f, np.int64), b=np.asarray(b, np.int64), tri=np.asarray(tri, np.int64), V=int(V), xy=xy)


def finish(case, B, H, W, seed=0):
    """Pad F with unreferenced triangles so that the entry point takes the table size the case names (asserted), resolve the ids out of
    range, and lay the list out on a [B,H,W] frame: entry p of image b gets a pixel of its own (random order inside the image).
    Adds F, P, pix [P] int64, ids [B,H,W] (-1 = background or not listed)."""
    rng = np.random.default_rng(seed + 1000)
    P, Fu = len(case["f"]), len(case["tri"])
    if case["table"] == "big":
        F = max(Fu, int(P / (0.6 * B)) + 1)
        assert P < 0.6 * B * F, "the 1024-slot instance: P < 0.6 * B * F"
    else:
        F = Fu
        assert P >= 0.6 * B * F, "the 512-slot instance: P >= 0.6 * B * F"
    tri = np.concatenate([case["tri"], np.tile(np.array([[0, 1, 2]]), (F - Fu, 1))]) if F > Fu else case["tri"]
    f = case["f"].copy()
    oob = f == -2
    f[oob] = F + rng.integers(0, 4, int(oob.sum()))
    hw = H * W
    pix = np.zeros(P, np.int64)
    ids = np.full((B, hw), -1, np.int64)
    for bi in range(B):
        sel = np.nonzero(case["b"] == bi)[0]
        assert len(sel) <= hw, "the frame holds the image's share of the list"
        where = rng.permutation(hw)[: len(sel)]
        pix[sel] = bi * hw + where
        ids[bi, where] = f[sel]
    case.update(F=F, P=P, B=B, H=H, W=W, tri=tri, f=f, pix=pix, ids=ids.reshape(B, H, W))
    return case


def simulate(case):
    """What gb_bwd_kernel does with each work-group of the list, replayed on the CPU: per work-group dict(merge1, merge8 = entries
    absorbed in either round, entries = 3 x surviving entries, rows = distinct vertex rows, longest = most staged entries on one row,
    worst_hash = most distinct rows on one gb_hash value of the case's table)."""
    slots = TABLES[case["table"]][0]
    f, b, F, V, tri = case["f"], case["b"], case["F"], case["V"], case["tri"]
    out = []
    for w0 in range(0, len(f), WG):
        fw, bw = f[w0:w0 + WG], b[w0:w0 + WG]
        n = len(fw)
        live = np.zeros(WG, bool)
        live[:n] = (fw >= 0) & (fw < F)
        key = -1 - np.arange(WG)
        key[:n] = np.where(live[:n], bw * F + fw, key[:n])
        L = np.arange(WG)
        same = live & (key[L ^ 1] == key)
        active = live & ~(same & ((L & 1) == 1))
        key2 = np.where(active, key, -1 - L)
        same8 = active & (key2[L ^ 8] == key2)
        active2 = active & ~(same8 & ((L & 8) != 0))
        a = np.nonzero(active2[:n])[0]
        rows = (tri[fw[a]] + (bw[a] * V)[:, None]).reshape(-1)
        uniq, counts = np.unique(rows, return_counts=True)
        _, per_hash = np.unique(gb_hash(uniq, slots), return_counts=True) if len(uniq) else (None, np.array([0]))
        out.append(dict(merge1=int((same & ((L & 1) == 1)).sum()), merge8=int((same8 & ((L & 8) != 0)).sum()), entries=3 * len(a),
                        rows=len(uniq), longest=int(counts.max()) if len(uniq) else 0, worst_hash=int(per_hash.max())))
    return out


def assert_forced(case):
    """The stage of gb_bwd_kernel the case's pattern is there to force, asserted on ``simulate``'s replay, and the side of
    P < 0.6 * B * F that selects the table size the case names."""
    name, table = case["name"], case["table"]
    slots, entries = TABLES[table]
    assert (case["P"] < 0.6 * case["B"] * case["F"]) == (table == "big")
    sim = simulate(case)
    full = [s for s, w0 in zip(sim, range(0, case["P"], WG)) if w0 + WG <= case["P"]]
    if name == "runs":
        assert sum(s["merge1"] for s in sim) > 100 and sum(s["merge8"] for s in sim) > 50
        assert case["P"] % 2 == 1 and case["P"] % WG != 0
    elif name == "period8":
        assert all(s["merge1"] == 0 and s["merge8"] == 128 for s in sim), "only the second merge round fires"
    elif name == "checker":
        assert all(s["merge1"] == 0 and s["merge8"] == 0 and s["entries"] == 768 and s["rows"] == 4 for s in sim)
        assert (768 > entries) == (table == "small"), "the entry overflow on its own (640-entry instance): 4 slots in use"
    elif name == "unique":
        assert all(s["rows"] == 768 and s["entries"] == 768 for s in sim)
        assert (768 > slots and 768 > entries) == (table == "small"), "more rows than slots and more entries than the stage holds"
    elif name == "collide":
        f, b = case["f"], case["b"]
        for bi in np.unique(b):
            r = np.unique(case["tri"][f[b == bi]] + bi * case["V"])
            assert len(r) >= 33 and len(np.unique(gb_hash(r, slots))) == 1, "one hash value for every row of the image"
        assert all(s["worst_hash"] >= 33 > GB_PROBES for s in full), "more rows on one probe sequence than probes"
    elif name == "fan":
        assert all(s["longest"] >= 256 and s["merge1"] == 0 and s["merge8"] == 0 for s in sim), "one slot, a list of 256 entries"
    elif name == "boundary":
        f, b = case["f"], case["b"]
        assert f[128] == f[129] == f[136] and b[128] != b[129] and b[128] != b[136] and (128 ^ 1, 128 ^ 8) == (129, 136)
        assert sim[0]["merge1"] == 127 and sim[0]["merge8"] > 0, "every ^ 1 pair of the work-group merges but 128 / 129"
    elif name == "holes":
        f = case["f"]
        if case["P"] > 1:
            assert (f < 0).any() and (f >= case["F"]).any() and ((f >= 0) & (f < case["F"])).sum() > case["P"] // 2
    else:
        raise ValueError(name)


# ------------------------------------------------------------------------------------------------ inputs
def _ints(rng, shape, lo=-8, hi=8):
    return torch.from_numpy(rng.integers(lo, hi + 1, shape)).float()


def _nonzero_ints(rng, shape):
    return torch.from_numpy(rng.integers(1, 5, shape) * rng.choice([-1, 1], shape)).float()


def exact_tensors(case, E=0, prior_batch=None, with_tex=True, seed=0):
    """The exact mode's inputs (module docstring).  Frame-size condition: P <= B*H*W <= 2^16."""
    B, V, P = case["B"], case["V"], case["P"]
    assert B * case["H"] * case["W"] <= 2 ** 16, "the exactness bound: B*H*W <= 2^16"
    rng = np.random.default_rng(seed + 2000)
    Bp = B if prior_batch is None else prior_batch
    t = dict(v_pos=_ints(rng, (B, V, 3)), v_nrm=_ints(rng, (B, V, 3)), prior=_ints(rng, (Bp, V, 3)),
             extra=_ints(rng, (B, V, E)) if E else None, g_out=_nonzero_ints(rng, (P, 12)),
             g_extra=_nonzero_ints(rng, (P, E)) if E else None, g_tex=_nonzero_ints(rng, (P, 3)) if with_tex else None,
             rast=raster_from_ids(case["ids"], rng))
    t["g_out"][:, 3:6] = 0.0
    return t


def normal_tensors(case, seed=0, tiny=()):
    """The normal mode's inputs: real vertex attributes, random upstream gradients (the face normal's included), no extra attribute.
    ``tiny``: (triangle, scale) pairs -- that triangle's vertices (which must be private) become a right-angled triangle of leg
    ``scale`` at the origin, so that d = |cross|^2 = scale^4 sits where the caller wants it against the 1e-20 clamp."""
    B, V, P = case["B"], case["V"], case["P"]
    rng = np.random.default_rng(seed + 3000)
    nrm = lambda *s: torch.from_numpy(rng.normal(0.0, 1.0, s)).float()
    t = dict(v_pos=nrm(B, V, 3), v_nrm=nrm(B, V, 3), prior=nrm(B, V, 3), extra=None, g_out=nrm(P, 12), g_extra=None, g_tex=nrm(P, 3),
             rast=raster_from_ids(case["ids"], rng))
    for tr, s in tiny:
        i0, i1, i2 = case["tri"][tr]
        jit = lambda: torch.from_numpy(rng.uniform(-0.05, 0.05, (B, 3))).float() * s
        t["v_pos"][:, i0] = jit()
        t["v_pos"][:, i1] = torch.tensor([s, 0.0, 0.0]) + jit()
        t["v_pos"][:, i2] = torch.tensor([0.0, s, 0.0]) + jit()
    return t


# ------------------------------------------------------------------------------------------------ references
def gather(case, rast):
    """Per list entry: live [P] bool, and for the live ones the entry index [n], vertex rows b*V + tri[f] [n,3], barycentrics
    (u, v, 1 - u - v) in float64 [n,3] and the image [n]."""
    f, b = torch.from_numpy(case["f"]), torch.from_numpy(case["b"])
    live = (f >= 0) & (f < case["F"])
    idx = live.nonzero().reshape(-1)
    r = rast.double().reshape(-1, 4)[torch.from_numpy(case["pix"])][idx]
    assert torch.equal(r[:, 3].long() - 1, f[idx]), "the texel of a live entry carries its triangle"
    rows = torch.from_numpy(case["tri"])[f[idx]] + (b[idx] * case["V"])[:, None]
    bary = torch.stack([r[:, 0], r[:, 1], 1.0 - r[:, 0] - r[:, 1]], -1)
    return live, idx, rows, bary, b[idx]


def face_normal(p):
    """cross(p1 - p0, p2 - p0) / sqrt(clamp(dot, 1e-20)) of corner positions [n,3,3] (safe_normalize of the reference)."""
    n = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=-1)
    return n / torch.sqrt(torch.clamp((n * n).sum(-1, keepdim=True), min=1e-20))


def _prior_rows(case, t, rows, img):
    return rows - (img * case["V"])[:, None] if t["prior"].shape[0] == 1 else rows


def forward_reference(case, t):
    """Float64 G-buffer rows: (out [P,12], extra_out [P,E] | None, live [P]); entries that are not live are zero rows."""
    P = case["P"]
    live, idx, rows, bary, img = gather(case, t["rast"])
    mix = lambda attr, r: (bary[..., None] * attr.double().reshape(-1, attr.shape[-1])[r]).sum(1)
    out = torch.zeros(P, 12, dtype=torch.float64)
    out[idx, 0:3] = mix(t["v_pos"], rows)
    out[idx, 3:6] = face_normal(t["v_pos"].double().reshape(-1, 3)[rows])
    out[idx, 6:9] = mix(t["v_nrm"], rows)
    out[idx, 9:12] = mix(t["prior"], _prior_rows(case, t, rows, img))
    ex = None
    if t["extra"] is not None:
        ex = torch.zeros(P, t["extra"].shape[-1], dtype=torch.float64)
        ex[idx] = mix(t["extra"], rows)
    return out, ex, live


def backward_reference(case, t, want_prior=True, use_tex=True):
    """Float64 gradient rows [B*V,16] of a3d_gbuffer_bwd WITHOUT the clip columns (12..15 left zero), the float64 (gu, gv) image
    [B,H,W,4] that feeds rast_bwd_reference, and the per-(entry, corner) terms of columns 0..2 [n,3,3] with their rows [n,3]."""
    B, V = case["B"], case["V"]
    live, idx, rows, bary, img = gather(case, t["rast"])
    g = t["g_out"].double()[idx]
    gc = g[:, 9:12] + (t["g_tex"].double()[idx] if (use_tex and t["g_tex"] is not None) else 0.0)
    flat = rows.reshape(-1)
    ref = torch.zeros(B * V, GB_ROW, dtype=torch.float64)
    add = lambda c0, terms: ref[:, c0:c0 + terms.shape[-1]].index_add_(0, flat, terms.reshape(-1, terms.shape[-1]))
    pos = t["v_pos"].double().reshape(-1, 3)[rows].clone().requires_grad_(True)
    (g_fn,) = torch.autograd.grad((face_normal(pos) * g[:, 3:6]).sum(), pos)
    pos = pos.detach()
    terms_pos = bary[..., None] * g[:, None, 0:3] + g_fn
    add(0, terms_pos)
    add(3, bary[..., None] * g[:, None, 6:9])
    if want_prior:
        add(6, bary[..., None] * gc[:, None, :])
    nrm = t["v_nrm"].double().reshape(-1, 3)[rows]
    pri = t["prior"].double().reshape(-1, 3)[_prior_rows(case, t, rows, img)]
    pairs = [(g[:, 0:3], pos), (g[:, 6:9], nrm), (gc, pri)]
    if t["extra"] is not None:
        E = t["extra"].shape[-1]
        ge = t["g_extra"].double()[idx]
        add(9, bary[..., None] * ge[:, None, :])
        pairs.append((ge, t["extra"].double().reshape(-1, E)[rows]))
    gu = sum((gg * (A[:, 0] - A[:, 2])).sum(-1) for gg, A in pairs)
    gv = sum((gg * (A[:, 1] - A[:, 2])).sum(-1) for gg, A in pairs)
    g_rast = torch.zeros(B * case["H"] * case["W"], 4, dtype=torch.float64)
    p = torch.from_numpy(case["pix"])[idx]
    g_rast[p, 0], g_rast[p, 1] = gu, gv
    return ref, g_rast.reshape(B, case["H"], case["W"], 4), terms_pos, rows


def clip_reference(case, clip, g_rast):
    """Columns 12..15 through rast_bwd_reference on the listed live pixels: (reference [B*V,4], bound [B*V,4], feeds [B*V])."""
    ref, bound, feeds, _, _, _ = rast_bwd_reference(case["ids"], case["tri"], case["V"], True, clip, g_rast)
    return ref, bound, feeds


# ------------------------------------------------------------------------------------------------ columns 0..2 in normal mode: the bound
class Err:
    """A float64 value with a first-order bound on the absolute error of its fp32 evaluation, in units of 2^-24: every + - * adds one
    rounding of its result (|v|) to the propagated errors of its operands (a fused multiply-add rounds less, never more)."""

    def __init__(self, v, e=None):
        self.v, self.e = v, torch.zeros_like(v) if e is None else e

    def __add__(self, o):
        v = self.v + o.v
        return Err(v, self.e + o.e + v.abs())

    def __sub__(self, o):
        v = self.v - o.v
        return Err(v, self.e + o.e + v.abs())

    def __mul__(self, o):
        v = self.v * o.v
        return Err(v, self.v.abs() * o.e + o.v.abs() * self.e + v.abs())


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def vpos_terms(pos, bary, g_pos, g_fn):
    """gb_load_tri + gb_pixel_adjoint's contribution to columns 0..2, operation by operation, as Err values: [corner][component].

    Rounding count per element, from the kernel's code: e1, e2 one subtraction each; the cross product 2 products + 1 subtraction per
    component; d = n.n 3 products + 2 additions; 1 / sqrtf(d) a square root (2 units = 1 ulp) and a division (5 units = 2.5 ulp);
    fn = n * inv_len 1; dot = fn.h 3 + 2; q = (h - fn * dot) * inv_len 3; g1 = e2 x q and g2 = q x e1 3 each; w = 1 - u - v 2; the
    corner's term u * g 1 product, g1 + g2 1, and the final subtraction / addition 1.  Degenerate branch (d <= 1e-20): q = h * 1e10,
    one product.  pos [n,3,3], bary [n,3], g_pos, g_fn [n,3] in float64."""
    E = lambda x: Err(x)
    P = [[E(pos[:, k, c]) for c in range(3)] for k in range(3)]
    e1 = [P[1][c] - P[0][c] for c in range(3)]
    e2 = [P[2][c] - P[0][c] for c in range(3)]
    n = _cross(e1, e2)
    d = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
    degenerate = ~(d.v > 1e-20)
    dv = torch.where(degenerate, torch.ones_like(d.v), d.v)
    r = dv ** -0.5
    inv = Err(r, 0.5 * d.e * dv ** -1.5 + (SQRT_ULP + DIV_ULP) * r)
    fn = [n[c] * inv for c in range(3)]
    h = [E(g_fn[:, c]) for c in range(3)]
    dot = fn[0] * h[0] + fn[1] * h[1] + fn[2] * h[2]
    q_reg = [(h[c] - fn[c] * dot) * inv for c in range(3)]
    big = E(torch.full_like(d.v, 1e10))
    q_deg = [h[c] * big for c in range(3)]
    q = [Err(torch.where(degenerate, q_deg[c].v, q_reg[c].v), torch.where(degenerate, q_deg[c].e, q_reg[c].e)) for c in range(3)]
    g1, g2 = _cross(e2, q), _cross(q, e1)
    u, v = E(bary[:, 0]), E(bary[:, 1])
    w = E(torch.ones_like(bary[:, 0])) - u - v
    gp = [E(g_pos[:, c]) for c in range(3)]
    return [[u * gp[c] - (g1[c] + g2[c]) for c in range(3)], [v * gp[c] + g1[c] for c in range(3)], [w * gp[c] + g2[c] for c in range(3)]]


def vpos_bound(case, t):
    """Reference and bound of columns 0..2 in normal mode: (ref [B*V,3], bound [B*V,3], feeds [B*V], terms [n,3,3] as the Err chain
    evaluates them, rows [n,3], the same terms from autograd [n,3,3]).

    bound = 2^-24 * (sum_p err_p + n * sum_p |term_p|) over the n (entry, corner) terms that feed the element: err_p is the term's own
    propagated error (vpos_terms), and the n - 1 additions that join the terms -- in a merge, a list walk or an atomic, in any order --
    each round a partial sum that is at most sum |term|."""
    ref, _, terms_ref, rows = backward_reference(case, t)
    live, idx, _, bary, _ = gather(case, t["rast"])
    g = t["g_out"].double()[idx]
    acc = vpos_terms(t["v_pos"].double().reshape(-1, 3)[rows], bary, g[:, 0:3], g[:, 3:6])
    val = torch.stack([torch.stack([a.v for a in corner], -1) for corner in acc], 1)  # [n,3,3]
    err = torch.stack([torch.stack([a.e for a in corner], -1) for corner in acc], 1)
    flat = rows.reshape(-1)
    BV = case["B"] * case["V"]
    zeros = lambda: torch.zeros(BV, 3, dtype=torch.float64)
    feeds = torch.zeros(BV, dtype=torch.float64).index_add_(0, flat, torch.ones(flat.numel(), dtype=torch.float64))
    mag = zeros().index_add_(0, flat, val.abs().reshape(-1, 3))
    bound = EPS * (zeros().index_add_(0, flat, err.reshape(-1, 3)) + feeds[:, None] * mag)
    return ref[:, 0:3], bound, feeds.long(), val, rows, terms_ref


def attr_bound(case, t, want_prior=True):
    """Bound of columns 3..8 in normal mode: a term is bary * g -- one product, after w = 1 - u - v (two roundings, |g| each at most)
    and, for the canonical columns, g + g_tex (one) -- and n terms are joined by n - 1 additions: 2^-24 * (sum (|term| + 3 |g|) +
    n * sum |term|)."""
    live, idx, rows, bary, _ = gather(case, t["rast"])
    g = t["g_out"].double()[idx]
    gc = g[:, 9:12].abs() + (t["g_tex"].double()[idx].abs() if t["g_tex"] is not None else 0.0)
    flat = rows.reshape(-1)
    BV = case["B"] * case["V"]
    feeds = torch.zeros(BV, dtype=torch.float64).index_add_(0, flat, torch.ones(flat.numel(), dtype=torch.float64))
    bound = torch.zeros(BV, 6, dtype=torch.float64)
    for c0, gg in ((0, g[:, 6:9].abs()), (3, gc)):
        if c0 == 3 and not want_prior:
            continue
        term = (bary[..., None] * gg[:, None, :]).reshape(-1, 3)
        slack = (3 * gg[:, None, :].expand(-1, 3, -1)).reshape(-1, 3)
        mag = torch.zeros(BV, 3, dtype=torch.float64).index_add_(0, flat, term)
        bound[:, c0:c0 + 3] = EPS * (torch.zeros(BV, 3, dtype=torch.float64).index_add_(0, flat, term + slack) + feeds[:, None] * mag)
    return bound
