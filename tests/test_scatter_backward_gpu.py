"""The tile-scatter backwards (csrc/tile_scatter.h) on adversarial rasters: a3d_interp_bwd (ip_bwd_tile_kernel, CM = 4 / 8 / 16, and
the per-pixel ip_bwd_kernel<16> beyond 16 channels) and a3d_rast_bwd (rs_bwd_kernel), plus the G-buffer backward's sum of the two
canonical-position gradients (a3d_gbuffer_bwd with g_tex).

Both scatter kernels reduce pixel -> vertex contributions through an in-wave merge of lanes on the same triangle (ts_merge), a 512-slot
LDS table with 8 linear probes, lists linked by atomicExch, and a global-atomic fallback for contributions that find no slot.  The id
maps below are fabricated so that each of those stages is forced: every merge distance, no merge at all, table hits between non-adjacent
lanes, more distinct vertex rows per tile than slots, probe exhaustion with few rows, partial tiles, empty tiles and ids out of range.
The fabricated rasters reach the entry points directly through the C ABI (_lib.call); one end-to-end case goes through ops.rasterize.

References are plain float64 torch written here: an index_add of bary * g for the interpolation, autograd of sum(g.x u + g.y v) for the
rasteriser.  Interpolation inputs are chosen so that every fp32 operation is exact, and the comparison is torch.equal.  The rasteriser
divides by s, so its bound is derived from float64 magnitudes of the terms each pixel adds, and a CPU self-check shows the bound would
catch one dropped pixel contribution.
"""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TS_SLOTS, TS_PROBES, TS_TILE = 512, 8, 16  # csrc/tile_scatter.h
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("3danimals_amd.ops")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("3danimals_amd._lib")


# ------------------------------------------------------------------------------------------------ adversarial id maps
def ts_hash(row):
    """The slot tile_scatter.h's TileScatter::slot() starts probing at: ((row * 0x9E3779B1) mod 2^32) >> 23."""
    return ((np.asarray(row, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - 9)


def _tri_xy(rng, n, min_cross=0.3):
    """n well-conditioned triangles in NDC: [n,3,2] with |cross(p1 - p0, p2 - p0)| >= min_cross (resampled until they are)."""
    xy = rng.uniform(-1.0, 1.0, (n, 3, 2))
    while True:
        e1, e2 = xy[:, 1] - xy[:, 0], xy[:, 2] - xy[:, 0]
        bad = np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) < min_cross
        if not bad.any():
            return xy
        xy[bad] = rng.uniform(-1.0, 1.0, (int(bad.sum()), 3, 2))


def _lattice_xy(ny, nx, rng):
    """Grid vertex (gy, gx) at a folded lattice point (spacing 0.6, period 4) + jitter: a triangle of neighbouring grid vertices is never
    smaller than 0.6 x 0.6 / 2 in NDC, whatever the block size in pixels."""
    gy, gx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    xy = np.stack([0.6 * (gx % 4) - 0.9, 0.6 * (gy % 4) - 0.9], -1).reshape(-1, 2)
    return xy + rng.uniform(-0.05, 0.05, xy.shape)


def _blocks(B, H, W, kh, kw, off, rng):
    """One triangle per kh x kw block (shifted by ``off`` pixels); block triangles are halves of the cells of a vertex grid, so that
    neighbouring blocks share vertices."""
    nby, nbx = (H + off) // kh + 1, (W + off) // kw + 1
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    by, bx = (y + off) // kh, (x + off) // kw
    ids = np.broadcast_to(by * nbx + bx, (B, H, W)).copy()
    gby, gbx = np.meshgrid(np.arange(nby), np.arange(nbx), indexing="ij")
    g = lambda yy, xx: yy * (nbx + 1) + xx
    even = ((gby + gbx) % 2 == 0)[..., None]
    t0 = np.stack([g(gby, gbx), g(gby, gbx + 1), g(gby + 1, gbx)], -1)
    t1 = np.stack([g(gby, gbx + 1), g(gby + 1, gbx + 1), g(gby + 1, gbx)], -1)
    tri = np.where(even, t0, t1).reshape(-1, 3)
    return ids, tri, _lattice_xy(nby + 1, nbx + 1, rng)


def make_pattern(name, B, H, W, per_image, seed=0):
    """Triangle-id map [B,H,W] (-1 = background; ids >= F are out of range), triangles [F,3], V and NDC vertex positions [V,2] of the
    named pattern.  ``per_image``: attributes / clip are [B,V,.] (vertex row b*V + idx) rather than shared [1,V,.] (row idx).

    single            one triangle over the whole frame: every merge round succeeds, one slot, every work-group's atomics meet at 3 rows
    blocks<k>[+1]     k x k blocks, aligned or offset by one pixel: partial merges at each distance of the rounds (lane ^ 1, 8, 2, 16, 4, 32)
    stripes<a>x<b>    a x b blocks (1 x k rows, k x 1 columns)
    checker           two triangles sharing an edge, alternating per pixel: no merge ever succeeds; the shared vertices meet in the table
    pool              random ids from 20 triangles over 12 vertices: the same triangle on non-adjacent lanes, table hits instead of merges
    unique            every pixel its own triangle with 3 private vertices: 768 distinct rows in a full tile > TS_SLOTS = 512, so the
                      global fallback runs whatever the hash is
    collide           WHITE-BOX: 8 triangles over 24 vertices whose rows all hash (ts_hash) to one slot, >= 2 x TS_PROBES per tile: probe
                      exhaustion with few vertices.  Mirrors tile_scatter.h's hash; a changed hash leaves this case a plain small pool
    holes             pool with ~30 % background, ~5 % ids >= F (must contribute nothing), and a few whole 16 x 16 tiles empty
    """
    rng = np.random.default_rng(seed)
    if name == "single":
        ids = np.zeros((B, H, W), np.int64)
        tri = np.array([[0, 1, 2]])
        xy = np.array([[-0.95, -0.9], [0.9, -0.8], [-0.1, 0.95]])
    elif name.startswith("blocks"):
        k, _, off = name[len("blocks"):].partition("+")
        ids, tri, xy = _blocks(B, H, W, int(k), int(k), int(off or 0), rng)
    elif name.startswith("stripes"):
        kh, kw = (int(s) for s in name[len("stripes"):].split("x"))
        ids, tri, xy = _blocks(B, H, W, kh, kw, 0, rng)
    elif name == "checker":
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        ids = np.broadcast_to((x + y) % 2, (B, H, W)).copy()
        tri = np.array([[0, 1, 2], [1, 3, 2]])
        xy = np.array([[-0.9, -0.8], [0.85, -0.7], [-0.75, 0.9], [0.8, 0.85]])
    elif name in ("pool", "holes"):
        xy = rng.uniform(-1.0, 1.0, (12, 2))
        tri = []
        while len(tri) < 20:
            t = rng.choice(12, 3, replace=False)
            e1, e2 = xy[t[1]] - xy[t[0]], xy[t[2]] - xy[t[0]]
            if abs(e1[0] * e2[1] - e1[1] * e2[0]) >= 0.3:
                tri.append(t)
        tri = np.array(tri)
        ids = rng.integers(0, 20, (B, H, W))
        if name == "holes":
            u = rng.random((B, H, W))
            ids[u < 0.3] = -1
            ids[u > 0.95] = 20 + rng.integers(0, 4, int((u > 0.95).sum()))  # out of range: f >= F
            tiles = [(b, ty, tx) for b in range(B) for ty in range(-(-H // TS_TILE)) for tx in range(-(-W // TS_TILE))]
            for j in rng.permutation(len(tiles))[: max(1, len(tiles) // 4)]:
                b, ty, tx = tiles[j]
                ids[b, ty * TS_TILE:(ty + 1) * TS_TILE, tx * TS_TILE:(tx + 1) * TS_TILE] = -1
    elif name == "unique":
        n = H * W
        ids = np.broadcast_to(np.arange(n).reshape(H, W), (B, H, W)).copy()
        tri = np.arange(3 * n).reshape(n, 3)
        xy = _tri_xy(rng, n).reshape(-1, 2)
    elif name == "collide":
        V = 20000
        tris, xy = [], rng.uniform(-1.0, 1.0, (V, 2))
        target = int(ts_hash(0))
        for b in range(B if per_image else 1):
            idx = np.arange(V)
            hit = idx[ts_hash(b * V * int(per_image) + idx) == target][:24]
            assert len(hit) == 24 and len(hit) >= 2 * TS_PROBES
            xy[hit] = _tri_xy(rng, 8).reshape(-1, 2)
            tris.append(hit.reshape(8, 3))
        tri = np.concatenate(tris)
        ids = rng.integers(0, 8, (B, H, W))
        if per_image:
            ids += 8 * np.arange(B)[:, None, None]  # image b uses the triangles whose rows collide in image b
        return ids, tri, V, xy
    else:
        raise ValueError(name)
    return ids, tri, xy.shape[0], xy


PATTERNS = (["single"] + [f"blocks{k}" for k in (1, 2, 4, 8, 16)] + [f"blocks{k}+1" for k in (1, 2, 4, 8, 16)]
            + [f"stripes1x{k}" for k in (2, 4, 16)] + [f"stripes{k}x1" for k in (2, 4, 16)] + ["checker", "pool", "unique", "collide", "holes"])


def rows_of(ids, tri, V, F, per_image):
    """(live [B,H,W], vertex rows [n,3] of the live pixels, pixel coordinates (b, y, x) of the live pixels)."""
    live = (ids >= 0) & (ids < F)
    b, y, x = np.nonzero(live)
    f = ids[b, y, x]
    rows = tri[f] + (b * V)[:, None] * int(per_image)
    return live, rows, (b, y, x)


def max_rows_in_a_full_tile(ids, tri, V, F, per_image):
    """The most distinct vertex rows any whole 16 x 16 tile references."""
    B, H, W = ids.shape
    best = 0
    for b in range(B):
        for ty in range(H // TS_TILE):
            for tx in range(W // TS_TILE):
                t = ids[b, ty * TS_TILE:(ty + 1) * TS_TILE, tx * TS_TILE:(tx + 1) * TS_TILE].reshape(-1)
                t = t[(t >= 0) & (t < F)]
                best = max(best, len(np.unique(tri[t].reshape(-1) + b * V * int(per_image))))
    return best


def raster_from_ids(ids, rng):
    """[B,H,W,4] float32 = (u, v, z, id + 1) with u, v multiples of 1/16 and 1 - u - v >= 1/16 (background / out-of-range pixels get
    values too: the kernels must not read them)."""
    a = rng.integers(0, 16, ids.shape)
    b = (rng.random(ids.shape) * (16 - a)).astype(np.int64)  # 0 <= b <= 15 - a
    rast = np.stack([a / 16.0, b / 16.0, rng.uniform(0.0, 1.0, ids.shape), np.maximum(ids, -1) + 1.0], -1)
    return torch.from_numpy(rast).float()


# ------------------------------------------------------------------------------------------------ a3d_interp_bwd: bit-exact
def _interp_case(L, dev, ids, tri, V, per_image, C, seed, want_g_attr=True):
    """Run a3d_interp_fwd / a3d_interp_bwd on the fabricated raster and compare with the float64 reference, torch.equal throughout.

    Exactness: u, v are multiples of 1/16 with 1 - u - v >= 1/16, attributes integers in [-8, 8], upstream gradients non-zero integers
    in [-4, 4].  Every product is then exact in fp32; every term of g_attr is a multiple of 1/16 of magnitude < 4, so with
    B*H*W <= 2^18 every partial sum of one element is below 2^20 and is exact too (24 bits = 20 integer + 4 fractional); forward values
    and g_rast sums are integers or 1/16 multiples far below that.  Every summation order gives the same fp32 number, so one lost,
    doubled or misrouted contribution changes the result."""
    B, H, W = ids.shape
    assert B * H * W <= 2 ** 18, "the exactness bound: B*H*W <= 2^18"
    rng = np.random.default_rng(seed)
    F = tri.shape[0]
    Ba = B if per_image else 1
    attr = torch.from_numpy(rng.integers(-8, 9, (Ba, V, C))).float()
    g = torch.from_numpy(rng.integers(1, 5, (B, H, W, C)) * rng.choice([-1, 1], (B, H, W, C))).float()
    rast = raster_from_ids(ids, rng)
    # float64 reference
    live, rows, (pb, py, px) = rows_of(ids, tri, V, F, per_image)
    rows_t = torch.from_numpy(rows)
    r64 = rast.double()[pb, py, px]
    bary = torch.stack([r64[:, 0], r64[:, 1], 1.0 - r64[:, 0] - r64[:, 1]], -1)  # [n,3]
    A = attr.double().reshape(Ba * V, C)[rows_t]  # [n,3,C]
    g64 = g.double()[pb, py, px]  # [n,C]
    out_ref = torch.zeros(B, H, W, C, dtype=torch.float64)
    out_ref[pb, py, px] = (bary[..., None] * A).sum(1)
    g_attr_ref = torch.zeros(Ba * V, C, dtype=torch.float64).index_add_(0, rows_t.reshape(-1), (bary[..., None] * g64[:, None, :]).reshape(-1, C))
    g_rast_ref = torch.zeros(B, H, W, 4, dtype=torch.float64)
    g_rast_ref[pb, py, px, 0] = (g64 * (A[:, 0] - A[:, 2])).sum(-1)
    g_rast_ref[pb, py, px, 1] = (g64 * (A[:, 1] - A[:, 2])).sum(-1)
    # the kernels, through the C ABI (outputs poisoned: anything a kernel fails to write shows up as NaN)
    tri_d = torch.from_numpy(tri).int().to(dev)
    attr_d, rast_d, g_d = attr.to(dev), rast.to(dev), g.to(dev)
    out = torch.full((B, H, W, C), float("nan"), device=dev)
    L.call("a3d_interp_fwd", L.ptr(attr_d), Ba, C, L.ptr(rast_d), L.ptr(tri_d), B, V, F, H, W, L.ptr(out), L.stream())
    g_attr = torch.full((Ba, V, C), float("nan"), device=dev) if want_g_attr else None
    g_rast = torch.full((B, H, W, 4), float("nan"), device=dev)
    L.call("a3d_interp_bwd", L.ptr(g_d), L.ptr(attr_d), Ba, C, L.ptr(rast_d), L.ptr(tri_d), B, V, F, H, W, L.ptr(g_attr), L.ptr(g_rast),
           L.stream())
    torch.cuda.synchronize()
    out, g_rast = out.cpu(), g_rast.cpu()
    assert torch.equal(out, out_ref.float()), "forward"
    assert torch.equal(g_rast[..., :2], g_rast_ref[..., :2].float()), "g_rast[..., :2]"
    assert torch.equal(g_rast[..., 2:], torch.zeros(B, H, W, 2)), "g_rast[..., 2:]"
    if want_g_attr:
        got = g_attr.cpu().reshape(Ba * V, C)
        ref = g_attr_ref.float()
        bad = (got != ref).any(-1).nonzero().reshape(-1)
        assert bad.numel() == 0, (f"g_attr differs at {bad.numel()} of {Ba * V} vertex rows, e.g. row {int(bad[0])}: "
                                  f"{got[bad[0]].tolist()} vs {ref[bad[0]].tolist()}")
    return live


INTERP_C = [1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 33, 64]  # tile kernel CM = 4 (1..4), 8 (5..8), 16 (9..16); per-pixel kernel beyond 16


@pytest.mark.parametrize("per_image", [False, True], ids=["shared", "per_image"])
@pytest.mark.parametrize("C", INTERP_C)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_interp_bwd_exact_on_pattern(pattern, C, per_image, dev, L):
    """B = 2, 40 x 52: six whole tiles and partial tiles along the right (4 columns) and bottom (8 rows) edges."""
    B, H, W = 2, 40, 52
    ids, tri, V, _ = make_pattern(pattern, B, H, W, per_image, seed=C)
    if pattern == "unique":
        assert max_rows_in_a_full_tile(ids, tri, V, tri.shape[0], per_image) > TS_SLOTS
    if pattern == "collide":
        live, rows, _ = rows_of(ids, tri, V, tri.shape[0], per_image)
        assert len(np.unique(ts_hash(np.unique(rows)))) == 1 and len(np.unique(rows)) // (B if per_image else 1) >= 2 * TS_PROBES
    _interp_case(L, dev, ids, tri, V, per_image, C, seed=C)


FRAMES = [(1, 1), (1, 300), (250, 3), (17, 33), (16, 16), (256, 256)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", FRAMES, ids=[f"{h}x{w}" for h, w in FRAMES])
def test_interp_bwd_exact_frame_shapes(H, W, B, dev, L):
    """Degenerate and odd frames (one pixel, one row, one column, partial tiles only, exactly one tile) and a large frame (B = 3 x 256 x 256
    = 196608 pixels <= 2^18), shared and per-image attributes, each tile instance and the per-pixel kernel."""
    for k, (pattern, C, per_image) in enumerate([("pool", 3, False), ("holes", 8, True), ("single", 16, False), ("blocks2+1", 33, True),
                                                 ("unique", 12, True), ("checker", 5, False)]):
        ids, tri, V, _ = make_pattern(pattern, B, H, W, per_image, seed=k)
        _interp_case(L, dev, ids, tri, V, per_image, C, seed=k)


def test_interp_bwd_without_g_attr_exact_g_rast(dev, L):
    """attr without a gradient: g_attr == nullptr (no table, no flush), g_rast still exact, for every kernel instance."""
    ids, tri, V, _ = make_pattern("holes", 2, 37, 45, True, seed=5)
    for C in (3, 6, 12, 20):
        _interp_case(L, dev, ids, tri, V, True, C, seed=C, want_g_attr=False)


def test_interp_bwd_rejects_more_than_64_channels(dev, L):
    """IP_MAXC = 64: C = 65 is refused at the entry point (A3DError), nothing is launched."""
    ids, tri, V, _ = make_pattern("pool", 1, 16, 16, False)
    rast = raster_from_ids(ids, np.random.default_rng(0)).to(dev)
    C = 65
    attr = torch.zeros(1, V, C, device=dev)
    g = torch.zeros(1, 16, 16, C, device=dev)
    g_attr, g_rast = torch.empty_like(attr), torch.empty_like(rast)
    tri_d = torch.from_numpy(tri).int().to(dev)
    with pytest.raises(L.A3DError):
        L.call("a3d_interp_bwd", L.ptr(g), L.ptr(attr), 1, C, L.ptr(rast), L.ptr(tri_d), 1, V, tri.shape[0], 16, 16, L.ptr(g_attr), L.ptr(g_rast),
               L.stream())


@pytest.mark.parametrize("C", [5, 12])
def test_interp_autograd_reaches_the_cm8_cm16_tile_kernels(C, dev, ops):
    """ops.interpolate's backward (the public route to the CM = 8 and CM = 16 instances) on the exact inputs: torch.equal."""
    B, H, W = 2, 33, 47
    ids, tri, V, _ = make_pattern("pool", B, H, W, True, seed=C)
    rng = np.random.default_rng(C)
    rast = raster_from_ids(ids, rng)
    attr = torch.from_numpy(rng.integers(-8, 9, (B, V, C))).float()
    g = torch.from_numpy(rng.integers(1, 5, (B, H, W, C)) * rng.choice([-1, 1], (B, H, W, C))).float()
    a = attr.to(dev).requires_grad_(True)
    r = rast.to(dev).requires_grad_(True)
    out = ops.interpolate(a, r, torch.from_numpy(tri).to(dev))
    (out * g.to(dev)).sum().backward()
    live, rows, (pb, py, px) = rows_of(ids, tri, V, tri.shape[0], True)
    r64 = rast.double()[pb, py, px]
    bary = torch.stack([r64[:, 0], r64[:, 1], 1.0 - r64[:, 0] - r64[:, 1]], -1)
    ref = torch.zeros(B * V, C, dtype=torch.float64).index_add_(0, torch.from_numpy(rows).reshape(-1),
                                                                 (bary[..., None] * g.double()[pb, py, px][:, None, :]).reshape(-1, C))
    assert torch.equal(a.grad.cpu().reshape(B * V, C), ref.float())


# ------------------------------------------------------------------------------------------------ a3d_rast_bwd: derived bound
def _clip_of(xy, per_image, B, seed):
    """Clip coordinates [B|1,V,4] of NDC positions: (x w, y w, z w, w) with w in [0.8, 1.25] per vertex and image."""
    rng = np.random.default_rng(seed)
    Bc = B if per_image else 1
    w = rng.uniform(0.8, 1.25, (Bc, 1, 1)) * rng.uniform(0.95, 1.05, (Bc, xy.shape[0], 1))
    z = rng.uniform(-0.5, 0.5, (Bc, xy.shape[0], 1))
    return torch.from_numpy(np.concatenate([xy[None] * w, z * w, w], -1)).float()


def _pixel_f(px, W):
    """The pixel centre in NDC as rs_bwd_kernel computes it, ((px + 0.5) * (2/W)_fp32 - 1) rounded once to fp32, as float64."""
    k = float(np.float32(2.0) / np.float32(W))
    return torch.from_numpy(((px + 0.5) * k - 1.0).astype(np.float32).astype(np.float64))


def rast_bwd_reference(ids, tri, V, per_image, clip, g_rast):
    """Float64 reference of a3d_rast_bwd and its error bound.

    Per live pixel (0 <= id < F): q_i = p_i.xy - f p_i.w, a_i = q_j x q_k, s = sum a_i, u = a0 / s, v = a1 / s and the gradient of
    L = g.x u + g.y v w.r.t. the clip (x, y, w) of its three vertices, by autograd; pixels with s == 0 contribute nothing.

    Bound per output element = 2^-24 * (2 * sum_p D_p + 64 * sum_p |c_p|) over the pixels p that feed it.  |c_p| = the sum of the
    absolute values of the terms the kernel adds for that element (|ga1 q2y| + |ga2 q1y| for x of vertex 0, ...): rounding of the final
    products and the summation across merges, lists and atomics.  D_p = the same terms' first-order error propagated from the fp32
    inputs in units of 2^-24: q carries |p.xy| + |f p.w| + (2|f| + 1)|p.w| (its own rounding and that of f), a_i, s, 1/s, u, v and
    g.x - t carry theirs forward.  For a well-conditioned triangle D_p is a few |c_p|; it grows where q cancels (pixels very close to a
    vertex) -- where fp32 itself cannot do better.

    Returns (reference [Bc*V,4], bound [Bc*V,4], number of contributing pixels per row [Bc*V], per-pixel contributions [n,3,4],
    rows [n,3])."""
    B, H, W = ids.shape
    F = tri.shape[0]
    Bc = clip.shape[0]
    _, rows, (pb, py, px) = rows_of(ids, tri, V, F, per_image)
    rows_t = torch.from_numpy(rows)
    P = clip.double().reshape(Bc * V, 4)[rows_t].clone().requires_grad_(True)  # [n,3,4]
    g = g_rast.double()[pb, py, px]
    gx, gy = g[:, 0], g[:, 1]
    fx, fy = _pixel_f(px, W), _pixel_f(py, H)
    f = torch.stack([fx, fy], -1)[:, None, :]  # [n,1,2]
    q = P[..., :2] - f * P[..., 3:4]
    a = [q[:, (i + 1) % 3, 0] * q[:, (i + 2) % 3, 1] - q[:, (i + 1) % 3, 1] * q[:, (i + 2) % 3, 0] for i in range(3)]
    s = a[0] + a[1] + a[2]
    ok = (s != 0) & ((gx != 0) | (gy != 0))
    s_safe = torch.where(ok, s, torch.ones_like(s))
    lsum = torch.where(ok, gx * a[0] / s_safe + gy * a[1] / s_safe, torch.zeros_like(s)).sum()
    (c,) = torch.autograd.grad(lsum, P)
    c = c.detach()
    # magnitudes (float64, no autograd)
    with torch.no_grad():
        p, q = P.detach(), q.detach()
        ab = [x.abs() for x in a]
        a = [x.detach() for x in a]
        s = s.detach()
        aq = q.abs()
        af = f.abs()
        Dq = p[..., :2].abs() + af * p[..., 3:4].abs() + (2 * af + 1) * p[..., 3:4].abs() + aq  # [n,3,2]
        Da = []
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            Da.append(aq[:, j, 0] * Dq[:, k, 1] + aq[:, k, 1] * Dq[:, j, 0] + aq[:, j, 1] * Dq[:, k, 0] + aq[:, k, 0] * Dq[:, j, 1]
                      + 2 * (aq[:, j, 0] * aq[:, k, 1] + aq[:, j, 1] * aq[:, k, 0]))
        Ds = Da[0] + Da[1] + Da[2] + 2 * (ab[0] + ab[1] + ab[2])
        ss = torch.where(ok, s.abs(), torch.ones_like(s))
        u, v = a[0] / ss * torch.sign(s), a[1] / ss * torch.sign(s)
        Du, Dv = (Da[0] + u.abs() * Ds) / ss + u.abs(), (Da[1] + v.abs() * Ds) / ss + v.abs()
        Dis = Ds / ss ** 2 + 1 / ss
        t = gx * u + gy * v
        Dt = gx.abs() * Du + gy.abs() * Dv + 2 * (gx.abs() * u.abs() + gy.abs() * v.abs())
        ga = [(gx - t) / ss * torch.sign(s), (gy - t) / ss * torch.sign(s), -t / ss * torch.sign(s)]
        num = [(gx - t).abs(), (gy - t).abs(), t.abs()]
        Dga = [Dt / ss + num[i] * Dis + 2 * ga[i].abs() for i in range(3)]
        mag = torch.zeros_like(c)  # sum of |terms| per (pixel, vertex, component)
        err = torch.zeros_like(c)  # first-order propagated error, units of 2^-24
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            # d a_j / d q_i and d a_k / d q_i: c_ix = -ga_j q_ky + ga_k q_jy,  c_iy = ga_j q_kx - ga_k q_jx
            for comp, other in ((0, 1), (1, 0)):
                m = ga[j].abs() * aq[:, k, other] + ga[k].abs() * aq[:, j, other]
                mag[:, i, comp] = m
                err[:, i, comp] = (Dga[j] * aq[:, k, other] + ga[j].abs() * Dq[:, k, other] + Dga[k] * aq[:, j, other]
                                   + ga[k].abs() * Dq[:, j, other] + 2 * m)
            # w: -fx c_ix - fy c_iy
            dfx, dfy = 2 * fx.abs() + 1, 2 * fy.abs() + 1
            mag[:, i, 3] = fx.abs() * mag[:, i, 0] + fy.abs() * mag[:, i, 1]
            err[:, i, 3] = (fx.abs() * err[:, i, 0] + c[:, i, 0].abs() * dfx + fy.abs() * err[:, i, 1] + c[:, i, 1].abs() * dfy
                            + 2 * mag[:, i, 3])
        keep = ok[:, None, None].double()
        mag, err = mag * keep, err * keep
        flat = rows_t.reshape(-1)
        ref = torch.zeros(Bc * V, 4, dtype=torch.float64).index_add_(0, flat, c.reshape(-1, 4))
        bound = EPS * torch.zeros(Bc * V, 4, dtype=torch.float64).index_add_(0, flat, (2 * err + 64 * mag).reshape(-1, 4))
        feeds = torch.zeros(Bc * V, dtype=torch.int64).index_add_(0, flat, ok[:, None].expand(-1, 3).reshape(-1).long())
    return ref, bound, feeds, c, rows_t, ok


def rast_violations(got, ref, bound):
    """Rows of [Bc*V,4] where |got - ref| exceeds the bound in x, y or w (column 2 is checked separately: exactly 0)."""
    d = (got.double() - ref).abs()[:, [0, 1, 3]]
    return (d > bound[:, [0, 1, 3]]).any(-1).nonzero().reshape(-1)


def _check_rast(got, ref, bound, feeds):
    assert torch.isfinite(got).all()
    assert torch.equal(got[:, 2], torch.zeros_like(got[:, 2])), "g_clip[..., 2] must be exactly 0"
    dead = feeds == 0
    assert torch.equal(got[dead], torch.zeros_like(got[dead])), f"{int((got[dead] != 0).any(-1).sum())} rows no pixel feeds are not 0"
    bad = rast_violations(got, ref, bound)
    if bad.numel():
        r = int(bad[0])
        pytest.fail(f"g_clip outside the bound at {bad.numel()} rows, e.g. row {r}: got {got[r].tolist()}, ref {ref[r].tolist()}, "
                    f"bound {bound[r].tolist()}")


def _rast_case(L, dev, ids, tri, V, xy, per_image, seed):
    B, H, W = ids.shape
    rng = np.random.default_rng(seed)
    clip = _clip_of(xy, per_image, B, seed)
    g = torch.from_numpy(rng.normal(0.0, 1.0, (B, H, W, 4))).float()  # (z, w of g are ignored by the kernel)
    g[..., :2][torch.from_numpy(rng.random((B, H, W)) < 0.1)] = 0.0  # pixels whose upstream g is (0, 0) contribute nothing
    rast = raster_from_ids(ids, rng)
    ref, bound, feeds, _, _, _ = rast_bwd_reference(ids, tri, V, per_image, clip, g)
    Bc = clip.shape[0]
    clip_d, g_d, rast_d = clip.to(dev), g.to(dev), rast.to(dev)
    tri_d = torch.from_numpy(tri).int().to(dev)
    g_clip = torch.full((Bc, V, 4), float("nan"), device=dev)
    L.call("a3d_rast_bwd", L.ptr(g_d), L.ptr(rast_d), L.ptr(clip_d), Bc, L.ptr(tri_d), B, V, tri.shape[0], H, W, L.ptr(g_clip), L.stream())
    torch.cuda.synchronize()
    _check_rast(g_clip.cpu().reshape(Bc * V, 4), ref, bound, feeds)
    return feeds


@pytest.mark.parametrize("per_image", [False, True], ids=["shared", "per_image"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_rast_bwd_on_pattern(pattern, per_image, dev, L):
    """B = 2, 40 x 52 (whole and partial tiles), ~10 % of the pixels with upstream g = (0, 0)."""
    B, H, W = 2, 40, 52
    ids, tri, V, xy = make_pattern(pattern, B, H, W, per_image, seed=7)
    if pattern == "unique":
        assert max_rows_in_a_full_tile(ids, tri, V, tri.shape[0], per_image) > TS_SLOTS
    feeds = _rast_case(L, dev, ids, tri, V, xy, per_image, seed=7)
    assert int((feeds > 0).sum()) > 0


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", FRAMES, ids=[f"{h}x{w}" for h, w in FRAMES])
def test_rast_bwd_frame_shapes(H, W, B, dev, L):
    """The frames of test_interp_bwd_exact_frame_shapes, shared and per-image clip."""
    for k, (pattern, per_image) in enumerate([("pool", False), ("holes", True), ("single", True), ("blocks4+1", False), ("unique", True)]):
        ids, tri, V, xy = make_pattern(pattern, B, H, W, per_image, seed=k)
        _rast_case(L, dev, ids, tri, V, xy, per_image, seed=k)


def _dyadic_soup_with_degenerates(H, W):
    """Triangles on a power-of-two frame with coordinates of a few bits (NDC multiples of 1/8, w in {0.5, 1, 1.5}): f = (2 px + 1)/W - 1
    is exact, so is every q and every product, and a triangle with two coincident vertices has s == 0 in fp32 as in float64.
    Returns (ids, tri, V, clip [1,V,4], degenerate triangle ids)."""
    rng = np.random.default_rng(11)
    good = [[(-7, -6), (6, -5), (-1, 7)], [(-6, 6), (7, -7), (7, 7)], [(-7, 2), (3, -7), (2, 5)]]
    degen = [[(-3, 3), (5, -2), (5, -2)], [(4, 4), (4, 4), (-6, 1)]]  # two coincident vertices each
    tris = good + degen
    xy = np.array([v for t in tris for v in t], np.float64) / 8.0
    w = rng.choice([0.5, 1.0, 1.5], (len(xy), 1))
    for t in (3, 4):  # coincident means the same clip coordinates
        i0 = 3 * t
        same = [i0 + 1, i0 + 2] if t == 3 else [i0, i0 + 1]
        w[same[1]] = w[same[0]]
    clip = torch.from_numpy(np.concatenate([xy * w, 0.25 * w, w], -1)[None]).float()
    tri = np.arange(3 * len(tris)).reshape(-1, 3)
    ids = rng.integers(0, len(tris), (1, H, W))
    return ids, tri, tri.size, clip, [3, 4]


@pytest.mark.parametrize("H,W", [(16, 16), (32, 64)])
def test_rast_bwd_degenerate_triangles_contribute_nothing(H, W, dev, L):
    """Exactly degenerate triangles (coincident vertices: s == 0 in both precisions) between well-conditioned ones: their private vertices
    get exactly 0, the others stay within the bound."""
    ids, tri, V, clip, degen = _dyadic_soup_with_degenerates(H, W)
    rng = np.random.default_rng(2)
    g = torch.from_numpy(rng.normal(0.0, 1.0, (1, H, W, 4))).float()
    rast = raster_from_ids(ids, rng)
    ref, bound, feeds, c, rows, ok = rast_bwd_reference(ids, tri, V, False, clip, g)
    f = torch.from_numpy(ids[ids >= 0])
    is_degen = (f == degen[0]) | (f == degen[1])
    assert bool(is_degen.any()) and not bool(ok[is_degen].any()), "s == 0 exactly in float64 for the degenerate triangles"
    # ... and in fp32, whatever the contraction: q and the products are exact (checked: float32 arithmetic gives the float64 values)
    _, _, (pb, py, px) = rows_of(ids, tri, V, tri.shape[0], False)
    P32 = clip.reshape(V, 4)[rows]
    f32 = torch.stack([_pixel_f(px, W).float(), _pixel_f(py, H).float()], -1)[:, None, :]
    q32 = P32[..., :2] - f32 * P32[..., 3:4]
    q64 = clip.double().reshape(V, 4)[rows][..., :2] - f32.double() * clip.double().reshape(V, 4)[rows][..., 3:4]
    assert torch.equal(q32.double(), q64)
    prods = torch.stack([q64[:, j, 0] * q64[:, k, 1] for j in range(3) for k in range(3)] +
                        [q64[:, j, 1] * q64[:, k, 0] for j in range(3) for k in range(3)], -1)
    assert torch.equal(prods.float().double(), prods), "every product of the cross products is exact in fp32 (fma or not)"
    clip_d, g_d, rast_d = clip.to(dev), g.to(dev), rast.to(dev)
    tri_d = torch.from_numpy(tri).int().to(dev)
    g_clip = torch.full((1, V, 4), float("nan"), device=dev)
    L.call("a3d_rast_bwd", L.ptr(g_d), L.ptr(rast_d), L.ptr(clip_d), 1, L.ptr(tri_d), 1, V, tri.shape[0], H, W, L.ptr(g_clip), L.stream())
    torch.cuda.synchronize()
    got = g_clip.cpu().reshape(V, 4)
    for t in degen:
        assert torch.equal(got[tri[t]], torch.zeros(3, 4)), f"degenerate triangle {t} contributed"
    _check_rast(got, ref, bound, feeds)


def test_rast_bwd_bound_catches_one_dropped_contribution():
    """Sensitivity self-check, CPU only: the comparison of test_rast_bwd_* applied to the float64 reference with ONE pixel's contribution
    removed at a sample of vertices must fail.  Soup of well-conditioned triangles (B = 2, 64 x 64, per-image clip, the 'pool' and
    'blocks8' patterns), the removed pixel the one of median magnitude among those that feed the vertex."""
    for pattern in ("pool", "blocks8", "holes"):
        B, H, W = 2, 64, 64
        ids, tri, V, xy = make_pattern(pattern, B, H, W, True, seed=3)
        rng = np.random.default_rng(3)
        clip = _clip_of(xy, True, B, 3)
        g = torch.from_numpy(rng.normal(0.0, 1.0, (B, H, W, 4))).float()
        ref, bound, feeds, c, rows, ok = rast_bwd_reference(ids, tri, V, True, clip, g)
        assert rast_violations(ref, ref, bound).numel() == 0
        fed = (feeds > 1).nonzero().reshape(-1)
        sample = fed[torch.from_numpy(rng.permutation(fed.numel())[:16])]
        assert sample.numel() >= 8
        for r in sample.tolist():
            where = (rows == r).nonzero()  # (pixel, corner) pairs of row r
            where = where[ok[where[:, 0]]]
            size = c[where[:, 0], where[:, 1]].abs().amax(-1)
            pick = where[int(torch.argsort(size)[size.numel() // 2])]
            dropped = ref.clone()
            dropped[r] -= c[pick[0], pick[1]]
            bad = rast_violations(dropped, ref, bound)
            assert r in bad.tolist(), (pattern, r, int(feeds[r]), (dropped[r] - ref[r]).tolist(), bound[r].tolist())


def test_rast_bwd_end_to_end_one_triangle_per_pixel(dev, ops):
    """ops.rasterize autograd on a real soup: one tiny triangle around each pixel centre of a 37 x 53 frame, private vertices.  The
    public route and the 'unique' overflow together (6 whole tiles of 768 distinct rows each > 512 slots)."""
    H, W = 37, 53
    rng = np.random.default_rng(4)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cx, cy = ((xs + 0.5) * 2 / W - 1).reshape(-1), ((ys + 0.5) * 2 / H - 1).reshape(-1)
    offs = np.array([[-1.0, -0.8], [1.0, -0.7], [0.1, 1.1]]) * np.array([0.6 / W, 0.6 / H])
    xy = (np.stack([cx, cy], -1)[:, None, :] + offs[None]).reshape(-1, 2)
    clip = _clip_of(xy, False, 1, 4)
    tri = np.arange(3 * H * W).reshape(-1, 3)
    V = tri.size
    c_d = clip.to(dev).requires_grad_(True)
    rast = ops.rasterize(c_d, torch.from_numpy(tri).int().to(dev), (H, W))
    ids = (rast[..., 3].detach().cpu().numpy().astype(np.int64) - 1)
    assert np.array_equal(ids[0], np.arange(H * W).reshape(H, W)), "every pixel owned by its own triangle"
    assert max_rows_in_a_full_tile(ids, tri, V, tri.shape[0], False) > TS_SLOTS
    g = torch.from_numpy(rng.normal(0.0, 1.0, (1, H, W, 4))).float()
    g[..., 2:] = 0.0  # (z/w and the id get no gradient: only (u, v) reach a3d_rast_bwd)
    (rast * g.to(dev)).sum().backward()
    ref, bound, feeds, _, _, _ = rast_bwd_reference(ids, tri, V, False, clip, g)
    _check_rast(c_d.grad.cpu().reshape(V, 4), ref, bound, feeds)


# ------------------------------------------------------------------------------------------------ a3d_gbuffer_bwd: g_tex is summed
@pytest.mark.parametrize("shared", [True, False], ids=["shared_prior", "per_image_prior"])
@pytest.mark.parametrize("loss", ["gb_only", "tex_only", "both"])
def test_gbuffer_bwd_sums_g_tex_and_gb_canonical_columns(loss, shared, dev, ops):
    """covered_gbuffer(..., field_inputs=bucket) hands out the canonical position twice: gb[:, 9:12] and tex_in.  The gradient w.r.t.
    prior_v_pos must be the float64 index_add of bary * (w_gb + w_tex) for a loss that reads either or both."""
    B, H, W, bucket = 2, 32, 40, 64
    rng = np.random.default_rng(9)
    xy = _tri_xy(rng, 24, min_cross=0.05).reshape(-1, 2) * 0.9
    V = xy.shape[0]
    clip = _clip_of(xy, True, B, 9).to(dev)
    tri = torch.arange(V, dtype=torch.int32).reshape(-1, 3).to(dev)
    v_pos = torch.from_numpy(rng.normal(0, 1, (B, V, 3))).float().to(dev)
    v_nrm = torch.nn.functional.normalize(torch.from_numpy(rng.normal(0, 1, (B, V, 3))).float(), dim=-1).to(dev)
    prior = torch.from_numpy(rng.normal(0, 1, (1 if shared else B, V, 3))).float().to(dev).requires_grad_(True)
    rast = ops.rasterize(clip, tri, (H, W))
    gb, pix, inv, tex_in, img = ops.covered_gbuffer(clip, v_pos, v_nrm, prior, rast, tri, field_inputs=bucket)
    P = gb.shape[0]
    assert P > 200 and tex_in.shape[0] % bucket == 0 and tex_in.shape[0] >= P
    w_gb = torch.from_numpy(rng.uniform(-1, 1, (P, 3))).float()
    w_tex = torch.from_numpy(rng.uniform(-2, 2, (P, 3))).float()
    terms = []
    if loss in ("gb_only", "both"):
        terms.append((gb[:, 9:12] * w_gb.to(dev)).sum())
    if loss in ("tex_only", "both"):
        terms.append((tex_in[:P] * w_tex.to(dev)).sum())
    (got,) = torch.autograd.grad(sum(terms), [prior])
    # float64 reference: canonical = sum_k bary_k prior[row_k], bary = (u, v, 1 - u - v) of the listed pixel
    wsum = (w_gb if loss != "tex_only" else 0 * w_gb) + (w_tex if loss != "gb_only" else 0 * w_tex)
    pix_c = pix.cpu()
    r = rast.detach().cpu().double().reshape(-1, 4)[pix_c]
    f = r[:, 3].long() - 1
    b = pix_c // (H * W)
    rows = tri.cpu().long()[f] + (0 if shared else b[:, None] * V)
    bary = torch.stack([r[:, 0], r[:, 1], 1 - r[:, 0] - r[:, 1]], -1)
    contrib = bary[..., None] * wsum.double()[:, None, :]  # [P,3,3]
    Bp = prior.shape[0]
    ref = torch.zeros(Bp * V, 3, dtype=torch.float64).index_add_(0, rows.reshape(-1), contrib.reshape(-1, 3))
    scale = torch.zeros(Bp * V, 3, dtype=torch.float64).index_add_(0, rows.reshape(-1), contrib.abs().reshape(-1, 3))
    err = (got.cpu().double().reshape(Bp * V, 3) - ref).abs()
    worst = int(torch.argmax((err - 1e-4 * scale).max(-1).values))
    assert bool((err <= 1e-4 * scale + 1e-30).all()), (f"d loss / d prior_v_pos ({loss}): row {worst} got "
                                                       f"{got.cpu().reshape(Bp * V, 3)[worst].tolist()}, want {ref[worst].tolist()}")
