"""The hand-made rasters tests/test_aa_cpu.py and tests/test_aa_adversarial_gpu.py run the silhouette antialiasing on, and the RUNS
(a case + the buffers of one call) they evaluate.  Each case is the smallest shape at which its site in csrc/antialias.hip can go
wrong; every frame is under 2000 pixels.

The basic cell is the one-pixel triangle of silhouette_scene in tests/test_scan_boundaries_gpu.py: corners (0.5625, -0.25), (-0.25,
1.25), (1.25, 1.25) from the pixel's corner -- all multiples of 1/32 -- turned by quarter turns about the pixel's centre where a case
wants the long side elsewhere.  On a power-of-two frame with every w a power of two each product of the analysis is exact in float32
(a LATTICE case: ``lattice`` True; float32 and float64 then decide identically, tests/test_aa_cpu.py).  The raster is HAND-MADE: ids
and depths are written directly, the analysis reads nothing else of it, so a texel may name a triangle that does not cover it.

build(name) -> dict(name, rast [B,H,W,4], clip [1|B,V,4], tri int64 [F,3], B, H, W, lattice, expect).  Names carry the frame as HxW.
"""
import functools
import zlib

import numpy as np
import torch

import aa_ref as A

CELL = np.array([[0.0625, -0.75], [-0.75, 0.75], [0.75, 0.75]])  # the basic cell from the pixel's CENTRE (y down): long side below


def cell(x, y, turn=0):
    """The basic cell at pixel (x, y), turned by ``turn`` quarter turns: 0 reaches down (crossing distances: left 0.34375, right 0.40625,
    down 0.75, up none), 1 left, 2 up, 3 right.  [3,2] pixel coordinates."""
    p = CELL.copy()
    for _ in range(turn % 4):
        p = np.stack([-p[:, 1], p[:, 0]], 1)
    return p + np.array([x + 0.5, y + 0.5])


class Scene:
    """Triangles in pixel coordinates (private vertices unless ``share`` names existing ones) and a raster written texel by texel."""

    def __init__(self, B, H, W):
        self.B, self.H, self.W = B, H, W
        self.pts, self.w, self.tri = [], [], []
        self.rast = torch.zeros(B, H, W, 4)

    def vertex(self, p, w=1.0):
        self.pts.append([float(p[0]), float(p[1])])
        self.w.append(float(w))
        return len(self.pts) - 1

    def add(self, pts, w=(1.0, 1.0, 1.0), share=(None, None, None)):
        """-> triangle id; ``share``: per corner an existing vertex index instead of a new vertex."""
        self.tri.append([self.vertex(p, wi) if s is None else s for p, wi, s in zip(pts, w, share)])
        return len(self.tri) - 1

    def own(self, b, y, x, t, depth=0.25):
        self.rast[b, y, x, 2] = depth
        self.rast[b, y, x, 3] = t + 1

    def finish(self, name, lattice, image_w=None, expect=None):
        """``image_w``: per image a factor on every clip coordinate (a per-image clip tensor [B,V,4]: x / w unchanged); None: one shared."""
        pts, w = np.asarray(self.pts, np.float64).reshape(-1, 2), np.asarray(self.w, np.float64)
        ndc = pts / np.array([self.W / 2.0, self.H / 2.0]) - 1.0
        clip = np.concatenate([ndc * w[:, None], np.zeros((len(w), 1)), w[:, None]], 1)[None]
        if image_w is not None:
            clip = clip * np.asarray(image_w, np.float64)[:, None, None]
        tri = torch.tensor(self.tri, dtype=torch.long).reshape(-1, 3)
        return dict(name=name, rast=self.rast, clip=torch.from_numpy(clip).float().contiguous(), tri=tri, B=self.B, H=self.H, W=self.W, lattice=lattice,
                    expect=expect or {})


def _pow2(n):
    return n & (n - 1) == 0


def _size(name):
    h, w = name.rsplit("_", 1)[1].split("x")
    return int(h), int(w)


def checker(name, H, W, every=False, seed=0, w_choices=None, negative_w=None, rows=None):
    """Pixels with x + y even (``every``: all) own a cell each; ``every`` draws the depths from {0, 1/8, 2/8, 3/8} (ties: the depth rule
    decides).  ``w_choices``: every vertex' w drawn from them; ``negative_w`` = (triangle, corner, w); ``rows``: only the first rows."""
    rng = np.random.default_rng(seed)
    s = Scene(1, H, W)
    for y in range(H):
        for x in range(W):
            if (every or (x + y) % 2 == 0) and (rows is None or y < rows):
                w = (1.0, 1.0, 1.0) if w_choices is None else tuple(rng.choice(w_choices, 3))
                if negative_w is not None and len(s.tri) == negative_w[0]:
                    w = tuple(negative_w[2] if k == negative_w[1] else wk for k, wk in enumerate(w))
                s.own(0, y, x, s.add(cell(x, y), w), float(rng.integers(0, 4)) / 8.0 if every else 0.25)
    return s.finish(name, _pow2(H) and _pow2(W))


def batch3(name, H, W, shared):
    """Image 0 a checkerboard, image 1 nothing covered, image 2 covered by ONE id everywhere (no candidate pair).  ``shared``: one clip
    tensor [1,V,4] for the three images, else [3,V,4] (image b's coordinates all scaled by 2^b: same screen positions)."""
    s = Scene(3, H, W)
    for y in range(H):
        for x in range(W):
            if (x + y) % 2 == 0:
                s.own(0, y, x, s.add(cell(x, y)))
    s.rast[2, ..., 2] = 0.5
    s.rast[2, ..., 3] = 1.0
    return s.finish(name, False, None if shared else (1.0, 2.0, 4.0))


def four(name, H, W, roles):
    """An inner pixel whose four neighbours each own a cell reaching towards it, at depth 1/8.  ``roles`` False (four_blends): the pixel is
    uncovered and is the destination of four blends.  True (four_roles): it is covered by a farther triangle (depth 1/2), so it is the
    first pixel of a right and a lower record and the second pixel of a left and an upper one -- all four slots of its g_slots row."""
    s = Scene(1, H, W)
    cx, cy = W // 2, H // 2
    for (dx, dy), turn in (((0, -1), 0), ((1, 0), 1), ((0, 1), 2), ((-1, 0), 3)):
        s.own(0, cy + dy, cx + dx, s.add(cell(cx + dx, cy + dy, turn)), 0.125)
    if roles:
        s.own(0, cy, cx, s.add(np.array([[cx - 3.25, cy - 2.75], [cx + 4.25, cy + 0.75], [cx - 2.75, cy + 4.25]])), 0.5)
        s.own(0, 0, 0, s.add(cell(0, 0)), 0.25)  # (a second, ordinary point: the depth range has two distinct covered values and the uncovered one)
    c = s.finish(name, _pow2(H) and _pow2(W))
    c["centre"] = (cy * W + cx)
    return c


def _edge_triangle(cx, cy, a, b, d, mirror):
    """A triangle whose edge a -> b (offsets from the pixel centre, pair direction first) is the one a pair leaves it through; the third
    vertex lies far on the other side, a quarter pixel off the pair's line.  ``d``: 1 transposes; ``mirror``: reflected in the pair
    direction (the triangle then belongs to the pair's SECOND pixel)."""
    pts = np.array([a, b, [-6.0, 0.25]])
    if mirror:
        pts[:, 0] = -pts[:, 0]
    if d:
        pts = pts[:, ::-1]
    return pts + np.array([cx + 0.5, cy + 0.5])


def clamp_window(name, H, W):
    """Vertical (pair-perpendicular) edges crossing at dc = -3/32, -1/32, 0, 1, 33/32, 35/32 from the owning pixel's centre, for both
    directions and for the triangle on either pixel of the pair: -1/32 and 33/32 are CLAMPED records (flag bit 4, alpha +-1/2, no
    position gradient), 0 and 1 exactly are records that are not clamped, -3/32 and 35/32 are outside the window."""
    s = Scene(1, H, W)
    expect = {}
    for i, dc in enumerate((-3 / 32, -1 / 32, 0.0, 1.0, 33 / 32, 35 / 32)):
        for j, (d, mirror) in enumerate(((0, False), (0, True), (1, False), (1, True))):
            x, y = 3 + 7 * j, 3 + 5 * i  # (24 sites on a grid 7 columns and 5 rows apart: none adjacent to another)
            t = s.add(_edge_triangle(x, y, [dc, -2.0], [dc, 2.0], d, mirror))
            s.own(0, y, x, t)
            pix0 = y * W + x - ((1 if d == 0 else W) if mirror else 0)
            expect[(pix0, d)] = None if dc in (-3 / 32, 35 / 32) else bool(dc in (-1 / 32, 33 / 32))
    return s.finish(name, True, expect=expect)


def slope_45(name, H, W):
    """Edges through a pair at |dy| == |dx| exactly (accepted) and one lattice step (1/32 over a run of 2) shallower (refused) and steeper
    (accepted), rising and falling, both directions, the triangle on either pixel."""
    s = Scene(1, H, W)
    expect = {}
    n = 0
    for step, want in ((0.0, True), (1 / 32, False), (-1 / 32, True)):
        for sign in (1.0, -1.0):
            for d, mirror in ((0, False), (0, True), (1, False), (1, True)):
                x, y = 3 + 7 * (n % 4), 3 + 5 * (n // 4)  # (24 sites, none adjacent to another)
                n += 1
                half = 1.0 + step
                t = s.add(_edge_triangle(x, y, [0.25 - sign * half, -1.0], [0.25 + sign * half, 1.0], d, mirror))
                s.own(0, y, x, t)
                expect[(y * W + x - ((1 if d == 0 else W) if mirror else 0), d)] = False if want else None
    return s.finish(name, True, expect=expect)


def topology(name, H, W):
    """Shared edges: the pair to the right of each site leaves its triangle through the vertical edge A-B at dc = 1/4.
      boundary   no neighbour across A-B                                        record
      interior   the neighbour's third vertex on the other side                 no record
      fold       the neighbour's third vertex on the same side                  record
      online+/-  the neighbour's third vertex exactly ON the line A-B (w is +0: the sign bit decides), in both windings of the own
                 triangle                                                        record / no record (whichever the sign rule says)
      fan        three triangles on A-B (non-manifold): the table's rule picks the neighbour
    """
    s = Scene(1, H, W)
    expect = {}
    sites = (("boundary", []), ("interior", ["R"]), ("fold", ["L2"]), ("online+", ["O"]), ("online-", ["O"]), ("fan", ["R", "L2"]))
    for i, (kind, others) in enumerate(sites):
        x, y = 4 + 14 * (i % 2), 3 + 5 * (i // 2)  # (32 x 16 frame: sites 14 columns and 5 rows apart)
        cx, cy = x + 0.5, y + 0.5
        A_, B_, L = [cx + 0.25, cy - 2.0], [cx + 0.25, cy + 2.0], [cx - 4.0, cy + 0.25]
        third = dict(R=[cx + 5.0, cy + 0.25], L2=[cx - 3.0, cy + 0.75], O=[cx + 0.25, cy + 6.0])
        own = s.add([B_, A_, L] if kind == "online-" else [A_, B_, L])
        va, vb = (s.tri[own][1], s.tri[own][0]) if kind == "online-" else (s.tri[own][0], s.tri[own][1])
        s.own(0, y, x, own, 0.125)
        for k, o in enumerate(others):
            t = s.add([B_, A_, third[o]], share=(vb, va, None)) if kind != "online-" else s.add([A_, B_, third[o]], share=(va, vb, None))
            if o == "R":
                s.own(0, y, x + 1, t, 0.5)  # the neighbour covers the pair's second pixel, farther away
        expect[(y * W + x, 0)] = {"boundary": False, "interior": None, "fold": False}.get(kind, "any")
    return s.finish(name, True, expect=expect)


def rasterised(name, H, W, seed):
    """B = 2: two perturbed, overlapping height-field patches with perspective w through the oracle's rasteriser: not on the lattice, the
    frame no power of two -- the ordinary statistics."""
    from oracle import raster_ref

    rng = np.random.default_rng(seed)
    vs, ts, base = [], [], 0
    for n, lo, hi, z in ((6, -0.85, 0.6, 0.3), (5, -0.3, 0.9, -0.2)):
        g = np.linspace(lo, hi, n)
        xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
        idx = lambda i, j: base + i * n + j
        ts += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i in range(n - 1) for j in range(n - 1)]
        ts += [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(n - 1) for j in range(n - 1)]
        vs.append(np.concatenate([xy, np.full((n * n, 1), z)], 1))
        base += n * n
    v = np.concatenate(vs, 0)
    v = v[None] + rng.uniform(-0.08, 0.08, (2,) + v.shape)
    w = rng.uniform(0.7, 1.4, (2, v.shape[1], 1))
    clip = torch.from_numpy(np.concatenate([v * w, w], -1)).float().contiguous()
    tri = torch.tensor(ts, dtype=torch.long)
    rast = raster_ref.rasterize(clip, tri.int(), (H, W))
    return dict(name=name, rast=rast, clip=clip, tri=tri, B=2, H=H, W=W, lattice=False, expect={})


# name -> (builder, keyword arguments); the comment names the site in csrc/antialias.hip the case is there for
CASES = {
    # aa_analyze_body: 480 candidates in ONE work-group -- both trips of the c0 loop over the LDS pool, the second one ragged (224 of its
    # 256 lanes: wave 3 half filled, no wave leaves)
    "checker_16x16": (checker, {}),
    # 302 candidates in one work-group: the second trip holds 46, so waves 1..3 leave through the whole-wave break in front of
    # aa_append's ballot while wave 0 appends
    "partial_16x16": (checker, dict(rows=10)),
    # s_cand[512] exactly full: the work-groups of rows 0 and 1 hold 512 candidates (511 at the row's end); row 2 right pairs only;
    # W > 256: the lower neighbour lives in another work-group
    "checker_3x512": (checker, {}),
    # both pixels of every pair covered, depths from {0, 1/8, 2/8, 3/8}: exact ties, the depth rule (z0 < z1, else the second) decides
    "every_3x512": (checker, dict(every=True, seed=3)),
    # narrow and ragged frames: W = 1, H = 1, H W < 256, = 255 / 256 / 257; nb_an = 1 or 2 (riding: the odd-grid exit j >= total)
    "narrow_1x1": (checker, {}),
    "narrow_1x257": (checker, {}),
    "narrow_300x1": (checker, {}),
    "ragged_5x7": (checker, {}),
    "ragged_17x15": (checker, {}),
    # clip_batch == 1 with B > 1 (g_clip [1,V,4] summed over images) against a per-image clip; an image without a covered pixel, an image
    # without a candidate pair; nb_an = 3 (odd) work-groups riding next to two buffers
    "batch3_shared_17x15": (batch3, dict(shared=True)),
    "batch3_own_17x15": (batch3, dict(shared=False)),
    # a destination pixel that takes four blends (atomics of four records on one pixel)
    "four_blends_8x8": (four, dict(roles=False)),
    # a point in all four roles of g_slots (first / second pixel of a right / lower pair)
    "four_roles_8x8": (four, dict(roles=True)),
    # dc in (-1/16, 0) and (1, 17/16): flag bit 4, alpha +-1/2, no position gradient; just outside the window; exactly 0 and 1
    "clamp_window_32x32": (clamp_window, {}),
    # |dy| == |dx| is accepted; one step shallower is not
    "slope_45_32x32": (slope_45, {}),
    # the opposite-vertex rule: boundary, interior, fold, opposite vertex exactly on the edge line (w == +-0, the sign bit), non-manifold fan
    "topology_16x32": (topology, {}),
    # w from {1/4, 1/2, 2, 4} per vertex and one vertex with w < 0: the w-gradient of aa_edge_adjoint
    "perspective_16x16": (checker, dict(seed=5, w_choices=(0.25, 0.5, 2.0, 4.0), negative_w=(5, 1, -2.0))),
    # ordinary statistics off the lattice
    "rasterised_24x40": (rasterised, dict(seed=5)),
    # frames that divide by 2 and 3, for the supersampled compositor
    "checker_12x12": (checker, {}),
    "four_roles_12x12": (four, dict(roles=True)),
    "batch3_shared_18x12": (batch3, dict(shared=True)),
}
RIDING = tuple(CASES)  # every case also runs through the riding analysis (one buffer, two buffers, mask)


@functools.lru_cache(maxsize=None)
def build(name):
    fn, kw = CASES[name]
    H, W = _size(name)
    return fn(name, H, W, **kw)


@functools.lru_cache(maxsize=None)
def decided(name, dtype=A.F32):
    c = build(name)
    return A.decide(c["rast"], c["clip"], c["tri"], dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------- runs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _grad(shape, kind, g):
    """An upstream gradient [B,H,W,K]: 'random'; 'channels' (channel 0, the last and every fifth all zero); 'pixels' (the pixels with
    x % 3 == 0 and a whole band of rows all zero); 'third' (every third element zero); 'alpha' (only the last channel: what is left when
    only the alpha channel of an image goes on)."""
    t = torch.randn(shape, generator=g)
    if kind == "channels":
        t[..., 0] = 0
        t[..., -1] = 0
        t[..., ::5] = 0
    elif kind == "pixels":
        t[:, :, ::3] = 0
        t[:, shape[1] // 3:shape[1] // 2] = 0
    elif kind == "third":
        t.view(-1)[::3] = 0
    elif kind == "alpha":
        t[..., :-1] = 0
    else:
        assert kind == "random", kind
    return t


def _background(kind, B, H, W, C1, g):
    """none | 'shared' [1,H,W,C1] | 'own' [B,H,W,C1] | 'short' [1,H,W,max(C1 - 1, 1) or 3]: fewer channels than the image."""
    if kind == "none":
        return None
    if kind == "short":
        return torch.randn((1, H, W, max(1, min(3, C1 - 1))), generator=g)
    return torch.randn((1 if kind == "shared" else B, H, W, C1), generator=g)


def spec(case, form, C=3, keep=None, bg="none", grad="random", equal=False, pad=0, s=None, shared_w2c=True):
    return dict(case=case, form=form, C=C, keep=keep, bg=bg, grad=grad, equal=equal, pad=pad, s=s, shared_w2c=shared_w2c)


def make_buffer(run, i, sp):
    """The aa_ref.Buffer of buffer ``i`` of run ``run`` (seeded by both): float32 CPU tensors, rows in ascending pixel order."""
    c = build(sp["case"])
    B, H, W, rast = c["B"], c["H"], c["W"], c["rast"]
    g = _gen(f"{run}#{i}")
    C, form = sp["C"], sp["form"]
    if form == "dense":
        color = torch.randn((B, H, W, C), generator=g)
        if sp["equal"]:  # equal colours across the right pairs of the even rows and the lower pairs of the even columns' first rows
            color[:, ::2, 1::2] = color[:, ::2, 0:-1:2] if W % 2 == 0 else color[:, ::2, 1::2]
        return A.Buffer("dense", _grad((B, H, W, C), sp["grad"], g), color=color)
    if form == "mask":
        return A.Buffer("mask", _grad((B, H, W, C + 1), sp["grad"], g), C=C, bg=_background(sp["bg"], B, H, W, C + 1, g))
    if form == "depth":
        P = int((rast[..., 3] > 0).sum())
        w2c = torch.randn((1 if sp["shared_w2c"] else B, 4, 4), generator=g)
        return A.Buffer("depth", _grad((B, H, W, 1), sp["grad"], g), gb=torch.randn((P, 3), generator=g), w2c=w2c)
    K = C + 1 if sp["keep"] is None else sp["keep"]
    if form == "msaa":
        s = sp["s"]
        h, w = H // s, W // s
        P = int((rast[:, ::s, ::s, 3] > 0).sum())
        return A.Buffer("msaa", _grad((B, h, w, K), sp["grad"], g), vals=torch.randn((P + sp["pad"], C), generator=g), null=torch.randn((B, C), generator=g),
                        bg=_background(sp["bg"], B, h, w, C + 1, g), s=s, keep=sp["keep"])
    assert form == "rows", form
    pix = A.covered_list(rast)
    vals = torch.randn((pix.shape[0] + sp["pad"], C), generator=g)
    bg = _background(sp["bg"], B, H, W, C + 1, g)
    if sp["equal"] and bg is not None and bg.shape[0] == B and bg.shape[3] == C + 1:
        # equal colours across a pair: the uncovered right neighbour of every second covered pixel holds that pixel's [vals, 1]
        for r in range(0, pix.shape[0], 2):
            p = int(pix[r])
            if (p + 1) % W and not bool(rast.reshape(-1, 4)[p + 1, 3] > 0):
                bg.view(-1, C + 1)[p + 1] = torch.cat([vals[r], torch.ones(1)])
    return A.Buffer("rows", _grad((B, H, W, K), sp["grad"], g), vals=vals, bg=bg, keep=sp["keep"])


def _runs():
    runs = {}
    for case in CASES:
        if case in ("checker_12x12", "four_roles_12x12", "batch3_shared_18x12"):
            continue
        runs[f"{case}:dense"] = [spec(case, "dense")]
        runs[f"{case}:rows"] = [spec(case, "rows", bg="own", pad=3)]
        runs[f"{case}:rows2"] = [spec(case, "rows", bg="short"), spec(case, "rows", C=16, keep=16, pad=5)]
        runs[f"{case}:mask"] = [spec(case, "mask", bg="shared")]
    # channel counts around the 32-lane channel loop of the backward kernels, keep in {None, 1, C}, every background form, gradients with
    # whole channels / whole pixels / every third element zero, equal colours across pairs
    k = "checker_16x16"
    for C, keep, bg, grad, equal in ((1, None, "none", "random", False), (1, 1, "own", "third", False), (4, None, "shared", "channels", False),
                                     (4, 4, "own", "random", True), (16, 1, "short", "pixels", False), (17, None, "own", "third", True),
                                     (17, 17, "none", "channels", False), (33, 33, "shared", "pixels", False), (33, None, "short", "random", False),
                                     (64, 64, "own", "third", True), (64, 1, "none", "random", False), (64, None, "shared", "channels", False)):
        runs[f"{k}:rows_C{C}_keep{keep}_{bg}_{grad}{'_equal' if equal else ''}"] = [spec(k, "rows", C=C, keep=keep, bg=bg, grad=grad, equal=equal, pad=2)]
    for C, grad, equal in ((1, "third", False), (4, "channels", True), (16, "pixels", False), (17, "random", True), (33, "channels", False), (64, "third", True)):
        runs[f"{k}:dense_C{C}_{grad}{'_equal' if equal else ''}"] = [spec(k, "dense", C=C, grad=grad, equal=equal)]
    for C, bg, grad in ((1, "none", "random"), (1, "own", "pixels"), (3, "own", "third"), (3, "none", "alpha"), (16, "shared", "channels")):
        runs[f"{k}:mask_C{C}_{bg}_{grad}"] = [spec(k, "mask", C=C, bg=bg, grad=grad)]
    runs["four_roles_8x8:rows_C1"] = [spec("four_roles_8x8", "rows", C=1, keep=1)]  # (the value rows of a depth call: what g_slots stands for)
    for case in ("four_roles_8x8", "checker_16x16", "batch3_shared_17x15"):
        runs[f"{case}:depth"] = [spec(case, "depth", C=1)]
        runs[f"{case}:depth2"] = [spec(case, "depth", C=1, shared_w2c=False, grad="third"), spec(case, "rows", C=16, keep=16, bg="short", pad=5)]
    for case in ("four_roles_12x12", "checker_12x12", "batch3_shared_18x12"):
        runs[f"{case}:dense"] = [spec(case, "dense")]
        for s in (2, 3):
            # (wide buffers: g_null has B C elements and each is a sum over every uncovered-sample block and record of its image -- with
            # a handful of live elements its largest error is one draw of the summation order, in the restatement and in the kernels alike)
            runs[f"{case}:msaa{s}"] = [spec(case, "msaa", C=33, s=s, bg="own", pad=3)]
            runs[f"{case}:msaa{s}_2"] = [spec(case, "msaa", C=17, s=s, bg="short", keep=17, grad="third"), spec(case, "msaa", C=64, s=s, keep=64, pad=4)]
    return runs


RUNS = _runs()


@functools.lru_cache(maxsize=None)
def buffers(run):
    return tuple(make_buffer(run, i, sp) for i, sp in enumerate(RUNS[run]))


def run_case(run):
    return RUNS[run][0]["case"]


def keys(run):
    """The quantities of a run, in the order of aa_ref.evaluate's names."""
    out = ["g_clip"]
    for i, b in enumerate(buffers(run)):
        out += [f"out{i}"] + [f"g_{n}{i}" for n in b.leaves]
    return out


@functools.lru_cache(maxsize=None)
def reference(run):
    """(float64 reference: name -> (value, magnitude), float32 restatement: name -> value) of a run, given the float32 decisions: computed
    once, shared, never modified."""
    c = build(run_case(run))
    d = decided(run_case(run))
    torch.set_num_threads(1)
    return A.evaluate(c, d["rec"], d["alpha"], buffers(run)), A.evaluate(c, d["rec"], d["alpha"], buffers(run), dtype=A.F32)
