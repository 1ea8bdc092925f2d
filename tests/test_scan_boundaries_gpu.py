"""Boundary cases of the work-group scans and cross-lane sums (csrc/a3d_common.h: a3d_block_excl_scan, a3d_wave_incl_scan,
a3d_row16_incl_scan, a3d_group_sum), through the public ops only, at the smallest inputs that put

  (a) non-zero counts into only a part of wave 0,
  (b) a non-zero count into lane 63 of one wave and into lane 0 of the next,
  (c) a partly filled last wave -- and, once per site, nothing but zeros

in front of every scan a test can steer.  Expected values come from torch on the CPU and from oracle/; every comparison is exact
(integers; float32 results of the same operations in the same order).  The large shapes are the business of tests/test_gpu_parity.py.

Run on the MI355X box:  python -m pytest tests/test_scan_boundaries_gpu.py -m gpu -q
"""
import importlib

import numpy as np
import pytest
import torch

from conftest import kuhn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("3danimals_amd.ops")


# ------------------------------------------------------------------------------------------------ vertex -> face lists
def expected_lists(tri, V):
    """(off int32 [V+1], adj int32 [3F]) of a triangle list: vertex v's entries are the keys corner * F + face in ascending order."""
    F = tri.shape[0]
    v = tri.long().t().reshape(-1)  # entry corner * F + face
    counts = torch.bincount(v, minlength=V)
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0)])
    return off.int(), torch.argsort(v, stable=True).int()


def hand_made_triangles(V, pattern):
    """Triangle lists with non-uniform valence, F <= 3 V.  The scan of the valences (nr_adj_scan_kernel) runs 1024 threads, each over
    per = ceil(V / 1024) consecutive vertices: 'low' uses the first few vertices only (a part of wave 0), 'seam' the vertices of lane 63
    of every wave and of lane 0 of the next, the last vertex and vertex 0 -- the first of each seam three times as often."""
    per = -(-V // 1024)
    if pattern == "none":
        return torch.zeros((0, 3), dtype=torch.int32)
    if pattern == "low":
        pool = torch.arange(min(V, 5))
    else:
        seams = [w * 64 * per + d for w in range(1, 16) for d in (-1, -1, -1, 0)]
        pool = torch.tensor([v for v in [0] + seams + [V - 2, V - 1, V - 1] if 0 <= v < V])
    g = torch.Generator().manual_seed(V)
    F = min(3 * V, 2 * pool.numel() + 1)
    return pool[torch.randint(0, pool.numel(), (F, 3), generator=g)].int().contiguous()


@pytest.mark.parametrize("pattern", ["none", "low", "seam"])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_vertex_face_adjacency_offsets(V, pattern, dev, ops):
    """Site: topo_common.h nr_adj_scan_kernel (a3d_block_excl_scan<16> over 1024 threads), through ops.vertex_face_adjacency ->
    a3d_mesh_topology.  V = 1, 63: a part of wave 0; 64, 65, 1025, 4097 ('seam'): lane 63 / lane 0 of the next wave, last wave partly
    filled (4097: five vertices per thread); 'none': every count zero.  Offsets against cumsum(bincount), lists against a stable sort."""
    tri = hand_made_triangles(V, pattern)
    adj = ops.vertex_face_adjacency(tri.to(dev), V)
    off, lists = expected_lists(tri, V)
    assert adj.stride == 0 and torch.equal(adj.off.cpu(), off)
    assert torch.equal(adj.adj.cpu()[:3 * tri.shape[0]], lists)


def strip_mesh(F):
    """F triangles of a two-row strip (an open manifold: boundary edges all around)."""
    n = F // 2 + 2
    i = torch.arange(n - 1)
    quads = torch.stack([torch.stack([i, i + 1, i + n], 1), torch.stack([i + 1, i + n + 1, i + n], 1)], 1).reshape(-1, 3)
    return quads[:F].int().contiguous(), 2 * n


@pytest.mark.parametrize("F", [1, 85, 86, 171])
def test_mesh_and_aa_topology_across_a_work_group(F, dev, ops):
    """Sites: nr_adj_scan_kernel again and a3d_sort8 (tp_sort_rearm_kernel), through ops.mesh_topology; the edge hash through
    ops.aa_topology / ops.AATopology.  The corner-parallel launches of topology.hip take 256 corners per work-group: 3 F = 255, 258
    (and 513) straddle one (two).  Lists against the stable sort, opposite vertices against oracle.raster_ref.edge_opposites."""
    from oracle import raster_ref

    tri, V = strip_mesh(F)
    off, lists = expected_lists(tri, V)
    opp = raster_ref.edge_opposites(tri.numpy())
    adj, topo = ops.mesh_topology(tri.to(dev), V)
    assert torch.equal(adj.off.cpu(), off) and torch.equal(adj.adj.cpu()[:3 * F], lists)
    assert np.array_equal(topo.opp.cpu().numpy(), opp)
    assert np.array_equal(ops.aa_topology(tri.to(dev), V).opp.cpu().numpy(), opp)
    assert np.array_equal(ops.AATopology(tri.to(dev), V).opp.cpu().numpy(), opp)
    assert np.array_equal(ops.opposite_vertices_from_lists(adj).cpu().numpy(), opp)


# ------------------------------------------------------------------------------------------------ covered-pixel list
def tile_order(B, H, W):
    """flat pixel indices in the list's order: image-major, 8x8 tiles row by row, row-major inside a tile"""
    return torch.arange(B * H * W).reshape(B, H // 8, 8, W // 8, 8).permute(0, 1, 3, 2, 4).reshape(-1)


@pytest.mark.parametrize("shape,which", [((1, 8, 8), "none"), ((1, 8, 8), "all"), ((1, 8, 8), [63]), ((2, 24, 40), "none"), ((2, 24, 40), "all"),
                                         ((2, 24, 40), [63, 64]), ((2, 24, 40), [255, 256, 1919]), ((1, 136, 128), [0, 16383, 16384, 17407]),
                                         ((1, 136, 128), "all")])
def test_covered_pixels_of_hand_made_buffers(shape, which, dev, ops):
    """Sites: cover_common.h cv_block_offset_wave0 (a3d_group_sum over the block counts and group sums) and the ballots of cover.hip,
    through ops.covered_pixels.  Nothing covered; everything; the last pixel of one 64-pixel wave and the first of the next; the same
    across a 256-pixel block and, at 136 x 128, across a group of 64 blocks (pixel 16384 of the list's order), last block partly
    covered.  Against torch.nonzero in the list's order."""
    B, H, W = shape
    order = tile_order(B, H, W)
    mask = torch.zeros(B * H * W, dtype=torch.bool)
    if which == "all":
        mask[:] = True
    elif which != "none":
        mask[order[torch.tensor(which)]] = True
    rast = torch.zeros(B, H, W, 4)
    rast[..., 3] = mask.reshape(B, H, W).float() * 7.0
    want = order[torch.nonzero(mask[order])[:, 0]]
    want_inv = torch.full((B * H * W,), -1, dtype=torch.int32)
    want_inv[want] = torch.arange(want.numel(), dtype=torch.int32)
    pix, inv = ops.covered_pixels(rast.to(dev), return_inverse=True)
    assert pix.dtype == torch.int64 and torch.equal(pix.cpu(), want)
    assert torch.equal(inv.cpu(), want_inv)
    assert torch.equal(ops.covered_pixels(rast.to(dev)).cpu(), want)


# ------------------------------------------------------------------------------------------------ rasteriser
@pytest.mark.parametrize("n_small,n_big", [(3, 0), (65, 3), (300, 65), (0, 256)])
def test_rasterize_candidate_and_tile_scans(n_small, n_big, dev, ops):
    """Site: raster.hip rs_tri_kernel (the prefix of a wave's box sizes that pools the candidate pixels, and the tile counts of a
    work-group's big boxes: a3d_block_excl_scan<4>).  64 x 64 frame; ``n_small`` triangles stacked inside one 8x8 tile at different
    depths -- 3 (a part of one wave's slice), 65 (one more than the 64 of a work-group) or 300 (several work-groups) -- and ``n_big``
    triangles whose boxes span most of the frame (above 512 pixels: the tile stage; none, a few beside small ones, and work-groups
    that hold nothing else).  Bit-exact against oracle/raster_ref.c."""
    from oracle import raster_ref

    H = W = 64
    g = torch.Generator().manual_seed(1000 * n_small + n_big)
    n = n_small + n_big
    small = torch.tensor([0.375, -0.125]) + 0.2 * (torch.rand(n_small, 3, 2, generator=g) - 0.5)  # about the tile at x 40..47, y 24..31
    big = torch.rand(n_big, 3, 2, generator=g) * 2.6 - 1.3
    xy = torch.cat([small, big], 0)
    z = torch.rand(n, 3, 1, generator=g) * 1.6 - 0.8
    w = 0.5 + torch.rand(n, 3, 1, generator=g)
    clip = torch.cat([xy * w, z * w, w], -1).reshape(1, 3 * n, 4).contiguous()
    tri = torch.arange(3 * n, dtype=torch.int32).reshape(n, 3)[torch.randperm(n, generator=g)].contiguous()
    ref = raster_ref.rasterize(clip, tri, (H, W))
    out = ops.rasterize(clip.to(dev), tri.to(dev), (H, W)).cpu()
    assert np.array_equal(out[..., 3].numpy(), ref[..., 3].numpy())
    assert np.array_equal(out.numpy(), ref.numpy())
    assert float((ref[..., 3] > 0).float().sum()) > 0


# ------------------------------------------------------------------------------------------------ DMTet
def dmtet_field(kind, res, pos):
    n = res + 1
    if kind == "empty":
        return -torch.ones(pos.shape[0])
    if kind == "sphere":
        return 0.3 * 7.0 - pos.norm(dim=1)
    # sign noise: the sign alternates with the parity of i + j + k -- every Kuhn tet walks 000 -> 111 one axis at a time, so every tet
    # (and every edge along an axis) crosses -- under a random magnitude
    idx = torch.arange(pos.shape[0])
    parity = (idx // (n * n) + (idx // n) % n + idx % n) % 2
    return (1.0 - 2.0 * parity) * (0.1 + torch.rand(pos.shape[0], generator=torch.Generator().manual_seed(res)))


@pytest.mark.parametrize("kind", ["empty", "sphere", "noise"])
@pytest.mark.parametrize("res,which", [(r, w) for r in (2, 3, 4, 7) for w in ("plain", "culled", "ordered")] + [(22, "plain")])
def test_dmtet_count_and_extraction(res, which, kind, dev, ops, monkeypatch):
    """Sites, all in dmtet.hip: dm_scan_kernel (the block sums: a3d_block_excl_scan<16>; the chunk counts of the vertex plane:
    a3d_group_sum<8> + a3d_block_excl_scan<16>; after the ordered count pass the words of a block: a3d_row16_incl_scan), dm_emit_kernel /
    dm_emit_words_kernel (the crossings of a work-group's 256 words: a3d_block_excl_scan<4> with the total) and
    dm_surface_vertices_chunk (the 32 words of a vertex chunk: a3d_wave_incl_scan).  Kuhn grids of 2, 3, 4 cells: one block of sums, a
    part of wave 0 everywhere; 22 cells (78 edge blocks, 1.2e3 edge words, 12 vertex chunks): block sums in lane 63 and in lane 0 of
    the next wave, a partly filled last work-group of words; plain pass only.  'empty': every count zero; 'noise': every tet crosses.
    The three count passes (taken for certain from 7 cells on); counts, vertices, faces, uv indices and the surface-vertex list against oracle.dmtet_ref, bit for bit.
    (Not reachable at these sizes: the unstaged scans of dm_scan_kernel, which take over above 24576 block sums.)"""
    from oracle import dmtet_ref

    T = importlib.import_module("3danimals_amd.model.geometry.dmtet").TetGridTopology
    pos, tets = kuhn(res)
    sdf = dmtet_field(kind, res, pos)
    monkeypatch.setattr(ops, "DMTET_CULL_MIN_VERTS", 0 if which != "plain" else 1 << 30)
    topo = T(tets.to(dev), positions=pos.to(dev))
    if which == "ordered":
        topo.WORD_GROUPS = False
    ref = dmtet_ref.topology(sdf.numpy(), tets.numpy())
    rv, rf, _, ru = dmtet_ref.marching_tets(pos, sdf, tets)
    occ = (sdf > 0)[tets]
    ntri = dmtet_ref.NUM_TRIANGLES[(occ.long() * (1 << torch.arange(4))).sum(-1).numpy()]
    surf = np.unique(ref["interp_v"].reshape(-1))
    want = [ref["interp_v"].shape[0], int((ntri == 1).sum()), int((ntri == 2).sum()), surf.shape[0]]
    counts = ops.dmtet_count_only(pos.to(dev), sdf.to(dev), topo, surface_vertices=True).cpu().tolist()
    assert res < 7 or topo._last_count_pass == which  # (a grid of a few cells is too small for the tables and picks another pass itself)
    assert counts[:4] == want
    v, f, u, ve, idx = ops.dmtet_extract(pos.to(dev), sdf.to(dev), topo, surface_vertices=True)
    assert np.array_equal(f.cpu().numpy(), rf.numpy()) and np.array_equal(u.cpu().numpy(), ru.numpy())
    assert np.array_equal(v.cpu().numpy(), rv.numpy())
    e = tets.numpy()[:, dmtet_ref.EDGE_SLOTS].reshape(-1, 2)  # the grid's edges in lexicographic order: a vertex names its edge's row
    all_edges = np.unique(e.min(1) * pos.shape[0] + e.max(1))
    assert np.array_equal(ve.cpu().numpy(), np.searchsorted(all_edges, ref["interp_v"][:, 0] * pos.shape[0] + ref["interp_v"][:, 1]))
    assert np.array_equal(idx.cpu().numpy(), surf)


@pytest.mark.parametrize("kind", ["sphere", "noise"])
@pytest.mark.parametrize("res", [2, 3, 4, 22])
def test_dmtet_topology_finalize_scan(res, kind, dev, ops, monkeypatch):
    """Site: topology.hip tp_finalize_kernel (every work-group scans the V valences: a3d_block_excl_scan<4> over 256 threads), reached
    when the emit launch only counts the valences (ops.DMTET_EMIT_LISTS off).  The small grids: a part of wave 0 up to a few vertices per thread; 22 cells: thousands of surface vertices, dozens per thread.  Offsets against cumsum(bincount), every
    list as a set against the stable sort (this path leaves the lists unsorted)."""
    T = importlib.import_module("3danimals_amd.model.geometry.dmtet").TetGridTopology
    pos, tets = kuhn(res)
    sdf = dmtet_field(kind, res, pos)
    monkeypatch.setattr(ops, "DMTET_EMIT_LISTS", False)
    v, f, _, _ = ops.dmtet_extract(pos.to(dev), sdf.to(dev), T(tets.to(dev)))
    V, F = v.shape[0], f.shape[0]
    assert V > 0 and F > 0
    adj = ops.vertex_face_adjacency(ops.tri_int32(f), V)
    assert adj.stride == 0 and not adj.sorted  # (the lists of a3d_mesh_topology_finalize)
    off, lists = expected_lists(f.cpu(), V)
    assert torch.equal(adj.off.cpu(), off)
    got = adj.adj.cpu()[:3 * F]
    owner = torch.repeat_interleave(torch.arange(V), (off[1:] - off[:-1]).long())
    assert torch.equal(got[torch.argsort(owner * (3 * F) + got.long(), stable=True)], lists)


# ------------------------------------------------------------------------------------------------ antialiasing
AA_ROWS = {"none": None, "few": [0, 1, 5], "seam": [63, 64], "last": [255], "seams": [63, 64, 127, 128, 191, 192, 255], "all": list(range(256))}


def silhouette_scene(rows, H=256, W=256):
    """(clip [1,3n,4], tri [n,3]): one small triangle per listed row r of a 256 x 256 frame, at column 8 + 5 r mod 240, covering the one
    pixel centre (column, r): corners (0.5625, -0.25), (-0.25, 1.25), (1.25, 1.25) from the pixel's corner, w = 1.  Its three silhouette
    records -- the pairs with the left, the right and the lower neighbour; the two steep edges give the pair with the upper neighbour
    none -- all start in row r, and a row of this frame is one analysis work-group, i.e. one segment of the work list.  Every number
    is a multiple of 1/32 (crossing distances 0.34375, 0.40625, 0.75), so with integer colours every blend is exact in float32 and no
    sum depends on its order.  ``rows`` None: one triangle over the whole frame -- covered everywhere, no silhouette pair."""
    if rows is None:
        xy = torch.tensor([[[-4.0, -2.0], [4.0, -2.0], [0.0, 6.0]]])
    else:
        corner = torch.tensor([[8.0 + (5 * r) % 240, float(r)] for r in rows])
        xy = (corner[:, None] + torch.tensor([[0.5625, -0.25], [-0.25, 1.25], [1.25, 1.25]])) / torch.tensor([W / 2.0, H / 2.0]) - 1.0
    n = xy.shape[0]
    clip = torch.cat([xy, torch.zeros(n, 3, 1), torch.ones(n, 3, 1)], -1).reshape(1, 3 * n, 4).contiguous()
    return clip, torch.arange(3 * n, dtype=torch.int32).reshape(n, 3)


@pytest.mark.parametrize("case", list(AA_ROWS))
def test_antialias_segment_offsets(case, dev, ops):
    """Site: antialias.hip aa_segment_offsets (a3d_block_excl_scan<4> over the 256 segment fills), called by aa_fwd_kernel /
    aa_bwd_kernel (ops.antialias) and ca_blend_kernel / ca_bwd_kernel (ops.composite_antialias).  Segments filled: none; 0, 1 and 5 (a
    part of wave 0); 63 and 64 (lane 63 and lane 0 of the next wave); 255 alone (the last lane of the last wave); every wave seam; all
    256.  Images and colour gradients against oracle.raster_ref.antialias, bit for bit (see silhouette_scene for why that holds)."""
    from oracle import raster_ref

    H = W = 256
    rows = AA_ROWS[case]
    clip, tri = silhouette_scene(rows)
    rast = raster_ref.rasterize(clip, tri, (H, W))
    covered = rast[0, ..., 3] > 0
    g = torch.Generator().manual_seed(len(case))
    ramp = (torch.arange(W)[None, :] + W * torch.arange(H)[:, None]).float()  # channel 0: every pixel its own value
    color = torch.cat([ramp[None, ..., None], torch.randint(0, 8, (1, H, W, 2), generator=g).float()], -1)
    wgt = torch.randint(-4, 5, (1, H, W, 4), generator=g).float()
    color_c = color.clone().requires_grad_(True)
    ref = raster_ref.antialias(color_c, rast, clip, tri)
    (g_ref,) = torch.autograd.grad((ref * wgt[..., :3]).sum(), color_c)
    # the scene is what the docstring says: one covered pixel per row, blended pixels = that one and the one below it
    want = torch.zeros(H, W, dtype=torch.bool)
    for r in rows or []:
        want[r:r + 2, 8 + (5 * r) % 240] = True
    assert torch.equal(ref.detach()[0, ..., 0] != ramp, want)
    assert bool(covered.all()) if rows is None else torch.equal(torch.nonzero(covered)[:, 0], torch.tensor(rows))
    rast_d, clip_d, tri_d = rast.to(dev), clip.to(dev), tri.to(dev)
    color_d = color.to(dev).requires_grad_(True)
    out = ops.antialias(color_d, rast_d, clip_d, tri_d)
    (g_out,) = torch.autograd.grad((out * wgt[..., :3].to(dev)).sum(), color_d)
    assert torch.equal(out.detach().cpu(), ref.detach()) and torch.equal(g_out.cpu(), g_ref)
    # the compositor's blend over the same records: value rows at the covered pixels over a background, plus the coverage channel
    pix = tile_order(1, H, W)
    pix = pix[torch.nonzero(covered.reshape(-1)[pix])[:, 0]]
    pix_d, inv_d = ops.covered_pixels(rast_d, return_inverse=True)
    assert torch.equal(pix_d.cpu(), pix)
    vals = color.reshape(-1, 3)[pix]
    bg = torch.randint(0, 8, (1, H, W, 3), generator=g).float()
    vals_c = vals.clone().requires_grad_(True)
    comp = torch.cat([bg, torch.zeros(1, H, W, 1)], -1).reshape(-1, 4).index_put((pix,), torch.cat([vals_c, torch.ones(pix.shape[0], 1)], 1)).reshape(1, H, W, 4)
    ref2 = raster_ref.antialias(comp, rast, clip, tri)
    (g_ref2,) = torch.autograd.grad((ref2 * wgt).sum(), vals_c)
    vals_d = vals.to(dev).requires_grad_(True)
    analysis = ops.AAAnalysis(rast_d, clip_d, ops.aa_topology(tri_d, clip.shape[1]))
    out2 = ops.composite_antialias(vals_d, pix_d, inv_d, bg.to(dev), clip_d, analysis)
    (g_out2,) = torch.autograd.grad((out2 * wgt.to(dev)).sum(), vals_d)
    assert torch.equal(out2.detach().cpu(), ref2.detach()) and torch.equal(g_out2.cpu(), g_ref2)
