"""torch.autograd.Function wrappers over the C ABI (include/a3d.h).

Every Function allocates its outputs with torch (so PyTorch's caching allocator owns all device memory),
launches on the current torch stream and returns real gradients for every differentiable input -- DDP runs
with find_unused_parameters=False in the reference.  Nothing here runs on CPU.
"""
from __future__ import annotations

import ctypes
import math
import os
from collections import OrderedDict

import torch

from . import _lib
from ._lib import call, f32c, f32h, ptr, require_device, stream


# ---------------------------------------------------------------------------------------------- index caches
class _IdentityCache:
    """Small LRU keyed by tensor identity (storage pointer, shape, version).

    The keyed tensor is kept alive inside the entry, so its storage cannot be recycled while the entry exists.
    """

    def __init__(self, maxsize=8):
        self.maxsize = maxsize
        self.data = OrderedDict()

    @staticmethod
    def key(t):
        return (t.data_ptr(), tuple(t.shape), t.dtype, t._version)

    def get(self, t, make):
        k = self.key(t)
        hit = self.data.get(k)
        if hit is not None:
            self.data.move_to_end(k)
            return hit[1]
        val = make(t)
        self.data[k] = (t, val)
        while len(self.data) > self.maxsize:
            self.data.popitem(last=False)
        return val

    def put(self, t, val):
        self.data[self.key(t)] = (t, val)
        self.data.move_to_end(self.key(t))
        while len(self.data) > self.maxsize:
            self.data.popitem(last=False)
        return val

    def peek(self, t):
        k = self.key(t)
        hit = self.data.get(k)
        if hit is None:
            return None
        self.data.move_to_end(k)
        return hit[1]

    def take(self, t):
        """peek + remove (None when absent)."""
        hit = self.data.pop(self.key(t), None)
        return None if hit is None else hit[1]


_tri32_cache = _IdentityCache()
_topo_cache = _IdentityCache()


def tri_int32(tri: torch.Tensor) -> torch.Tensor:
    """[F,3] (or [1,F,3]) index tensor -> contiguous int32 [F,3]; converted once per topology and cached
    (the reference converts with .int() at every dr.* call, render.py:182-209,292)."""
    if tri.dim() == 3:
        tri = tri[0]
    if tri.dtype == torch.int32 and tri.is_contiguous():
        return tri
    return _tri32_cache.get(tri, lambda t: t.to(torch.int32).contiguous())


class AATopology:
    """opp[F,3] for one triangle list (nvdiffrast's topology hash), built by a3d_aa_topology."""

    def __init__(self, tri32: torch.Tensor, num_vertices: int, build: bool = True, lists=None):
        """``lists`` (a VertexFaceAdjacency of the same triangle list) instead of the table: a3d_aa_analyze then looks the opposite
        vertices it needs up in the vertex -> face lists (the DMTet extraction's topology builds no hash and no table)."""
        require_device(tri32, what="aa_topology")
        F = tri32.shape[0]
        self.tri, self.lists = tri32, lists
        self.opp = torch.empty((F, 3), dtype=torch.int32, device=tri32.device) if lists is None else None
        if F > 0 and build:
            nbytes = _lib.lib().a3d_aa_hash_bytes(F)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=tri32.device)
            call("a3d_aa_topology", ptr(tri32), F, int(num_vertices), ptr(scratch), ptr(self.opp), stream())


def opposite_vertices_from_lists(adjacency) -> torch.Tensor:
    """opp[F,3] from the vertex -> face lists (a3d_aa_topology_from_lists): the table a3d_aa_topology builds with its hash."""
    tri32 = adjacency.tri
    opp = torch.empty((tri32.shape[0], 3), dtype=torch.int32, device=tri32.device)
    call("a3d_aa_topology_from_lists", ptr(tri32), tri32.shape[0], ptr(adjacency.off), ptr(adjacency.adj), ptr(opp), adjacency.stride, stream())
    return opp


def aa_topology(tri32: torch.Tensor, num_vertices: int) -> AATopology:
    hit = _topo_cache.peek(tri32)
    return hit if hit is not None else mesh_topology(tri32, num_vertices)[1]


_topology_scratch = {}


def mesh_topology(tri32: torch.Tensor, num_vertices: int):
    """(VertexFaceAdjacency, AATopology) of one triangle list, built together by a3d_mesh_topology (5 launches instead of 9) and
    entered into both caches: the normals, the G-buffer backward and the antialiasing of every mesh that shares the list hit them."""
    require_device(tri32, what="mesh_topology")
    F, V = tri32.shape[0], int(num_vertices)
    adj = VertexFaceAdjacency(tri32, V, build=False)
    topo = AATopology(tri32, V, build=False)
    # cursor + hash are kept per (device, stream, hash size): the last launch of a call re-arms them, so only the first use pays the init
    nbytes = _lib.lib().a3d_aa_hash_bytes(max(F, 1))
    key = (tri32.device, stream(), nbytes)
    kept = _topology_scratch.pop(key, None)
    clean = kept is not None and kept[0].shape[0] >= V
    if clean:
        cursor, scratch = kept
    else:
        cursor = torch.zeros(max(V, nbytes // 24), dtype=torch.int32, device=tri32.device)  # zero beyond V too: later calls of this F class may have more vertices (V <= 3F < slots)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=tri32.device)
    call("a3d_mesh_topology", ptr(tri32), V, F, ptr(adj.off), ptr(adj.adj), ptr(cursor), ptr(scratch), ptr(topo.opp), int(clean), stream())
    if len(_topology_scratch) >= 4:
        _topology_scratch.clear()
    if F > 0 or clean:  # only after a completed call whose last launch re-armed it (F == 0 launches nothing that touches the hash: a fresh,
        _topology_scratch[key] = (cursor, scratch)  # never initialised buffer must not be handed to the next call as clean)
    _adj_cache.put(tri32, adj)
    _topo_cache.put(tri32, topo)
    return adj, topo


# ---------------------------------------------------------------------------------------------- DMTet
DMTET_TOPOLOGY = True  # build the mesh topology inside the extraction (emit + one finalize launch) instead of a3d_mesh_topology on first use
_topo_sets = {}


def _topology_sets(dev, F, V):
    """Two alternating valence-count arrays (int32 [vcap], zero) per (device, stream, size class): an extraction's emit launch counts into
    one and its finalize launch zeroes the other, so only the first use of a size class pays an initialisation."""
    vcap = 1 << max(10, int(V - 1).bit_length())
    key = (dev, stream(), vcap)
    st = _topo_sets.get(key)
    if st is None:
        if len(_topo_sets) >= 4:
            _topo_sets.clear()
        st = _topo_sets[key] = dict(sets=[torch.zeros(vcap, dtype=torch.int32, device=dev) for _ in range(2)], cur=0, vcap=vcap, key=key)
    return st


DMTET_CULL_MIN_VERTS = 1 << 17
DMTET_EMIT_LISTS = os.environ.get("A3D_EMIT_LISTS", "1") != "0"  # the emit launch writes the vertex -> face lists itself (no finalize launch)
DMTET_EMIT_LISTS_MAX_STRIDE = 32
DMTET_SPECULATIVE_EMIT = os.environ.get("A3D_SPECULATIVE_EMIT", "1") != "0"  # the emit launch enqueued before the counts read-back (sizes guessed from the last extraction)
_dm_vertex_scratch = {}
_dm_grad_buffers = _IdentityCache(maxsize=2)  # vert_edge of an extraction -> its cleared SDF gradient buffer


def _dmtet_count(sdf_c, pos_c, grid, scratch, counts, vscratch, vclean, counters):
    """The count call of an extraction, by the pass the grid takes (TetGridTopology.count_pass): 'plain' / 'culled' = a3d_dmtet_count
    without / with the word groups of the file's own row order, 'ordered' = a3d_dmtet_count_ordered (any numbering).  -> the pass."""
    Ne, Nt, Nv = grid.edges32.shape[0], grid.tets32.shape[0], sdf_c.shape[0]
    which = grid.count_pass(Nv, pos_c) if hasattr(grid, "count_pass") else "plain"
    n_clear = 0 if counters is None else counters.shape[0]
    if which == "ordered":
        order = grid.spatial_order(pos_c)[0]
        call("a3d_dmtet_count_ordered", ptr(sdf_c), Nv, Ne, Nt, ctypes.addressof(order), ptr(scratch), ptr(counts), ptr(vscratch), int(vclean),
             ptr(counters), n_clear, stream())
    else:
        groups = grid.word_groups() if which == "culled" else None
        call("a3d_dmtet_count", ptr(sdf_c), ptr(grid.edges32), ptr(grid.tets32), Ne, Nt, ptr(scratch), ptr(counts), ptr(vscratch), int(vclean), Nv,
             ptr(groups[0]) if groups else None, ptr(groups[1]) if groups else None, groups[0].shape[1] if groups else 0, ptr(counters), n_clear,
             stream())
    grid._last_count_pass = which
    return which


def dmtet_count_only(pos, sdf, grid, surface_vertices=False):
    """The count call alone (measurement: tools/bench_dmtet.py); -> counts int32 [6] on the device.  With ``surface_vertices`` the flagged
    vertex plane is left dirty (no emit clears it), so every call pays its memset like a first call does."""
    pos_c, sdf_c = f32c(pos.detach()), f32c(sdf.detach()).reshape(-1)
    dev, Nv = pos_c.device, pos_c.shape[0]
    scratch = torch.empty(_lib.lib().a3d_dmtet_scratch_bytes(grid.edges32.shape[0], grid.tets32.shape[0]), dtype=torch.uint8, device=dev)
    vscratch = torch.empty(_lib.lib().a3d_dmtet_vertex_scratch_bytes(Nv), dtype=torch.uint8, device=dev) if surface_vertices else None
    counts = torch.empty(6, dtype=torch.int32, device=dev)
    _dmtet_count(sdf_c, pos_c, grid, scratch, counts, vscratch, False, None)
    return counts


def dmtet_extract(pos, sdf, grid, surface_vertices=False, for_backward=False, surface_points=0):
    """Topology + vertex placement, no autograd: (verts [V,3], faces int64 [F,3], uv_idx int64 [F,3], vert_edge int32 [V]).
    ``surface_vertices``: also the sorted int64 list of the grid vertices at the ends of sign-crossing edges (their count rides in the
    same read-back as V, n1, n2: no torch.nonzero, no second host synchronisation).
    ``for_backward``: a dmtet_verts(...) on this extraction will be differentiated -- its dense SDF gradient buffer is allocated now and
    cleared by the emit launch (picked up by dmtet_verts through the returned vert_edge tensor).
    ``surface_points`` = bucket > 0 (with surface_vertices): a sixth result, pos[idx] as a block of round_up(len(idx), bucket) rows with
    zero rows behind, written by the emit launch itself (a3d_dmtet_emit_opts.surf_pts)."""
    assert not surface_points or surface_vertices
    require_device(pos, sdf, grid.edges32, what="dmtet")
    pos_c, sdf_c = f32c(pos.detach()), f32c(sdf.detach()).reshape(-1)
    Ne, Nt, Nv = grid.edges32.shape[0], grid.tets32.shape[0], pos_c.shape[0]
    assert sdf_c.shape[0] == Nv, "sdf must have one value per grid vertex"
    dev = pos_c.device
    scratch = torch.empty(_lib.lib().a3d_dmtet_scratch_bytes(Ne, Nt), dtype=torch.uint8, device=dev)
    # the vertex bit plane is kept per (device, stream, grid size): the emit leaves it cleared, so only its first use pays the memset
    vscratch, vkey, vclean = None, (dev, stream(), Nv), False
    if surface_vertices:
        vscratch = _dm_vertex_scratch.pop(vkey, None)
        vclean = vscratch is not None
        if vscratch is None:
            vscratch = torch.empty(_lib.lib().a3d_dmtet_vertex_scratch_bytes(Nv), dtype=torch.uint8, device=dev)
    counts = torch.empty(6, dtype=torch.int32, device=dev)
    # (which count pass runs is decided by the grid: static tables let it skip the words off the surface.  Three launches (sign plane,
    # culled count, scan) against two: R = 64 (2.7e5 vertices) 14 vs 18 us back to back and equal inside the step, R = 128 32 vs 88 us;
    # small grids keep the plain pass)
    # mesh topology inside the extraction (DMTET_TOPOLOGY).  Preferred form: the emit launch writes the int32 triangle list AND the vertex ->
    # face lists themselves, every vertex owning ``stride`` slots (the grid bounds the valence: grid.face_list_stride()); the valence
    # counters it appends through are zeroed by the count call -- sized by a guess at V (the last extraction on this grid), since V is
    # only known after the read-back.  No launch of its own; the normals / antialiasing find the lists in the caches.
    stride = grid.face_list_stride() if (DMTET_TOPOLOGY and DMTET_EMIT_LISTS and hasattr(grid, "face_list_stride")) else 0
    counters = None
    if 0 < stride <= DMTET_EMIT_LISTS_MAX_STRIDE:
        guess = getattr(grid, "_last_surface_vertices", 0)
        counters = torch.empty(max(1024, -(-int(1.25 * guess) // 1024) * 1024), dtype=torch.int32, device=dev)
    which = _dmtet_count(sdf_c, pos_c, grid, scratch, counts, vscratch, vclean, counters)

    def alloc(Vn, Fn, n_surf_n):
        rows = -(-n_surf_n // surface_points) * surface_points if surface_points else 0
        return (torch.empty((Vn, 3), dtype=torch.float32, device=dev), torch.empty((Vn,), dtype=torch.int32, device=dev),
                torch.empty((Fn, 3), dtype=torch.int64, device=dev), torch.empty((Fn, 3), dtype=torch.int64, device=dev),
                torch.empty((n_surf_n,), dtype=torch.int64, device=dev) if surface_vertices else None,
                torch.empty((rows, 3), dtype=torch.float32, device=dev) if surface_points else None)

    g_sdf = torch.empty((Nv,), dtype=torch.float32, device=dev) if for_backward else None

    def emit(Vn, n1n, n2n, bufs, n_surf_n, tri32_t, cnt_t, adj_t, stride_n, listed, dev_counts):
        """a3d_dmtet_emit, or after the ordered count pass (surface items spread evenly over the planes) a3d_dmtet_emit_sparse."""
        use_lists = which != "ordered" and listed[0] >= 0 and listed[1] >= 0
        opts = _lib.DmtetEmitOpts(size=ctypes.sizeof(_lib.DmtetEmitOpts), Nv=Nv, vertex_scratch=ptr(vscratch), surf_idx=ptr(bufs[4]),
                                  g_sdf_to_clear=ptr(g_sdf), tri32=ptr(tri32_t), topo_count=ptr(cnt_t), topo_adj=ptr(adj_t),
                                  device_counts=ptr(dev_counts), n_surf=n_surf_n if surface_vertices else 0, topo_stride=stride_n,
                                  use_block_lists=int(use_lists), n_edge_blocks_listed=listed[0] if use_lists else 0,
                                  n_tet_blocks_listed=listed[1] if use_lists else 0, surf_bucket=int(surface_points), surf_pts=ptr(bufs[5]))
        call("a3d_dmtet_emit_sparse" if which == "ordered" else "a3d_dmtet_emit", ptr(pos_c), ptr(sdf_c), ptr(grid.edges32), ptr(grid.tet2edge32), Ne, Nt,
             ptr(scratch), Vn, n1n, n2n, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), ctypes.addressof(opts), stream())

    # SPECULATIVE emit: with the numbers of the previous extraction on this grid as a guess (+25 %), the emit launch is enqueued BEFORE
    # the host reads the counts -- the kernel takes the true sizes from the device, the GPU does not idle across the read-back, and the
    # host's wait overlaps the launch.  If anything outgrew its capacity the launch left every buffer untouched and the exact path
    # below runs as if nothing had happened.
    spec = None
    last = getattr(grid, "_last_counts", None)
    if DMTET_SPECULATIVE_EMIT and last is not None and which in ("culled", "ordered") and counters is not None and stride > 0:
        cap = lambda n, unit: max(unit, -(-int(1.25 * n) // unit) * unit)
        items = _lib.lib().a3d_dmtet_block_items()
        nbe, nbt = -(-Ne // items), -(-Nt // items)
        capV, capF, capS = min(cap(last[0], 256), counters.shape[0]), cap(last[1] + 2 * last[2], 256), cap(last[3], max(256, int(surface_points)))
        capE, capT = min(cap(last[4], 16), nbe), min(cap(last[5], 16), nbt)
        if last[0] > 0 and last[1] + last[2] > 0 and (last[4] >= 0 or which == "ordered") and capV * stride < 2 ** 31:
            bufs = alloc(capV, capF, capS)
            tri32_b = torch.empty((capF, 3), dtype=torch.int32, device=dev)
            adj_b = torch.empty(capV * stride, dtype=torch.int32, device=dev)
            emit(capV, capF, 0, bufs, capS, tri32_b, counters, adj_b, stride, (capE, capT), counts)
            spec = (capV, capF, capS, capE, capT, bufs, tri32_b, adj_b)
    # the one host sync of DMTet (the reference syncs here too, dmtet.py:110); listed_*: how many non-empty blocks the culled count
    # pass listed for the emit launch (-1: none listed)
    V, n1, n2, n_surf, listed_e, listed_t = _lib.read_back(counts).tolist()  # (+ any deferred device-side check: same transfer)
    F = n1 + 2 * n2
    grid._last_counts = (V, n1, n2, n_surf, listed_e, listed_t)
    if counters is not None:
        grid._last_surface_vertices = V
    if spec is not None and V > 0 and F > 0 and V <= spec[0] and F <= spec[1] and (not surface_vertices or n_surf <= spec[2]) \
            and (which == "ordered" or (0 <= listed_e <= spec[3] and listed_t <= spec[4])):
        bufs, tri32_b, adj_b = spec[5], spec[6], spec[7]
        verts, vert_edge, faces, uv_idx = bufs[0][:V], bufs[1][:V], bufs[2][:F], bufs[3][:F]
        idx = bufs[4][:n_surf] if surface_vertices else None
        pts = bufs[5][:-(-n_surf // surface_points) * surface_points] if surface_points else None
        tri32 = tri32_b[:F]
        adj = VertexFaceAdjacency(tri32, V, build=False, lists=(counters, adj_b, stride))
        _adj_cache.put(tri32, adj)
        _topo_cache.put(tri32, AATopology(tri32, V, build=False, lists=adj))
        _tri32_cache.put(faces, tri32)
    else:
        verts, vert_edge, faces, uv_idx, idx, pts = alloc(V, F, n_surf)
        emit_lists = counters is not None and F > 0 and 0 < V <= counters.shape[0] and V * stride < 2 ** 31
        # fallback (the guess at V was too small, or a grid with very many tets around an edge): the emit launch only counts the valences
        # and ONE more launch (a3d_mesh_topology_finalize) scans them and fills CSR lists -- instead of the conversion kernel + the four
        # launches of a3d_mesh_topology on first use
        topo = None
        if not emit_lists and DMTET_TOPOLOGY and F > 0 and 0 < V <= _lib.lib().a3d_mesh_topology_finalize_max_vertices():
            topo = _topology_sets(dev, F, V)
        tri32 = cur = nxt = lists_adj = None
        if topo is not None:
            cur, nxt = topo["sets"][topo["cur"]], topo["sets"][1 - topo["cur"]]
        if emit_lists:
            cur, lists_adj = counters, torch.empty(V * stride, dtype=torch.int32, device=dev)
        if cur is not None:
            tri32 = torch.empty((F, 3), dtype=torch.int32, device=dev)
        try:
            emit(V, n1, n2, (verts, vert_edge, faces, uv_idx, idx, pts), n_surf, tri32, cur, lists_adj, stride if emit_lists else 0, (listed_e, listed_t), None)
            adj = None
            if emit_lists:
                adj = VertexFaceAdjacency(tri32, V, build=False, lists=(counters, lists_adj, stride))
            elif topo is not None:
                adj = VertexFaceAdjacency(tri32, V, build=False)
                adj.sorted = False
                call("a3d_mesh_topology_finalize", ptr(tri32), V, F, ptr(cur), ptr(adj.off), ptr(adj.adj), ptr(nxt), topo["vcap"], stream())
                topo["cur"] ^= 1
            if adj is not None:
                _adj_cache.put(tri32, adj)
                _topo_cache.put(tri32, AATopology(tri32, V, build=False, lists=adj))
                _tri32_cache.put(faces, tri32)
        except Exception:
            if topo is not None:  # a half-used scratch pair must not be taken for clean
                _topo_sets.pop(topo["key"], None)
            raise
    if g_sdf is not None:
        _dm_grad_buffers.put(vert_edge, g_sdf)
    if not surface_vertices:
        return verts, faces, uv_idx, vert_edge
    if len(_dm_vertex_scratch) >= 4:
        _dm_vertex_scratch.clear()
    _dm_vertex_scratch[vkey] = vscratch  # only after a completed count + emit pair (a failed call leaves the buffer out of the cache)
    if surface_points:
        return verts, faces, uv_idx, vert_edge, idx, pts
    return verts, faces, uv_idx, vert_edge, idx


class _DMTetVerts(torch.autograd.Function):
    """Attaches the gradient of already-extracted surface vertices to (pos, sdf): forward returns ``verts0`` as is."""

    @staticmethod
    def forward(ctx, pos, sdf, verts0, vert_edge, grid):
        pos_c, sdf_c = f32c(pos), f32c(sdf).reshape(-1)
        ctx.save_for_backward(pos_c, sdf_c, vert_edge)
        ctx.grid, ctx.sdf_shape = grid, sdf.shape
        ctx.g_sdf = _dm_grad_buffers.take(vert_edge)  # cleared by the emit launch of dmtet_extract(for_backward=True), or None
        return verts0.detach()  # (a fresh tensor over the extraction's own buffer, which nobody else holds: no copy launch)

    @staticmethod
    def backward(ctx, g_verts):
        pos_c, sdf_c, vert_edge = ctx.saved_tensors
        Nv, V = pos_c.shape[0], vert_edge.shape[0]
        g_sdf, ctx.g_sdf = ctx.g_sdf, None  # serves ONE backward
        clear = g_sdf is not None and g_sdf.shape[0] == Nv
        if not clear:
            g_sdf = torch.empty_like(sdf_c)
        g_pos = torch.empty_like(pos_c) if ctx.needs_input_grad[0] else None
        g = f32c(g_verts) if V > 0 else None
        call("a3d_dmtet_bwd", ptr(g), ptr(pos_c), ptr(sdf_c), ptr(ctx.grid.edges32), ptr(vert_edge), V, Nv, ptr(g_pos), ptr(g_sdf), int(clear), stream())
        return g_pos, g_sdf.reshape(ctx.sdf_shape), None, None, None


def gather_rows_padded(src, idx, rows):
    """[rows,C] = src[idx] followed by zero rows (rows >= len(idx)); src [N,C] float32, idx int64 -- one launch, no autograd."""
    require_device(src, idx, what="gather_rows_padded")
    src = f32c(src)
    C = src.shape[1] if src.dim() == 2 else 1
    out = torch.empty((rows, C), dtype=torch.float32, device=src.device)
    call("a3d_dmtet_gather_rows", ptr(src), ptr(idx), idx.shape[0], rows, C, ptr(out), stream())
    return out


class _SurfaceSdf(torch.autograd.Function):
    """sdf0 with the graph of ``sdf_sub`` attached at the rows ``idx``: forward returns sdf0's values (the reference of this trick,
    sdf0.index_add(0, idx, sdf_sub - sdf_sub.detach()), adds exact zeros), backward gathers g[idx] into sdf_sub's (padded) shape."""

    @staticmethod
    def forward(ctx, sdf0, idx, sdf_sub):
        ctx.save_for_backward(idx)
        ctx.sub_shape = sdf_sub.shape
        return sdf0.detach()

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        return None, None, gather_rows_padded(g.reshape(g.shape[0], -1), idx, ctx.sub_shape[0]).view(ctx.sub_shape)


def surface_sdf(sdf0, idx, sdf_sub):
    """sdf0 [Nv,1] (no graph) whose rows idx [n] carry the graph of sdf_sub [>= n,1] (its first n rows; the rest is padding)."""
    return _SurfaceSdf.apply(sdf0, idx, sdf_sub)


def dmtet_verts(pos, sdf, verts0, vert_edge, grid):
    return _DMTetVerts.apply(pos, sdf, verts0, vert_edge, grid)


def dmtet(pos, sdf, grid):
    """(verts [V,3] differentiable w.r.t. sdf/pos, faces int64 [F,3], uv_idx int64 [F,3])."""
    verts0, faces, uv_idx, vert_edge = dmtet_extract(pos, sdf, grid)
    if torch.is_grad_enabled() and (pos.requires_grad or sdf.requires_grad):
        return _DMTetVerts.apply(pos, sdf, verts0, vert_edge, grid), faces, uv_idx
    return verts0, faces, uv_idx


# ---------------------------------------------------------------------------------------------- bone transforms
class _BoneTransforms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bones, angles, chain):
        require_device(bones, angles, chain, what="bone_transforms")
        bones, angles = f32c(bones), f32c(angles)
        N, K = angles.shape[0], angles.shape[1]
        assert bones.shape[0] in (1, N) and bones.shape[1] == K and chain.shape[0] == K and chain.dtype == torch.int32
        M = torch.empty((N, K, 12), dtype=torch.float32, device=angles.device)
        call("a3d_bone_transforms_fwd", ptr(bones), bones.shape[0], ptr(angles), ptr(chain), N, K, chain.shape[1], ptr(M), stream())
        ctx.save_for_backward(bones, angles, chain)
        return M

    @staticmethod
    def backward(ctx, g_M):
        bones, angles, chain = ctx.saved_tensors
        N, K = angles.shape[0], angles.shape[1]
        g_angles = torch.empty_like(angles)
        call("a3d_bone_transforms_bwd", ptr(f32h(g_M)), ptr(bones), bones.shape[0], ptr(angles), ptr(chain), N, K, chain.shape[1], ptr(g_angles),
             stream())
        return None, g_angles, None


def bone_transforms(bones, angles, chain):
    """bones [1|N,K,2,3] (no grad), angles [N,K,3], chain int32 [K,D] (root -> leaf, -1 padded) -> M [N,K,12]."""
    return _BoneTransforms.apply(bones, angles, chain)


_linspace_cache = {}


def _linspace01(n):
    """torch.linspace(0, 1, n) as Python floats (float32 values, computed once per n on the CPU: what the reference's tensors hold)."""
    if n not in _linspace_cache:
        _linspace_cache[n] = [float(v) for v in torch.linspace(0.0, 1.0, n, dtype=torch.float32)]
    return _linspace_cache[n]


# ---- the resample tail of a3d_estimate_bones (include/a3d.h; csrc/eb_common.h: a3d_eb_fps_tail).  _lib.EbFpsTail is its registered
# mirror (the eb_common.h entry of _lib.INTERNAL_SURFACES); filled here, behind the public struct.
FPS_TAIL_SIZE, FPS_MAX_V, FPS_REG_MAX_V = _lib.FPS_TAIL_SIZE, _lib.FPS_MAX_V, _lib.FPS_REG_MAX_V


def pack_fps_block(public, k, sample_only, start, sampled, idx):
    """The bytes a3d_estimate_bones takes for a call that resamples first: ``public`` (an _lib.EstimateBonesArgs; its ``size`` is set
    here) followed by the tail -- k, the sample-only flag and three device addresses (None = null).  8-byte aligned, like the struct."""
    n_public = ctypes.sizeof(_lib.EstimateBonesArgs)
    assert n_public % 8 == 0 and ctypes.sizeof(_lib.EbFpsTail) == FPS_TAIL_SIZE
    public.size = n_public + FPS_TAIL_SIZE
    block = (ctypes.c_uint64 * ((n_public + FPS_TAIL_SIZE) // 8))()
    ctypes.memmove(block, ctypes.addressof(public), n_public)
    tail = _lib.EbFpsTail.from_buffer(block, n_public)
    tail.k, tail.sample_only, tail.start, tail.sampled, tail.idx = int(k), int(bool(sample_only)), start, sampled, idx
    return block


def fps_workspace_words(N, V):
    """4-byte words of workspace the sampler itself needs (include/a3d.h: the running distances, beyond the register regime)."""
    return N * V if V > FPS_REG_MAX_V else 0


def fps_device_ok(pts, k):
    """Whether the device sampler takes ``pts`` [N,V,3] (else: the torch loop of geometry/util.py)."""
    return (pts.is_cuda and pts.dtype == torch.float32 and pts.dim() == 3 and pts.shape[2] == 3 and pts.shape[0] > 0
            and 1 <= k <= pts.shape[1] <= FPS_MAX_V and pts.shape[0] * pts.shape[1] <= _lib.EB_WIDE_MAX_POINTS)


def farthest_point_sample(pts, k, start, return_points=False):
    """Greedy farthest-point sampling on the GPU (csrc/fps.hip): pts [N,V,3] float32, start int64 [N] on the same device (each cloud's
    first pick) -> indices int64 [N,k]; with ``return_points`` also the points [N,k,3] (bit copies of pts).  One sample-only
    a3d_estimate_bones call: one launch, one work-group per cloud, no host synchronisation.  Ties go to the lowest index; a NaN
    distance counts as the greatest (csrc/fps.hip)."""
    require_device(pts, start, what="farthest_point_sample")
    if not fps_device_ok(pts, k):
        raise _lib.A3DError(f"farthest_point_sample: pts {tuple(pts.shape)} {pts.dtype}, k = {k}: needs [N,V,3] float32 with 1 <= k <= V <= {FPS_MAX_V} "
                            f"and N V <= {_lib.EB_WIDE_MAX_POINTS}")
    pos = f32c(pts.detach())
    N, V = pos.shape[:2]
    start = start.to(torch.int64).contiguous()
    assert start.shape == (N,)
    idx = torch.empty((N, k), dtype=torch.int64, device=pos.device)
    sampled = torch.empty((N, k, 3), dtype=torch.float32, device=pos.device)
    words = fps_workspace_words(N, V)
    work = torch.empty(words, dtype=torch.float32, device=pos.device) if words else None
    a = _lib.EstimateBonesArgs(N=N, pos=ptr(pos), V=V, workspace=ptr(work))
    block = pack_fps_block(a, k, True, ptr(start), ptr(sampled), ptr(idx))
    call("a3d_estimate_bones", ctypes.addressof(block), stream())
    return (idx, sampled) if return_points else idx


def estimate_bones_device(seq_shape, n_body_bones, n_leg_bones, body_mode_y_plus, y_threshold, attach, resample=None):
    """a3d_estimate_bones: seq_shape [B,F,V,3] (float32, on the GPU) -> (bones [B,F,K,2,3], nearest int32 [2], ok int32 [1]) -- one launch
    of one work-group, or (estimate_bones_is_wide) a dozen launches of many; no host synchronisation either way.  ``attach``: the four legs' body joints (negative = found on the device, see include/a3d.h); ``y_threshold``
    None or Fauna's bone_y_threshold.  ``resample`` (k, start int64 [B F]): the same call first reduces every cloud to k points by
    farthest-point sampling (the resample tail, csrc/fps.hip) and estimates the bones of those."""
    require_device(seq_shape, what="estimate_bones")
    pos = f32c(seq_shape)
    B, Fr, V = pos.shape[:3]
    K = n_body_bones + 4 * n_leg_bones
    dev = pos.device
    bones = torch.empty((B, Fr, K, 2, 3), dtype=torch.float32, device=dev)
    nearest = torch.empty(2, dtype=torch.int32, device=dev)
    ok = torch.empty(1, dtype=torch.int32, device=dev)
    Vb = V if resample is None else int(resample[0])  # the vertices the bones are estimated from
    # the workspace by the header's rule: 3 N V floats for the one work-group, A3D_EB_WIDE_WORKSPACE_WORDS(N, V) words for the wide path
    words = _lib.eb_wide_workspace_words(B * Fr, Vb) if estimate_bones_is_wide(B * Fr, Vb) else 3 * B * Fr * Vb
    if resample is not None:
        words = max(words, fps_workspace_words(B * Fr, V))
    work = torch.empty(words, dtype=torch.float32, device=dev)
    a = _lib.EstimateBonesArgs(size=ctypes.sizeof(_lib.EstimateBonesArgs), N=B * Fr, pos=ptr(pos), bones=ptr(bones), nearest=ptr(nearest), ok=ptr(ok), V=V,
                               workspace=ptr(work),
                               n_body=n_body_bones, n_leg=n_leg_bones, body_mode_y_plus=int(bool(body_mode_y_plus)),
                               use_y_threshold=int(y_threshold is not None), y_threshold=float(y_threshold or 0.0))
    for i, v in enumerate(attach):
        a.attach[i] = int(v)
    for i, v in enumerate(_linspace01(math.ceil((n_body_bones + 1) / 2))):
        a.blend[i] = v
    for i, v in enumerate(_linspace01(n_leg_bones + 1)):
        a.ramp[i] = v
    if resample is None:
        call("a3d_estimate_bones", ctypes.addressof(a), stream())
    else:
        k, start = resample
        require_device(start, what="estimate_bones")
        start = start.to(torch.int64).contiguous()
        sampled = torch.empty((B * Fr, Vb, 3), dtype=torch.float32, device=dev)
        block = pack_fps_block(a, k, False, ptr(start), ptr(sampled), None)
        call("a3d_estimate_bones", ctypes.addressof(block), stream())
    return bones, nearest, ok


def estimate_bones_is_wide(N, V):
    """Whether a3d_estimate_bones runs N instances of V vertices on its multi-work-group path (include/a3d.h: N and V alone decide)."""
    return N > _lib.EB_ONE_GROUP_MAX_N or N * V > _lib.EB_ONE_GROUP_MAX_POINTS


def estimate_bones_device_ok(seq_shape, n_body_bones, n_leg_bones, n_legs, wide=True):
    """Whether a3d_estimate_bones takes this call (else: the torch restatement).  ``wide`` False: only the calls of the one work-group."""
    return (seq_shape.is_cuda and seq_shape.dtype == torch.float32 and seq_shape.dim() == 4 and seq_shape.shape[3] == 3
            and seq_shape.shape[0] * seq_shape.shape[1] * seq_shape.shape[2] <= _lib.EB_WIDE_MAX_POINTS
            and (wide or not estimate_bones_is_wide(seq_shape.shape[0] * seq_shape.shape[1], seq_shape.shape[2]))
            and seq_shape.shape[2] > 0 and n_body_bones % 2 == 0 and 2 <= n_body_bones <= 32 and 0 <= n_leg_bones <= 8 and (n_leg_bones == 0 or n_legs == 4))


# ---------------------------------------------------------------------------------------------- skinning
class _Skin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, bones, T, temperature):
        require_device(v, bones, T, what="skinning")
        v, bones, T = f32c(v), f32c(bones), f32c(T)
        B, K = T.shape[0], T.shape[1]
        V = v.shape[1]
        assert v.shape[0] in (1, B) and bones.shape[0] in (1, B) and bones.shape[1] == K and T.shape[2] == 12
        out = torch.empty((B, V, 3), dtype=torch.float32, device=v.device)
        # the backward accumulates g_T with atomics: allocated now and cleared by the forward launch when a backward can follow
        g_T = torch.empty_like(T) if ctx.needs_input_grad[2] else None
        call("a3d_skin_fwd", ptr(v), v.shape[0], ptr(bones), bones.shape[0], ptr(T), B, V, K, float(temperature), ptr(out), None, ptr(g_T), stream())
        ctx.save_for_backward(v, bones, T)
        ctx.g_T = g_T
        ctx.temperature = float(temperature)
        return out

    @staticmethod
    def backward(ctx, g_out):
        v, bones, T = ctx.saved_tensors
        B, K, V = T.shape[0], T.shape[1], v.shape[1]
        g_v = torch.empty((B, V, 3), dtype=torch.float32, device=v.device) if ctx.needs_input_grad[0] else None
        g_T, ctx.g_T = ctx.g_T, None  # the cleared buffer serves ONE backward (it is handed out as the gradient)
        clear = g_T is not None
        if g_T is None:
            g_T = torch.empty_like(T)
        call("a3d_skin_bwd", ptr(f32h(g_out)), ptr(v), v.shape[0], ptr(bones), bones.shape[0], ptr(T), B, V, K, ctx.temperature, ptr(g_v),
             ptr(g_T), int(clear), stream())
        if g_v is not None and v.shape[0] == 1 and B > 1:
            g_v = g_v.sum(0, keepdim=True)  # shared canonical mesh: per-image partials, reduced here (no 16-way atomic contention)
        return g_v, None, g_T, None


def skin(v, bones, T, temperature):
    """v [1|B,V,3], bones [1|B,K,2,3] (detached), T [B,K,12] -> [B,V,3]."""
    return _Skin.apply(v, bones, T, temperature)


class _SkinPose(torch.autograd.Function):
    """skinning() as one launch each way (csrc/skin.hip, POSE kernels): (posed vertices [B,V,3], transforms T [B,K,12])."""

    @staticmethod
    def forward(ctx, v, bones, angles, chain, temperature):
        require_device(v, bones, angles, chain, what="skin_pose")
        v, bones, angles = f32c(v), f32c(bones), f32c(angles)
        B, K, V, D = angles.shape[0], angles.shape[1], v.shape[1], chain.shape[1]
        assert v.shape[0] in (1, B) and bones.shape[0] in (1, B) and bones.shape[1] == K and chain.shape[0] == K and chain.dtype == torch.int32
        out = torch.empty((B, V, 3), dtype=torch.float32, device=v.device)
        T = torch.empty((B, K, 12), dtype=torch.float32, device=v.device)
        # the backward accumulates the angle gradients with atomics: its buffer is allocated now and cleared by the forward launch
        g_angles = torch.empty_like(angles) if (ctx.needs_input_grad[0] or ctx.needs_input_grad[2]) else None
        products = None if g_angles is None else torch.empty((B, _lib.lib().a3d_skin_pose_products_floats(K, D)), dtype=torch.float32, device=v.device)
        call("a3d_skin_pose_fwd", ptr(v), v.shape[0], ptr(bones), bones.shape[0], ptr(angles), ptr(chain), B, V, K, D, float(temperature),
             ptr(out), ptr(T), ptr(products), ptr(g_angles), stream())
        ctx.save_for_backward(v, bones, angles, chain, T, products)
        ctx.g_angles = g_angles
        ctx.temperature = float(temperature)
        ctx.set_materialize_grads(False)
        return out, T

    @staticmethod
    def backward(ctx, g_out, g_T_ext):
        v, bones, angles, chain, T, products = ctx.saved_tensors
        B, K, V, D = angles.shape[0], angles.shape[1], v.shape[1], chain.shape[1]
        if g_out is None:  # only the transforms were used downstream
            g_out = torch.zeros((B, V, 3), dtype=torch.float32, device=v.device)
        g_v = torch.empty((B, V, 3), dtype=torch.float32, device=v.device) if ctx.needs_input_grad[0] else None
        g_angles, ctx.g_angles = ctx.g_angles, None  # the cleared buffer serves ONE backward
        clear = g_angles is not None
        if g_angles is None:
            g_angles = torch.empty_like(angles)
        call("a3d_skin_pose_bwd", ptr(f32h(g_out)), ptr(v), v.shape[0], ptr(bones), bones.shape[0], ptr(T), ptr(products), ptr(angles), ptr(chain), B, V, K, D,
             ctx.temperature, ptr(g_v), ptr(None if g_T_ext is None else f32h(g_T_ext)), ptr(g_angles), int(clear), stream())
        if g_v is not None and v.shape[0] == 1 and B > 1:
            g_v = g_v.sum(0, keepdim=True)
        return g_v, None, g_angles, None, None


def skin_pose_supported(K, D):
    return K <= _lib.lib().a3d_skin_pose_max_bones() and D <= 8


def skin_pose(v, bones, angles, chain, temperature):
    """v [1|B,V,3], bones [1|B,K,2,3] (detached), angles [B,K,3], chain int32 [K,D] -> (posed [B,V,3], T [B,K,12])."""
    return _SkinPose.apply(v, bones, angles, chain, temperature)


def skin_weights(v, bones, B, temperature):
    """aux['vertices_to_bones'] on demand: [K, Bw, V]."""
    require_device(v, bones, what="skin_weights")
    v, bones = f32c(v), f32c(bones)
    K, V = bones.shape[1], v.shape[1]
    Bw = max(v.shape[0], bones.shape[0])
    T = torch.zeros((Bw, K, 12), dtype=torch.float32, device=v.device)
    out = torch.empty((Bw, V, 3), dtype=torch.float32, device=v.device)
    w = torch.empty((K, Bw, V), dtype=torch.float32, device=v.device)
    call("a3d_skin_fwd", ptr(v), v.shape[0], ptr(bones), bones.shape[0], ptr(T), Bw, V, K, float(temperature), ptr(out), ptr(w), None, stream())
    return w


# ---------------------------------------------------------------------------------------------- normals
class VertexFaceAdjacency:
    """Vertex -> incident (corner, face) entries of one triangle list: CSR, built by a3d_normals_adjacency / a3d_mesh_topology[_finalize],
    or -- ``lists`` -- fixed stride, as the DMTet emit launch writes them."""

    def __init__(self, tri32: torch.Tensor, num_vertices: int, build: bool = True, lists=None):
        require_device(tri32, what="normals_adjacency")
        F, V = tri32.shape[0], int(num_vertices)
        self.tri, self.num_vertices = tri32, V
        self.sorted = True  # lists stored in ascending key order (False for the lists a3d_mesh_topology_finalize / the DMTet emit leave)
        self.stride = 0  # 0: CSR (off[V+1]); S > 0: list v = adj[v*S .. v*S + off[v]) -- written by the DMTet emit launch (include/a3d.h: lists_stride)
        if lists is not None:  # (list lengths, slots, stride) as a3d_dmtet_emit wrote them
            self.off, self.adj, self.stride = lists
            self.sorted = False
            return
        self.off = torch.empty(V + 1, dtype=torch.int32, device=tri32.device)
        self.adj = torch.empty(max(3 * F, 1), dtype=torch.int32, device=tri32.device)
        if build:
            cursor = torch.empty(V, dtype=torch.int32, device=tri32.device)
            call("a3d_normals_adjacency", ptr(tri32), V, F, ptr(self.off), ptr(self.adj), ptr(cursor), stream())


_adj_cache = _IdentityCache()


def vertex_face_adjacency(tri32: torch.Tensor, num_vertices: int) -> VertexFaceAdjacency:
    adj = _adj_cache.peek(tri32)
    if adj is None:
        adj = mesh_topology(tri32, num_vertices)[0]
    if adj.num_vertices != num_vertices:  # same triangle list used with another vertex count: rebuild, do not trust the cache
        adj = VertexFaceAdjacency(tri32, num_vertices)
    return adj


NORMALS_FACES_FIRST = os.environ.get("A3D_NORMALS_FACES_FIRST", "1") != "0"  # a3d_normals_bwd: every face's adjoint once + a sum per vertex


def _normals_bwd_call(g, acc, v, tri32, adjacency, B, V, F):
    """a3d_normals_bwd for one vertex array -> g_v.  Faces first (a [B,F,9] scratch) unless switched off: same bits, ~half the gathers."""
    g_v = torch.empty_like(v)
    faces_first = NORMALS_FACES_FIRST and F > 0
    face_scratch = torch.empty((B, F, 9), dtype=torch.float32, device=v.device) if faces_first else None
    scratch = None if faces_first else torch.empty_like(v)
    call("a3d_normals_bwd", ptr(g), g.stride(1), ptr(acc), ptr(v), ptr(tri32), ptr(adjacency.off), ptr(adjacency.adj), B, V, F, ptr(scratch),
         ptr(g_v), adjacency.stride, ptr(face_scratch), stream(), tag=f"[B{B}]")
    return g_v


class _Normals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, tri32, adjacency):
        require_device(v, tri32, what="vertex_normals")
        v = f32c(v)
        B, V, F = v.shape[0], v.shape[1], tri32.shape[0]
        acc = torch.empty_like(v)
        nrm = torch.empty_like(v)
        call("a3d_normals_fwd", ptr(v), ptr(tri32), ptr(adjacency.off), ptr(adjacency.adj), B, V, F, ptr(acc), ptr(nrm), adjacency.stride,
             stream(), tag=f"[B{B}]")
        ctx.save_for_backward(v, acc, tri32)
        ctx.adjacency = adjacency
        return nrm

    @staticmethod
    def backward(ctx, g_nrm):
        v, acc, tri32 = ctx.saved_tensors
        B, V, F = v.shape[0], v.shape[1], tri32.shape[0]
        if g_nrm.dtype != torch.float32 or g_nrm.stride(2) != 1 or g_nrm.stride(0) != V * g_nrm.stride(1):  # rows must be evenly strided
            g_nrm = f32c(g_nrm)
        return _normals_bwd_call(g_nrm, acc, v, tri32, ctx.adjacency, B, V, F), None, None


class _NormalsPair(torch.autograd.Function):
    """Vertex normals of two vertex arrays over one triangle list from ONE launch: (nrm_a [Ba,V,3], nrm_b [Bb,V,3])."""

    @staticmethod
    def forward(ctx, v_a, v_b, tri32, adjacency):
        require_device(v_a, v_b, tri32, what="vertex_normals_pair")
        v_a, v_b = f32c(v_a), f32c(v_b)
        V, F = v_a.shape[1], tri32.shape[0]
        assert v_b.shape[1] == V
        acc_a, nrm_a, acc_b, nrm_b = torch.empty_like(v_a), torch.empty_like(v_a), torch.empty_like(v_b), torch.empty_like(v_b)
        call("a3d_normals_fwd_pair", ptr(v_a), v_a.shape[0], ptr(v_b), v_b.shape[0], ptr(tri32), ptr(adjacency.off), ptr(adjacency.adj), V, F,
             ptr(acc_a), ptr(nrm_a), ptr(acc_b), ptr(nrm_b), adjacency.stride, stream(), tag=f"[B{v_a.shape[0]}+B{v_b.shape[0]}]")
        ctx.save_for_backward(v_a, acc_a, v_b, acc_b, tri32)
        ctx.adjacency = adjacency
        ctx.set_materialize_grads(False)
        return nrm_a, nrm_b

    @staticmethod
    def backward(ctx, g_a, g_b):
        v_a, acc_a, v_b, acc_b, tri32 = ctx.saved_tensors
        F = tri32.shape[0]
        out = []
        for v, acc, g in ((v_a, acc_a, g_a), (v_b, acc_b, g_b)):
            if g is None or v is None:
                out.append(None)
                continue
            B, V = v.shape[0], v.shape[1]
            if g.dtype != torch.float32 or g.stride(2) != 1 or g.stride(0) != V * g.stride(1):
                g = f32c(g)
            out.append(_normals_bwd_call(g, acc, v, tri32, ctx.adjacency, B, V, F))
        return out[0], out[1], None, None


class NormalsJob:
    """The forward pass of vertex_normals_pair(v_a, v_b, tri) as a side job of the rasteriser's triangle launch: hand it to
    rasterize(normals_job=...), which fills acc / nrm and sets ``done``; vertex_normals_attach then puts the results on the autograd
    graph.  ``v_b`` may be None."""

    def __init__(self, v_a, v_b, tri):
        self.tri32 = tri_int32(tri)
        self.v_a = f32c(v_a.detach())
        self.v_b = None if v_b is None else f32c(v_b.detach())
        assert self.v_b is None or self.v_b.shape[1] == self.v_a.shape[1]
        self.adjacency = vertex_face_adjacency(self.tri32, self.v_a.shape[1])
        self.acc_a = self.nrm_a = self.acc_b = self.nrm_b = None
        self.done = False


class _NormalsAttach(torch.autograd.Function):
    """(nrm_a, nrm_b) of a finished NormalsJob as functions of (v_a, v_b): forward hands out the job's buffers, backward is
    _NormalsPair's."""

    @staticmethod
    def forward(ctx, v_a, v_b, job):
        assert job.done
        ctx.save_for_backward(job.v_a, job.acc_a, job.v_b, job.acc_b, job.tri32)
        ctx.adjacency = job.adjacency
        ctx.set_materialize_grads(False)
        return job.nrm_a, job.nrm_b

    @staticmethod
    def backward(ctx, g_a, g_b):
        return _NormalsPair.backward(ctx, g_a, g_b)[:2] + (None,)


def vertex_normals_attach(v_a, v_b, job):
    """(normals of v_a, normals of v_b or None) computed by ``job`` inside a rasteriser launch, differentiable like vertex_normals_pair."""
    return _NormalsAttach.apply(v_a, v_b, job)


def vertex_normals_pair(v_a, v_b, tri):
    """(normals of v_a, normals of v_b): two meshes that share ``tri``, one launch."""
    tri32 = tri_int32(tri)
    return _NormalsPair.apply(v_a, v_b, tri32, vertex_face_adjacency(tri32, v_a.shape[1]))


def vertex_normals(v, tri):
    """Area-weighted, normalised vertex normals [B,V,3] (auto_normals); the adjacency is built once per triangle list."""
    tri32 = tri_int32(tri)
    return _Normals.apply(v, tri32, vertex_face_adjacency(tri32, v.shape[1]))


# ---------------------------------------------------------------------------------------------- clip-space transform
class _XfmPoints(torch.autograd.Function):
    """xfm_points(points, matrix, use_python=True) (renderutils/ops.py:515-531): [points, 1] . matrix^T as one launch each way
    (csrc/xfm.hip) instead of pad + bmm (+ two bmm and a slice backward)."""

    @staticmethod
    def forward(ctx, points, matrix, alias=False):
        require_device(points, matrix, what="xfm_points")
        points, matrix = f32c(points), f32c(matrix)
        Bp, V, Bm = points.shape[0], points.shape[1], matrix.shape[0]
        B = max(Bp, Bm)
        assert points.shape[2] == 3 and matrix.shape[1:] == (4, 4) and Bp in (1, B) and Bm in (1, B)
        out = torch.empty((B, V, 4), dtype=torch.float32, device=points.device)
        g_M = torch.empty_like(matrix) if ctx.needs_input_grad[1] else None  # (accumulated by the backward with atomics: cleared here)
        call("a3d_xfm_points_fwd", ptr(points), Bp, ptr(matrix), Bm, B, V, ptr(out), ptr(g_M), stream())
        ctx.save_for_backward(points, matrix)
        ctx.g_M = g_M
        ctx.set_materialize_grads(False)
        # ``alias``: the points once more as a second output (no copy) for their OTHER consumer in render_mesh (the G-buffer's position
        # attribute): both gradients then arrive at this node and are summed inside its one backward launch, instead of by an accumulation
        # kernel of the autograd engine in front of it.  alias = 2: ... and a third output for their third consumer, the vertex normals.
        # alias = 3: ... and the CLIP positions a second time, for the consumer beside the rasteriser / G-buffer: the antialiasing.
        if alias and Bp == B:
            return out, points.detach(), (points.detach() if int(alias) >= 2 else None), (out.detach() if int(alias) >= 3 else None)
        return out, None, None, None

    @staticmethod
    def backward(ctx, g, g_alias=None, g_alias2=None, g_second=None):
        points, matrix = ctx.saved_tensors
        Bp, V, Bm = points.shape[0], points.shape[1], matrix.shape[0]
        B = max(Bp, Bm)
        if g_alias is None and g_alias2 is not None:
            g_alias, g_alias2 = g_alias2, None
        if g is None and g_second is not None:
            g, g_second = g_second, None
        if g is None:
            if g_alias is None:
                return None, None, None
            g = torch.zeros((B, V, 4), dtype=torch.float32, device=points.device)
        # (the gradient may be the clip columns of the G-buffer's 16-float gradient rows: read in place, with its vertex stride)
        if g.dtype != torch.float32 or g.stride(2) != 1 or g.stride(1) < 4 or g.stride(0) != V * g.stride(1):
            g = f32c(g)
        if g_alias is not None and (g_alias.dtype != torch.float32 or g_alias.stride(2) != 1 or g_alias.stride(1) < 3 or g_alias.stride(0) != V * g_alias.stride(1)):
            g_alias = f32c(g_alias)
        if g_second is not None and (g_second.dtype != torch.float32 or g_second.stride(2) != 1 or g_second.stride(1) < 4 or g_second.stride(0) != V * g_second.stride(1)):
            g_second = f32c(g_second)
        if g_alias2 is not None and (g_alias2.dtype != torch.float32 or g_alias2.stride(2) != 1 or g_alias2.stride(1) < 3 or g_alias2.stride(0) != V * g_alias2.stride(1)):
            g_alias2 = f32c(g_alias2)
        g_p = torch.empty((B, V, 3), dtype=torch.float32, device=points.device) if ctx.needs_input_grad[0] else None
        g_M, ctx.g_M = ctx.g_M, None  # the cleared buffer serves ONE backward
        clear = g_M is not None
        if g_M is None and ctx.needs_input_grad[1]:
            g_M = torch.empty_like(matrix)
        if g_alias is not None and g_p is None:
            g_p = torch.empty((B, V, 3), dtype=torch.float32, device=points.device)
        call("a3d_xfm_points_bwd", ptr(g), g.stride(1), ptr(points), Bp, ptr(matrix), Bm, B, V, ptr(g_p), ptr(g_M), int(clear), ptr(g_alias),
             0 if g_alias is None else g_alias.stride(1), ptr(g_alias2), 0 if g_alias2 is None else g_alias2.stride(1), ptr(g_second),
             0 if g_second is None else g_second.stride(1), stream())
        if g_p is not None and Bp == 1 and B > 1:
            g_p = g_p.sum(0, keepdim=True)
        return g_p, g_M, None


def xfm_points(points, matrix, alias=False):
    """points [1|B,V,3], matrix [1|B,4,4] -> [B,V,4] homogeneous clip-space positions.  ``alias``: -> (clip, the points as a second output
    of the same node or None); alias = 2: -> (clip, second output, third output); alias = 3: -> (..., clip once more): see _XfmPoints."""
    out, again, third, out_again = _XfmPoints.apply(points, matrix, alias)
    if int(alias) >= 3:
        return out, again, third, out_again
    if int(alias) == 2:
        return out, again, third
    return (out, again) if alias else out


class _FlowDelta(torch.autograd.Function):
    """delta_xy of render_mesh (render.py:281-288) from the clip positions: one launch each way (csrc/xfm.hip)."""

    @staticmethod
    def forward(ctx, clip, num_frames):
        require_device(clip, what="flow_delta")
        clip = f32c(clip)
        N, V = clip.shape[0], clip.shape[1]
        delta = torch.empty((N, V, 2), dtype=torch.float32, device=clip.device)
        call("a3d_flow_delta_fwd", ptr(clip), N, int(num_frames), V, ptr(delta), stream())
        ctx.save_for_backward(clip)
        ctx.num_frames = int(num_frames)
        return delta

    @staticmethod
    def backward(ctx, g):
        (clip,) = ctx.saved_tensors
        N, V = clip.shape[0], clip.shape[1]
        g_clip = torch.empty_like(clip)
        # (the gradient may be two columns of the G-buffer backward's 16-float rows: read in place, with its vertex stride)
        if g.dtype != torch.float32 or g.stride(2) != 1 or g.stride(1) < 2 or g.stride(0) != V * g.stride(1):
            g = f32c(g)
        call("a3d_flow_delta_bwd", ptr(g), g.stride(1), ptr(clip), N, ctx.num_frames, V, ptr(g_clip), stream())
        return g_clip, None


def flow_delta(clip, num_frames):
    """clip [B*F,V,4] -> [B*F,V,2]: ndc of the next frame minus ndc of this one, zeros for a sequence's last frame."""
    return _FlowDelta.apply(clip, num_frames)


# ---------------------------------------------------------------------------------------------- covered pixels
_cover_counts = _IdentityCache(maxsize=2)  # raster buffer -> block counts of its covered-pixel list
_aa_prepared = _IdentityCache(maxsize=2)  # raster buffer -> (key of its clip tensor, screen positions, zeroed counters)


def _cover_counted(rast, tile):
    """(scratch, length of the list): block counts + group sums left by the rasteriser's resolve (same launch), otherwise a counting pass
    of our own; the ONE read-back: the group sums (a few KB; unused words are zero), added up on the host."""
    B, H, W = rast.shape[:3]
    ensure_resolved(rast)
    scratch = _cover_counts.peek(rast) if tile == 8 else None
    if scratch is None:
        scratch = torch.empty(_lib.lib().a3d_cover_scratch_bytes(B, H, W) // 4, dtype=torch.int32, device=rast.device)
        call("a3d_cover_count", ptr(rast), B, H, W, tile, ptr(scratch), stream())
    nb = _lib.lib().a3d_cover_blocks(B, H, W)
    tail = _lib.read_back(scratch[nb:nb + _lib.lib().a3d_cover_groups(B, H, W) * _lib.lib().a3d_cover_group_stride()])  # THE read-back: one sum per group of 64 blocks, one per 64-byte line; the other words of a line are never part of the sums
    return scratch, int(tail[::_lib.lib().a3d_cover_group_stride()].sum())


def covered_pixels(rast, tile=8, return_inverse=False):
    """int64 [P] flat indices of the pixels with rast[...,3] > 0, image-major, 8x8-tile order inside an image (``tile=8``; falls back
    to row-major when H or W is not a multiple of 8).  One 8-byte read-back (P) between the count and the emit launches.
    ``return_inverse``: also int32 [B*H*W], the list entry of every pixel (-1 = uncovered), written by the same launch."""
    require_device(rast, what="covered_pixels")
    rast = f32c(rast.detach())
    B, H, W = rast.shape[:3]
    if tile != 8 or H % 8 or W % 8:
        tile = 0
    dev = rast.device
    scratch, total = _cover_counted(rast, tile)
    pix = torch.empty(total, dtype=torch.int64, device=dev)
    inv = torch.empty(B * H * W, dtype=torch.int32, device=dev) if return_inverse else None
    if pix.shape[0] or return_inverse:
        call("a3d_cover_emit", ptr(rast), B, H, W, tile, ptr(scratch), ptr(pix), ptr(inv), stream())
    return (pix, inv) if return_inverse else pix


# ---------------------------------------------------------------------------------------------- rasterise
_rast_keys = {}
# (round 5) rasterize(defer_resolve=True): only the triangle launch runs; the raster buffer is WRITTEN by the covered_gbuffer call that
# follows (a3d_rast_resolve_gbuffer_fwd: resolve + covered-pixel list + G-buffer rows in one launch, the list offsets by decoupled
# look-back) -- or, for any other reader, by ensure_resolved (the stand-alone resolve).  The list's length is not known when that launch
# is enqueued: its rows are allocated for the previous frame's length + 25 % (per device and frame size) and the exact two-launch path
# re-runs when the frame outgrew them.
DEFER_RESOLVE = os.environ.get("A3D_DEFER_RESOLVE", "1") != "0"


class _PendingResolves(_IdentityCache):
    """raster buffer -> what its resolve needs (clip, triangle list, key buffer).  An entry that is pushed out before anybody resolved
    it is RESOLVED on the way out (stand-alone launch): a raster buffer handed to a reader must never be left as uninitialised texels
    because a third deferred call came before its consumer did."""

    def put(self, t, val):
        self.data[self.key(t)] = (t, val)
        self.data.move_to_end(self.key(t))
        while len(self.data) > self.maxsize:
            _, (rast_old, pend) = self.data.popitem(last=False)
            _run_standalone_resolve(rast_old, pend)
            resolve_events["evicted"] = resolve_events.get("evicted", 0) + 1
        return val


def _run_standalone_resolve(rast, pend):
    B, H, W = rast.shape[:3]
    clip, tri32 = pend["clip"], pend["tri32"]
    call("a3d_rast_resolve", ptr(clip), clip.shape[0], ptr(tri32), B, clip.shape[1], tri32.shape[0], H, W, ptr(pend["rast"]), ptr(pend["keys"]),
         ptr(pend["cover"]), stream())
    _rast_keys[pend["key"]] = pend["keys"]  # (re-armed by the resolve)
    resolve_events["standalone"] += 1


_pending_resolve = _PendingResolves(maxsize=2)
_cover_last_len = {}  # (device, B, H, W) -> length of the last covered-pixel list
resolve_events = dict(fused=0, outgrown=0, standalone=0)
_debug_force_lookback_timeout = False  # tests: take the recovery path of a timed-out look-back


_dispatch_probe = {}  # device -> dict(ok, workgroups, stride, ms): the look-back's dispatch-order property as probed on that device


def dispatch_order_ok(device, n_workgroups=16384, stride=64):
    """Probe (once per device and process) that work-groups are dispatched in the order of their linear index -- what the fused resolve's
    look-back rests on (a3d_dispatch_order_probe) -- and remember the answer; rasterize defers its resolve only where it holds."""
    key = torch.device(device)
    hit = _dispatch_probe.get(key)
    if hit is None:
        import time

        with torch.cuda.device(key):
            scratch = torch.empty(n_workgroups + 1, dtype=torch.int32, device=key)
            torch.cuda.synchronize(key)
            t0 = time.perf_counter()
            call("a3d_dispatch_order_probe", n_workgroups, stride, ptr(scratch), stream())
            status = int(scratch[n_workgroups].item())
            ms = (time.perf_counter() - t0) * 1e3
        hit = _dispatch_probe[key] = dict(ok=status == 2, status=status, workgroups=n_workgroups, stride=stride, ms=round(ms, 3))
        if not hit["ok"]:
            import warnings

            warnings.warn(f"a3d_dispatch_order_probe on {key}: status {status} (2 = in order): the rasteriser's resolve will not be deferred on this device")
    return hit["ok"]


def ensure_resolved(rast):
    """Run the stand-alone resolve launch now if ``rast`` came out of rasterize(defer_resolve=True) and nothing has resolved it yet."""
    pend = _pending_resolve.take(rast)
    if pend is not None:
        _run_standalone_resolve(rast, pend)


def drop_pending_resolve(rast):
    """A deferred raster buffer whose consumer failed before it ran: resolve it now (keys re-armed, nothing left pinned)."""
    ensure_resolved(rast)


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, clip, tri32, B, H, W, prev, job, defer=False):
        require_device(clip, tri32, what="rasterize")
        clip = f32c(clip)
        V, F = clip.shape[1], tri32.shape[0]
        rast = torch.empty((B, H, W, 4), dtype=torch.float32, device=clip.device)
        # the (depth, id) key buffer is kept per (device, stream, size): the resolve leaves it armed, so only its first use pays the clear
        key = (clip.device, stream(), B, H, W)
        if prev is not None:
            prev = f32c(prev.detach())
            assert prev.shape == (B, H, W, 4)
        # the covered-pixel list's block counts ride along with the resolve when the list's tile order applies (covered_pixels picks them up)
        cover = None
        if H % 8 == 0 and W % 8 == 0 and (H * W) % 256 == 0 and F > 0:
            cover = torch.empty(_lib.lib().a3d_cover_scratch_bytes(B, H, W) // 4, dtype=torch.int32, device=clip.device)
        scratch = _rast_keys.pop(key, None)
        clean = scratch is not None
        if scratch is None:
            scratch = torch.empty(_lib.lib().a3d_rast_scratch_bytes(B, H, W), dtype=torch.uint8, device=clip.device)
        # ... and so does what the silhouette analysis of this frame needs first (pixel-space vertex positions, zeroed append counters):
        # AAAnalysis picks them up when it is built for this raster buffer and this clip tensor
        aa_screen = aa_count = None
        if F > 0 and prev is None:
            aa_screen = torch.empty((clip.shape[0], V, 2), dtype=torch.float32, device=clip.device)
            aa_count = torch.empty((_lib.lib().a3d_aa_shards(),), dtype=torch.int32, device=clip.device)
        # ... and the opposite-vertex table, when this triangle list came with vertex -> face lists only (DMTet extraction): filled by
        # further extra work-groups of the same launch, picked up by the silhouette analysis through the topology cache
        topo = _topo_cache.peek(tri32) if F > 0 else None
        lists = getattr(topo, "lists", None) if (topo is not None and topo.opp is None) else None
        opp = torch.empty((F, 3), dtype=torch.int32, device=clip.device) if lists is not None else None
        # ... and a pending vertex-normals pass over the same triangle list (NormalsJob: the mesh being rasterised + the canonical one)
        if job is not None and not (F > 0 and job.tri32.data_ptr() == tri32.data_ptr() and job.v_a.shape[1] == V and job.v_a.device == clip.device):
            job = None  # (stays not done: the caller computes the normals in a launch of their own)
        opts = _lib.RastOpts(size=ctypes.sizeof(_lib.RastOpts), prev_rast=ptr(prev), cover_scratch=ptr(cover), aa_screen=ptr(aa_screen),
                             aa_count=ptr(aa_count), topo_off=ptr(None if lists is None else lists.off), topo_adj=ptr(None if lists is None else lists.adj),
                             topo_opp=ptr(opp))
        stride = lists.stride if lists is not None else (job.adjacency.stride if job is not None else 0)
        if job is not None and lists is not None and lists is not job.adjacency and lists.stride != job.adjacency.stride:
            job = None  # (one layout per launch)
        if job is not None:
            job.acc_a, job.nrm_a = torch.empty_like(job.v_a), torch.empty_like(job.v_a)
            if job.v_b is not None:
                job.acc_b, job.nrm_b = torch.empty_like(job.v_b), torch.empty_like(job.v_b)
            opts.normals_v_a, opts.normals_B_a, opts.normals_v_b = ptr(job.v_a), job.v_a.shape[0], ptr(job.v_b)
            opts.normals_B_b = 0 if job.v_b is None else job.v_b.shape[0]
            opts.normals_off, opts.normals_adj = ptr(job.adjacency.off), ptr(job.adjacency.adj)
            opts.normals_acc_a, opts.normals_a, opts.normals_acc_b, opts.normals_b = ptr(job.acc_a), ptr(job.nrm_a), ptr(job.acc_b), ptr(job.nrm_b)
        opts.lists_stride = stride
        defer = bool(defer) and DEFER_RESOLVE and cover is not None and prev is None and F > 0
        defer = defer and not torch.cuda.is_current_stream_capturing() and dispatch_order_ok(clip.device)  # (probed once per device)
        opts.defer_resolve = int(defer)
        call("a3d_rast_fwd", ptr(clip), clip.shape[0], ptr(tri32), B, V, F, H, W, ptr(rast), ptr(scratch), int(clean), ctypes.addressof(opts), stream(),
             tag=("" if job is None else f"[N{opts.normals_B_a}+{opts.normals_B_b}]") + ("[defer]" if defer else ""))
        if job is not None:
            job.done = True
        if opp is not None:
            topo.opp = opp
        if cover is not None:
            _cover_counts.put(rast.detach(), cover)  # keyed on a detached alias: the entry must not pin this iteration's autograd graph
        if aa_screen is not None:
            # (the clip tensor rides in the entry so that its address cannot be recycled while the entry can still match)
            _aa_prepared.put(rast.detach(), (_IdentityCache.key(clip), aa_screen, aa_count, clip.detach()))
        if len(_rast_keys) >= 4:
            _rast_keys.clear()
        if defer:  # the keys are full until a resolve has consumed them: they travel with the raster buffer, not back into the cache
            _pending_resolve.put(rast.detach(), dict(clip=clip, tri32=tri32, keys=scratch, key=key, rast=rast, cover=cover))
        elif F > 0 or clean:  # only after a successful call whose resolve re-armed the keys (F == 0 returns before touching
            _rast_keys[key] = scratch  # them: a fresh torch.empty buffer must not come back as "clean"; a failed call leaves the buffer out too)
        ctx.save_for_backward(clip, tri32, rast)
        return rast

    @staticmethod
    def backward(ctx, g_rast):
        clip, tri32, rast = ctx.saved_tensors
        ensure_resolved(rast)
        B, H, W = rast.shape[:3]
        g_clip = torch.empty_like(clip)
        call("a3d_rast_bwd", ptr(f32h(g_rast)), ptr(rast), ptr(clip), clip.shape[0], ptr(tri32), B, clip.shape[1], tri32.shape[0], H, W,
             ptr(g_clip), stream())
        return g_clip, None, None, None, None, None, None, None


def rasterize(clip, tri, resolution, batch=None, prev=None, normals_job=None, defer_resolve=False):
    """clip [B|1,V,4] -> rast [B,H,W,4] = (u, v, z/w, triangle_id+1); differentiable through (u,v).  ``prev`` = the previous
    depth layer (DepthPeeler.rasterize_next_layer for layer n > 0): the nearest surface strictly behind it is returned.
    ``normals_job``: a NormalsJob over the same triangle list, run as extra work-groups of the triangle launch.
    ``defer_resolve``: the caller promises that covered_gbuffer(..., rast, ...) comes next (render_mesh's fused path): the texels are then
    written by THAT launch (see DEFER_RESOLVE); any other reader must call ensure_resolved(rast) first (covered_pixels does)."""
    if clip.dim() == 2:
        clip = clip[None]
    B = clip.shape[0] if batch is None else batch
    return _Rasterize.apply(clip, tri_int32(tri), B, int(resolution[0]), int(resolution[1]), prev, normals_job, defer_resolve)


def _deriv_on_gpu(*tensors):
    """The derivative kernels take CUDA float32 tensors; anything else (CPU, float64 ...) goes to the torch statement."""
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


class _RasterizeDb(torch.autograd.Function):
    """a3d_rast_db_fwd / a3d_rast_db_bwd (csrc/deriv.hip): one launch each way.  ``rast`` receives no gradient (it only names the
    triangle).  A backward under create_graph=True (double backward) differentiates the torch statement instead."""

    @staticmethod
    def forward(ctx, clip, tri32, rast):
        require_device(clip, tri32, rast, what="rasterize_db")
        ensure_resolved(rast)
        clip_c, rast_c = f32c(clip), f32c(rast)
        B, H, W = rast_c.shape[:3]
        assert clip_c.dim() == 3 and clip_c.shape[0] in (1, B) and clip_c.shape[2] == 4 and rast_c.shape[3] == 4
        db = torch.empty((B, H, W, 4), dtype=torch.float32, device=rast_c.device)
        call("a3d_rast_db_fwd", ptr(clip_c), clip_c.shape[0], ptr(tri32), ptr(rast_c), B, clip_c.shape[1], tri32.shape[0], H, W, ptr(db), stream())
        ctx.save_for_backward(clip, tri32, rast_c)
        return db

    @staticmethod
    def backward(ctx, g_db):
        clip, tri32, rast = ctx.saved_tensors
        if torch.is_grad_enabled():  # double backward: the torch statement, differentiated by autograd
            with torch.enable_grad():
                (g_clip,) = torch.autograd.grad(_rasterize_db_torch(clip, tri32, rast), clip, g_db, create_graph=True)
            return g_clip, None, None
        clip_c = f32c(clip)
        B, H, W = rast.shape[:3]
        g_clip = torch.empty_like(clip_c)
        call("a3d_rast_db_bwd", ptr(f32h(g_db)), ptr(clip_c), clip_c.shape[0], ptr(tri32), ptr(rast), B, clip_c.shape[1], tri32.shape[0], H, W,
             ptr(g_clip), stream())
        return g_clip, None, None


def rasterize_db(clip, tri, rast):
    """rast_db [B,H,W,4] = (du/dX, du/dY, dv/dX, dv/dY) per pixel: the image-space derivatives of the perspective-correct
    barycentrics of the stored triangle, from the definition u = a0/s, a_i = q_j x q_k, q_i = p_i.xy - f p_i.w; differentiable w.r.t.
    clip like nvdiffrast's (grad_db).  CUDA float32 tensors: one HIP launch each way (a3d_rast_db_fwd / _bwd, csrc/deriv.hip; a pixel
    whose triangle is exactly edge-on at the pixel centre, s == 0, which the rasteriser never stores, gets zeros); anything else --
    CPU tensors, float64, a double backward -- evaluates the torch statement _rasterize_db_torch, which is also the specification.
    Nothing on the training path consumes it (render.py:24 passes rast_db=None)."""
    if clip.dim() == 2:
        clip = clip[None]
    if _deriv_on_gpu(clip, rast) and tri.is_cuda:
        return _RasterizeDb.apply(clip, tri_int32(tri), rast)
    return _rasterize_db_torch(clip, tri, rast)


def _rasterize_db_torch(clip, tri, rast):
    """rasterize_db as torch operations (about 30 launches over [B,H,W,3,4] gathers): the statement the kernels follow operation by
    operation, the path of CPU / float64 tensors and of a double backward, and what tests and tools/bench_deriv.py compare against."""
    B, H, W, _ = rast.shape
    ensure_resolved(rast)
    ids = rast[..., 3].long() - 1
    hit = ids >= 0
    t = tri.long()[ids.clamp(min=0)]
    P = clip.expand(B, -1, -1)[torch.arange(B, device=rast.device)[:, None, None, None].expand_as(t), t]  # [B,H,W,3,4]
    fx = ((torch.arange(W, dtype=torch.float32, device=rast.device) + 0.5) * (2.0 / W) - 1.0)[None, None, :, None]
    fy = ((torch.arange(H, dtype=torch.float32, device=rast.device) + 0.5) * (2.0 / H) - 1.0)[None, :, None, None]
    x, y, w = P[..., 0], P[..., 1], P[..., 3]
    qx, qy = x - fx * w, y - fy * w
    a = [qx[..., 1] * qy[..., 2] - qy[..., 1] * qx[..., 2], qx[..., 2] * qy[..., 0] - qy[..., 2] * qx[..., 0],
         qx[..., 0] * qy[..., 1] - qy[..., 0] * qx[..., 1]]
    # d a_i / d fx = -w_j qy_k + qy_j w_k ;  d a_i / d fy = -qx_j w_k + w_j qx_k   (j, k) = (i+1, i+2)
    dax = [-w[..., (i + 1) % 3] * qy[..., (i + 2) % 3] + qy[..., (i + 1) % 3] * w[..., (i + 2) % 3] for i in range(3)]
    day = [-qx[..., (i + 1) % 3] * w[..., (i + 2) % 3] + w[..., (i + 1) % 3] * qx[..., (i + 2) % 3] for i in range(3)]
    s_ = a[0] + a[1] + a[2]
    s_ = torch.where(hit, s_, torch.ones_like(s_))
    sx, sy = dax[0] + dax[1] + dax[2], day[0] + day[1] + day[2]
    d = lambda ai, dai, ds, scale: (dai * s_ - ai * ds) / (s_ * s_) * scale
    db = torch.stack([d(a[0], dax[0], sx, 2.0 / W), d(a[0], day[0], sy, 2.0 / H), d(a[1], dax[1], sx, 2.0 / W), d(a[1], day[1], sy, 2.0 / H)], -1)
    return torch.where(hit[..., None], db, torch.zeros_like(db))


# ---------------------------------------------------------------------------------------------- interpolate
class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, tri32):
        require_device(attr, rast, tri32, what="interpolate")
        ensure_resolved(rast)
        attr, rast = f32c(attr), f32c(rast)
        B, H, W = rast.shape[:3]
        V, C = attr.shape[1], attr.shape[2]
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=rast.device)
        call("a3d_interp_fwd", ptr(attr), attr.shape[0], C, ptr(rast), ptr(tri32), B, V, tri32.shape[0], H, W, ptr(out), stream(),
             tag=f"[C{C}]")
        ctx.save_for_backward(attr, rast, tri32)
        return out

    @staticmethod
    def backward(ctx, g_out):
        attr, rast, tri32 = ctx.saved_tensors
        B, H, W = rast.shape[:3]
        V, C = attr.shape[1], attr.shape[2]
        g_attr = torch.empty_like(attr) if ctx.needs_input_grad[0] else None
        g_rast = torch.empty_like(rast)
        call("a3d_interp_bwd", ptr(f32h(g_out)), ptr(attr), attr.shape[0], C, ptr(rast), ptr(tri32), B, V, tri32.shape[0], H, W, ptr(g_attr),
             ptr(g_rast), stream(), tag=f"[C{C}]")
        return g_attr, (g_rast if ctx.needs_input_grad[1] else None), None


def interpolate(attr, rast, tri):
    """attr [B|1,V,C] (or [V,C]) -> [B,H,W,C]."""
    if attr.dim() == 2:
        attr = attr[None]
    return _Interpolate.apply(attr, rast, tri_int32(tri))


def _selected(diff_attrs, C):
    """'all' -> None; a list of attribute indices (repeats allowed, negative = from the end) -> tuple of channels in [0, C)."""
    if isinstance(diff_attrs, str):
        if diff_attrs != "all":
            raise ValueError(f"diff_attrs must be 'all' or a list of attribute indices, not {diff_attrs!r}")
        return None
    sel = tuple(int(i) for i in (diff_attrs.tolist() if torch.is_tensor(diff_attrs) else diff_attrs))
    if any(i < -C or i >= C for i in sel):
        raise IndexError(f"diff_attrs {list(sel)} out of range for {C} attributes")
    return tuple(i % C for i in sel)


class _InterpolateDa(torch.autograd.Function):
    """a3d_interp_da_fwd / a3d_interp_da_bwd (csrc/deriv.hip): one launch each way; gradients to attr (tile scatter, zero on unselected
    channels) and rast_db.  The gradient w.r.t. rast is identically zero.  Double backward: the torch statement."""

    @staticmethod
    def forward(ctx, attr, rast, tri32, rast_db, sel):
        require_device(attr, rast, tri32, rast_db, what="interpolate_da")
        ensure_resolved(rast)
        attr_c, rast_c, db_c = f32c(attr), f32c(rast), f32c(rast_db)
        B, H, W = rast_c.shape[:3]
        V, C = attr_c.shape[1], attr_c.shape[2]
        assert attr_c.shape[0] in (1, B) and db_c.shape == (B, H, W, 4)
        S = C if sel is None else len(sel)
        sel_d = None if sel is None else torch.tensor(sel, dtype=torch.int32, device=rast_c.device)  # (kept for the backward)
        out = torch.empty((B, H, W, 2 * S), dtype=torch.float32, device=rast_c.device)
        call("a3d_interp_da_fwd", ptr(attr_c), attr_c.shape[0], C, ptr(sel_d), S, ptr(rast_c), ptr(db_c), ptr(tri32), B, V, tri32.shape[0], H, W,
             ptr(out), stream(), tag=f"[S{S}]")
        ctx.save_for_backward(attr, rast_c, tri32, rast_db, sel_d)
        ctx.sel = sel
        return out

    @staticmethod
    def backward(ctx, g_da):
        attr, rast, tri32, rast_db, sel_d = ctx.saved_tensors
        want_attr, want_db = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        if torch.is_grad_enabled():  # double backward: the torch statement, differentiated by autograd
            with torch.enable_grad():
                ins = [t for t, w in ((attr, want_attr), (rast_db, want_db)) if w]
                out = _interpolate_da_torch(attr, rast, tri32, rast_db, "all" if ctx.sel is None else list(ctx.sel))
                gs = list(torch.autograd.grad(out, ins, g_da, create_graph=True))
            return (gs.pop(0) if want_attr else None), None, None, (gs.pop(0) if want_db else None), None
        attr_c, db_c = f32c(attr), f32c(rast_db)
        B, H, W = rast.shape[:3]
        V, C = attr_c.shape[1], attr_c.shape[2]
        S = C if ctx.sel is None else len(ctx.sel)
        g_attr = torch.empty_like(attr_c) if want_attr else None
        g_db = torch.empty_like(db_c) if want_db else None
        call("a3d_interp_da_bwd", ptr(f32h(g_da)), ptr(attr_c), attr_c.shape[0], C, ptr(sel_d), S, ptr(rast), ptr(db_c), ptr(tri32), B, V,
             tri32.shape[0], H, W, ptr(g_attr), ptr(g_db), stream(), tag=f"[S{S}]")
        return g_attr, None, None, g_db, None


def interpolate_da(attr, rast, tri, rast_db, diff_attrs="all"):
    """out_da [B,H,W,2*S] = (dA/dX, dA/dY) per selected attribute (dr.interpolate's second output with ``rast_db`` / ``diff_attrs``):
    dA/dX = du/dX (A0 - A2) + dv/dX (A1 - A2), differentiable w.r.t. attr and rast_db.  CUDA float32 tensors: one HIP launch each way
    (a3d_interp_da_fwd / _bwd, csrc/deriv.hip; up to 64 attributes and 64 selected ones); anything else -- CPU tensors, float64, wider
    rows, a double backward -- evaluates the torch statement _interpolate_da_torch.  Nothing on the training path consumes it
    (render.py:24)."""
    a = attr if attr.dim() == 3 else attr[None]
    C = a.shape[-1]
    if _deriv_on_gpu(a, rast, rast_db) and tri.is_cuda and 0 < C <= _lib.DERIV_MAX_SELECTED:
        sel = _selected(diff_attrs, C)
        if sel is None or 0 < len(sel) <= _lib.DERIV_MAX_SELECTED:
            return _InterpolateDa.apply(a, rast, tri_int32(tri), rast_db, sel)
    return _interpolate_da_torch(attr, rast, tri, rast_db, diff_attrs)


def _interpolate_da_torch(attr, rast, tri, rast_db, diff_attrs="all"):
    """interpolate_da as torch operations (a [B,H,W,3,S] gather and a dozen element-wise launches; backward = autograd's index_put): the
    statement the kernels follow, the path of CPU / float64 tensors and of a double backward, and what tests and tools/bench_deriv.py
    compare against."""
    a = attr if attr.dim() == 3 else attr[None]
    sel = list(range(a.shape[-1])) if isinstance(diff_attrs, str) and diff_attrs == "all" else list(diff_attrs)
    B = rast.shape[0]
    ids = rast[..., 3].long() - 1
    hit = (ids >= 0)[..., None]
    t = tri.long()[ids.clamp(min=0)]
    A = a.expand(B, -1, -1)[torch.arange(B, device=rast.device)[:, None, None, None].expand_as(t), t][..., sel]  # [B,H,W,3,S]
    d0, d1 = A[..., 0, :] - A[..., 2, :], A[..., 1, :] - A[..., 2, :]
    dx = rast_db[..., 0:1] * d0 + rast_db[..., 2:3] * d1
    dy = rast_db[..., 1:2] * d0 + rast_db[..., 3:4] * d1
    da = torch.stack([dx, dy], -1).reshape(*dx.shape[:-1], -1)
    return torch.where(hit, da, torch.zeros_like(da))


# ---------------------------------------------------------------------------------------------- fused G-buffer
GBUFFER_GRAD_COLS = _lib.GBUFFER_GRAD_COLS


def _round_up(n, m):
    return -(-int(n) // int(m)) * int(m) if m else int(n)


class _GBuffer(torch.autograd.Function):
    """-> (rows [P,12], extra rows [P,E] | None, tex_in [Pp,3] | None, img [Pp] | None, pix [P], inv [B*H*W] | None).

    ``bucket`` > 0 (round 6): the launch also writes what the texture / feature fields take from the G-buffer in the form they take it
    (a3d_gb_aux): ``tex_in`` = the canonical positions as dense rows, padded with zero rows to a multiple of ``bucket``, and ``img`` =
    the point -> image index, padded with the last image.  The fields' input gradient then comes back as dense rows too (``g_tex`` of
    the backward): no column slice of the 12-wide rows, no pad, no padded gradient of either -- no torch kernel between this path and
    model/networks in either direction."""

    @staticmethod
    def forward(ctx, clip, v_pos, v_nrm, prior, rast, tri32, pix, extra, bucket=0):
        require_device(clip, v_pos, v_nrm, prior, rast, tri32, pix, extra, what="gbuffer")
        clip, v_pos, v_nrm, prior, rast = f32c(clip), f32c(v_pos), f32c(v_nrm), f32c(prior), f32c(rast)
        B, H, W = rast.shape[:3]
        V = v_pos.shape[1]
        assert clip.shape[:2] == (B, V) and v_pos.shape[0] == B and v_nrm.shape == v_pos.shape and prior.shape[0] in (1, B)
        listed = pix is None  # no list given: build it in the same launch (a3d_cover_gbuffer_fwd) and return it with the rows
        inv = cover_scratch = None
        dev = rast.device
        E = 0
        if extra is not None:
            extra = f32c(extra)
            E = extra.shape[2]
            assert extra.shape[:2] == (B, V) and 1 <= E <= 3
        # when a backward will follow, its gradient rows (one 64-byte row per (image, vertex), see backward) are allocated now and
        # cleared by the forward launch: one memset less on the backward path
        needs_grad = any(ctx.needs_input_grad)  # (forward runs with grad mode off: this is what says whether a backward can follow)
        rows = torch.empty((B, V, GBUFFER_GRAD_COLS), dtype=torch.float32, device=dev) if needs_grad else None
        out = extra_out = tex_in = img = None
        want_aux = ctx_wants_aux(bucket)  # (-1 / None: the rows alone)
        bucket = int(bucket) if want_aux else 0

        def aux_for(n_rows):
            """(struct or None, tex buffer, img buffer) with ``n_rows`` rows behind them."""
            if not want_aux:
                return None, None, None
            t = torch.empty((n_rows, 3), dtype=torch.float32, device=dev)
            im = torch.empty((n_rows,), dtype=torch.int64, device=dev)
            return _lib.GbAux(size=ctypes.sizeof(_lib.GbAux), tex_out=ptr(t), img_out=ptr(im), rows=n_rows, pad_to=bucket), t, im

        cap_key = (dev, B, H, W)
        pend = _pending_resolve.peek(rast) if listed else None
        if pend is not None and cap_key in _cover_last_len:
            # the raster buffer is still keys (rasterize(defer_resolve=True)): resolve, list and rows from ONE launch, the rows allocated for
            # the previous frame's list length + 25 %; the read-back of the true length comes after the launch is enqueued
            _pending_resolve.take(rast)
            cap = max(1024, -(-int(1.25 * _cover_last_len[cap_key] + 1) // 1024) * 1024)
            clip_r, tri_r = pend["clip"], pend["tri32"]
            cover_scratch = _cover_counts.peek(rast)
            pix_c = torch.empty(cap, dtype=torch.int64, device=dev)
            inv = torch.empty(B * H * W, dtype=torch.int32, device=dev)
            out_c = torch.empty((cap, 12), dtype=torch.float32, device=dev)
            extra_c = torch.empty((cap, E), dtype=torch.float32, device=dev) if extra is not None else None
            aux, tex_c, img_c = aux_for(_round_up(cap, bucket))
            call("a3d_rast_resolve_gbuffer_fwd", ptr(clip_r), clip_r.shape[0], ptr(tri_r), B, V, tri_r.shape[0], H, W, ptr(rast), ptr(pend["keys"]),
                 ptr(cover_scratch), cap, ptr(pix_c), ptr(inv), ptr(v_pos), ptr(v_nrm), ptr(prior), prior.shape[0], ptr(out_c), ptr(extra), E,
                 ptr(extra_c), ptr(rows), None if aux is None else ctypes.addressof(aux), stream())
            _rast_keys[pend["key"]] = pend["keys"]  # (every key the launch consumed is re-armed)
            nb = _lib.lib().a3d_cover_blocks(B, H, W)
            tail = _lib.read_back(cover_scratch[nb:nb + _lib.lib().a3d_cover_groups(B, H, W) * _lib.lib().a3d_cover_group_stride()])
            P = int(tail[::_lib.lib().a3d_cover_group_stride()].sum())
            resolve_events["fused"] += 1
            if int(tail[3]) != 0 or _debug_force_lookback_timeout:
                # a look-back ran out of its spin budget (never observed; it would mean work-groups were not dispatched in the order of their
                # index): offsets and sums of this launch are not to be trusted -- but the TEXELS are complete (they do not depend on the
                # look-up).  Count from the texels, take the two-launch path's second half, and stop deferring in this process.
                import warnings

                globals()["DEFER_RESOLVE"] = False
                resolve_events["timeouts"] = resolve_events.get("timeouts", 0) + 1
                warnings.warn("a3d_rast_resolve_gbuffer_fwd: look-back timed out; recovered through a3d_cover_count + a3d_cover_gbuffer_fwd, "
                              "deferred resolve switched off for this process")
                cover_scratch = torch.empty(_lib.lib().a3d_cover_scratch_bytes(B, H, W) // 4, dtype=torch.int32, device=dev)
                call("a3d_cover_count", ptr(rast), B, H, W, 8, ptr(cover_scratch), stream())
                _cover_counts.put(rast, cover_scratch)
                tail = _lib.read_back(cover_scratch[nb:nb + _lib.lib().a3d_cover_groups(B, H, W) * _lib.lib().a3d_cover_group_stride()])
                P, cap = int(tail[::_lib.lib().a3d_cover_group_stride()].sum()), -1
            _cover_last_len[cap_key] = P
            if P <= cap:
                pix, out, extra_out = pix_c[:P], out_c[:P], (extra_c[:P] if extra_c is not None else None)
                if want_aux:
                    tex_in, img = tex_c[:_round_up(P, bucket)], img_c[:_round_up(P, bucket)]
            else:  # outgrown: texels, block counts and sums are complete -- the exact list + rows through the two-launch path's second half
                resolve_events["outgrown"] += 1
                pix = torch.empty(P, dtype=torch.int64, device=dev)
        elif listed:
            cover_scratch, P = _cover_counted(rast, 8)  # (resolves a deferred buffer first)
            _cover_last_len[cap_key] = P
            pix = torch.empty(P, dtype=torch.int64, device=dev)
            inv = torch.empty(B * H * W, dtype=torch.int32, device=dev)
        P = pix.shape[0]
        assert pix.dtype == torch.int64 and pix.is_contiguous()
        fused_done = out is not None
        if out is None:
            out = torch.empty((P, 12), dtype=torch.float32, device=dev)
            if extra is not None:
                extra_out = torch.empty((P, E), dtype=torch.float32, device=dev)
        if fused_done:
            pass
        elif listed:
            aux, tex_in, img = aux_for(_round_up(P, bucket))
            call("a3d_cover_gbuffer_fwd", ptr(rast), ptr(tri32), B, V, tri32.shape[0], H, W, ptr(cover_scratch), P, ptr(pix), ptr(inv), ptr(v_pos),
                 ptr(v_nrm), ptr(prior), prior.shape[0], ptr(out), ptr(extra), E, ptr(extra_out), ptr(rows),
                 None if aux is None else ctypes.addressof(aux), stream())
        else:
            aux, tex_in, img = aux_for(_round_up(P, bucket))
            call("a3d_gbuffer_fwd", ptr(rast), ptr(tri32), ptr(pix), P, ptr(v_pos), ptr(v_nrm), ptr(prior), prior.shape[0], B, V, tri32.shape[0], H, W,
                 ptr(out), ptr(extra), E, ptr(extra_out), ptr(rows), None if aux is None else ctypes.addressof(aux), stream())
        ctx.save_for_backward(clip, v_pos, v_nrm, prior, rast, tri32, pix, extra)
        ctx.rows = rows
        ctx.set_materialize_grads(False)
        nondiff = [t for t in (img, pix if listed else None, inv) if t is not None]
        if nondiff:
            ctx.mark_non_differentiable(*nondiff)
        return out, extra_out, tex_in, img, (pix if listed else None), inv

    @staticmethod
    def backward(ctx, g_out, g_extra_out=None, g_tex=None, *_):
        clip, v_pos, v_nrm, prior, rast, tri32, pix, extra = ctx.saved_tensors
        B, H, W = rast.shape[:3]
        V, P = v_pos.shape[1], pix.shape[0]
        want_prior, want_clip = ctx.needs_input_grad[3], ctx.needs_input_grad[0]
        E = 0 if extra is None else extra.shape[2]
        if extra is not None and g_extra_out is None:
            g_extra_out = torch.zeros((P, E), dtype=torch.float32, device=rast.device)
        if g_out is None:  # (only the fields' input had a gradient)
            g_out = torch.zeros((P, 12), dtype=torch.float32, device=rast.device)
        # one 64-byte gradient row per (image, vertex): the kernel's atomics of a vertex are then one line request; the gradients are
        # strided views of the rows (a3d.h: v_pos 0..2 | v_nrm 3..5 | canonical 6..8 | extra 9..11 | clip 12..15)
        rows, ctx.rows = ctx.rows, None  # the rows the forward cleared serve ONE backward (their views are handed out as gradients)
        clear = rows is not None
        if rows is None:
            rows = torch.empty((B, V, GBUFFER_GRAD_COLS), dtype=torch.float32, device=rast.device)
        call("a3d_gbuffer_bwd", ptr(f32h(g_out)), ptr(rast), ptr(tri32), ptr(pix), P, ptr(v_pos), ptr(v_nrm), ptr(prior), prior.shape[0],
             ptr(clip) if want_clip else None, B, V, tri32.shape[0], H, W, ptr(rows), int(clear), int(want_prior), ptr(extra), E,
             None if extra is None else ptr(f32h(g_extra_out)), None if g_tex is None else ptr(f32h(g_tex)), stream())
        g_vpos, g_vnrm = rows[..., 0:3], rows[..., 3:6]
        g_clip = rows[..., 12:16] if want_clip else None
        g_prior = None
        if want_prior:
            if prior.shape[0] == 1:  # shared canonical mesh: the per-image partials summed by one small launch
                g_prior = torch.empty((1, V, 3), dtype=torch.float32, device=rast.device)
                call("a3d_gbuffer_prior_grad", ptr(rows), B, V, ptr(g_prior), stream())
            else:
                g_prior = rows[..., 6:9]
        g_extra = rows[..., 9:9 + E] if (extra is not None and ctx.needs_input_grad[7]) else None
        return g_clip, g_vpos, g_vnrm, g_prior, None, None, None, g_extra, None


def ctx_wants_aux(bucket):
    return bucket is not None and int(bucket) >= 0


def covered_gbuffer(clip, v_pos, v_nrm, prior_v_pos, rast, tri, extra=None, field_inputs=None):
    """covered_pixels(rast, return_inverse=True) + gbuffer(...) as ONE launch: (gb [P,12][, extra [P,E]], pix [P], inv [B*H*W]).
    H and W must be multiples of 8 (the tile-ordered list).
    ``field_inputs`` = bucket size (0 = no padding): also (tex_in [Pp,3], img [Pp]) -- see _GBuffer -- appended to the result."""
    assert rast.shape[1] % 8 == 0 and rast.shape[2] % 8 == 0
    gb, ex, tex_in, img, pix, inv = _GBuffer.apply(clip, v_pos, v_nrm, prior_v_pos, f32c(rast.detach()), tri_int32(tri), None, extra,
                                                   -1 if field_inputs is None else int(field_inputs))
    res = (gb, pix, inv) if extra is None else (gb, ex, pix, inv)
    return res if field_inputs is None else res + (tex_in, img)


def gbuffer(clip, v_pos, v_nrm, prior_v_pos, rast, tri, pix, extra=None):
    """[P,12] = world position | face normal | smooth normal | canonical position at the covered pixels ``pix``; with ``extra`` [B,V,E<=3]
    also that attribute interpolated to [P,E] (returns a pair).

    Differentiable w.r.t. v_pos, v_nrm, prior_v_pos, extra and -- through the barycentrics -- clip (x, y, w); pass ``rast.detach()``
    semantics are implied: the gradient to ``clip`` is produced here, not through ``rast``.
    """
    gb, ex = _GBuffer.apply(clip, v_pos, v_nrm, prior_v_pos, rast.detach(), tri_int32(tri), pix, extra, -1)[:2]
    return gb if extra is None else (gb, ex)


# ---------------------------------------------------------------------------------------------- per-point shading
class _ShadePoints(torch.autograd.Function):
    """(shading normal [P,3], shading [P,1], shaded [P,3]) from the G-buffer rows, the camera/light rows and kd."""

    @staticmethod
    def forward(ctx, gb, par, kd, two_sided, img):
        require_device(gb, par, img, what="shade_points")
        gb, par = f32c(gb), f32c(par)
        P, ncol = gb.shape[0], par.shape[1]
        assert gb.shape == (P, 12) and ncol in (12, 17) and (kd is not None) == (ncol == 17)
        assert par.shape[0] == P if img is None else (img.shape == (P,) and img.dtype == torch.int64 and img.is_contiguous())
        _assert_sorted(img)
        nrm = torch.empty((P, 3), dtype=torch.float32, device=gb.device)
        shading = shaded = None
        kd_stride = 0
        if kd is not None:
            assert kd.shape == (P, 3) and kd.dtype == torch.float32
            if kd.stride(1) != 1:
                kd = kd.contiguous()
            kd_stride = kd.stride(0)
            shading = torch.empty((P, 1), dtype=torch.float32, device=gb.device)
            shaded = torch.empty((P, 3), dtype=torch.float32, device=gb.device)
        # per-image rows: their gradient is accumulated by the backward with atomics -- allocated now, cleared by the forward launch
        g_par = torch.empty_like(par) if (img is not None and ctx.needs_input_grad[1]) else None
        call("a3d_shade_fwd", ptr(gb), ptr(par), ncol, ptr(img), ptr(kd), kd_stride, P, int(two_sided), ptr(nrm), ptr(shading), ptr(shaded),
             ptr(g_par), par.shape[0], stream())
        ctx.save_for_backward(gb, par, kd, img)
        ctx.g_par = g_par
        ctx.two_sided, ctx.kd_stride = int(two_sided), kd_stride
        ctx.set_materialize_grads(False)  # (an output nobody differentiated arrives as None = a NULL pointer, not as a tensor of zeros filled for it)
        if kd is None:
            return nrm
        return nrm, shading, shaded

    @staticmethod
    def backward(ctx, g_nrm, g_shading=None, g_shaded=None):
        gb, par, kd, img = ctx.saved_tensors
        P, ncol = gb.shape[0], par.shape[1]
        g_gb = torch.empty_like(gb)
        g_par, ctx.g_par = ctx.g_par, None  # (cleared by the forward launch; serves one backward)
        clear = g_par is not None
        if g_par is None:
            g_par = torch.empty_like(par)
        g_kd = torch.empty((P, 3), dtype=torch.float32, device=gb.device) if kd is not None else None
        opt = lambda t: None if t is None else f32h(t)
        call("a3d_shade_bwd", ptr(opt(g_nrm)), ptr(opt(g_shading)), ptr(opt(g_shaded)), ptr(gb), ptr(par), ncol, ptr(img), par.shape[0], ptr(kd),
             ctx.kd_stride, P, ctx.two_sided, ptr(g_gb), ptr(g_par), ptr(g_kd), int(clear), stream())
        return g_gb, g_par, g_kd, None, None


def shade_points(gb, par, kd=None, two_sided=True, img=None):
    """Shading normal, Lambert shading and shaded colour at the covered pixels (csrc/shade.hip).

    gb [P,12] from :func:`gbuffer`; par rows (w2c rotation 9, view position 3[, light direction 3, ambient, diffuse]): one per point
    [P,12|17], or -- with ``img`` [P] (point -> image, int64, non-decreasing) -- one per image [B,12|17], in which case their gradient is
    reduced per image inside the backward kernel; kd [P,3] (any row stride).  Returns nrm, or (nrm, shading [P,1], shaded [P,3]) when a
    light is given."""
    return _ShadePoints.apply(gb, par, kd, two_sided, img)


KEEP_SHADED_COLOUR = os.environ.get("A3D_KEEP_SHADED", "1") != "0"  # the compositor keeps the colours it computes on the fly for its blend launch and its backward


class ShadeRecipe:
    """The shaded colour of a fused render, NOT computed yet: what it is computed from.  Handed to shade_composite_antialias the colour of
    every covered pixel is computed inside the compositor's launches (a3d_ca_shade) and the whole backward -- compositor gather, shading
    adjoint -- is ONE autograd node that writes the gradients of the G-buffer rows, of the texture field's output rows and of the camera
    / light tensors where their consumers read them (round 6; a3d_shade_fwd / a3d_shade_bwd and the [B,17] table, its cat and the slices
    around them are not part of that path).  Any other reader calls ``materialize()``: the classic ops.shade_points on the same inputs.

    gb [P,12]; w2c [1|B,4,4] (or [.,3,3]); view_pos [1|B,3]; light [1|B,5] = DirectionalLight.forward(feat) (direction 3, ambient,
    diffuse); all_tex [>= P, >= 3]: the texture field's output rows, kd = columns 0..2 (rows past P: padding, never read)."""

    def __init__(self, gb, w2c, view_pos, light, all_tex, two_sided, img):
        self.gb, self.w2c, self.view_pos, self.light, self.all_tex, self.two_sided, self.img = gb, w2c, view_pos, light, all_tex, bool(two_sided), img
        self.outs = None

    def per_image(self):
        """The [B,17] table of a3d_shade_fwd (rotation 9 | view 3 | light 5) from the same tensors (torch ops: the unfused path)."""
        b = max(self.w2c.shape[0], self.view_pos.shape[0], self.light.shape[0])
        return torch.cat([self.w2c[:, :3, :3].reshape(-1, 9).expand(b, 9), self.view_pos.reshape(-1, 3).expand(b, 3), self.light.expand(b, 5)], dim=-1)

    def materialize(self):
        """(shading normal [P,3], shading [P,1], shaded colour [P,3]) through the stand-alone launch."""
        if self.outs is None:
            P = self.gb.shape[0]
            self.outs = shade_points(self.gb, self.per_image(), self.all_tex[:P, :3], self.two_sided, img=self.img[:P])
        return self.outs


# ---------------------------------------------------------------------------------------------- per-image rows <-> points
class _RowsPerPoint(torch.autograd.Function):
    """t[img] for a per-image tensor t [B,C] and a point -> image map img [P]; backward = per-image segment sums (csrc/segsum.hip)
    instead of index_add's P x C float atomics onto B rows."""

    @staticmethod
    def forward(ctx, t, img):
        ctx.save_for_backward(img)
        ctx.b = t.shape[0]
        return t.index_select(0, img)

    @staticmethod
    def backward(ctx, g):
        (img,) = ctx.saved_tensors
        g = f32c(g)
        P, C = g.shape[0], int(math.prod(g.shape[1:]))
        out = torch.empty((ctx.b,) + tuple(g.shape[1:]), dtype=torch.float32, device=g.device)
        call("a3d_rows_segsum", ptr(g), ptr(img), P, C, ctx.b, ptr(out), stream(), tag=f"[C{C}]")
        return out, None


CHECK_SORTED_INDEX = False  # debugging aid: device-side assert (no host sync) that a point -> image index is non-decreasing


def _assert_sorted(img):
    """The per-image segment sums (csrc/segsum.hip) treat a 128-row block whose first and last rows belong to the same image as
    single-image: the index must be non-decreasing (the render path's is: pixel lists are image-major, padding rows repeat the LAST
    image).  A list that breaks the contract is summed wrongly without a sign -- one of at most 128 rows that starts and ends in image 0
    with other images in between goes to image 0 whole -- and this check, when switched on, is what reports it."""
    if CHECK_SORTED_INDEX and img is not None and img.numel() > 1:
        torch._assert_async((img[1:] >= img[:-1]).all(), "point -> image index must be non-decreasing")


def rows_per_point(t, img):
    """t [B,...] -> [P,...] rows gathered by img [P] (int64, contiguous, NON-DECREASING: see _assert_sorted)."""
    require_device(t, img, what="rows_per_point")
    _assert_sorted(img)
    return _RowsPerPoint.apply(t, img) if (t.requires_grad and torch.is_grad_enabled()) else t.index_select(0, img)


class _RowsAddReLU(torch.autograd.Function):
    """relu(y + rows[img]) computed in place on y (the output of a GEMM over the point list)."""

    @staticmethod
    def forward(ctx, y, rows, img):
        require_device(y, rows, img, what="rows_add_relu")
        assert y.is_contiguous() and y.dtype == torch.float32 and y.dim() == 2 and rows.shape[1] == y.shape[1] and img.shape[0] == y.shape[0]
        rows = f32c(rows)
        call("a3d_rows_add_relu_fwd", ptr(y), ptr(rows), ptr(img), y.shape[0], y.shape[1], rows.shape[0], stream(), tag=f"[C{y.shape[1]}]")
        ctx.mark_dirty(y)
        ctx.save_for_backward(y, img)
        ctx.b = rows.shape[0]
        return y

    @staticmethod
    def backward(ctx, g):
        y, img = ctx.saved_tensors
        g = f32c(g)
        g_pre = torch.empty_like(g)
        g_rows = torch.empty((ctx.b, y.shape[1]), dtype=torch.float32, device=g.device)
        call("a3d_rows_add_relu_bwd", ptr(g), ptr(y), ptr(img), y.shape[0], y.shape[1], ctx.b, ptr(g_pre), ptr(g_rows), stream(),
             tag=f"[C{y.shape[1]}]")
        return g_pre, g_rows, None


def _rows_args(what, y, rows, img, in_place=True):
    """Shapes and types of a point list y [P,C], per-image rows [B,C] (or B itself) and the point -> image index: the entry points take
    raw pointers, so what they would misread is refused here -- shapes and types first (ValueError), then the device (A3DError)."""
    b = rows if isinstance(rows, int) else (rows.shape[0] if rows.dim() == 2 else -1)
    if y.dim() != 2 or y.shape[1] < 1 or b < 1 or (not isinstance(rows, int) and rows.shape[1] != y.shape[1]):
        raise ValueError(f"{what}: expected a point list [P,C] with C >= 1 and B >= 1 per-image rows [B,C], got {list(y.shape)} and "
                         f"{rows if isinstance(rows, int) else list(rows.shape)}")
    if img.dtype != torch.int64 or img.dim() != 1 or img.shape[0] != y.shape[0] or not img.is_contiguous():
        raise ValueError(f"{what}: the point -> image index must be int64, contiguous and [P] = [{y.shape[0]}], got {img.dtype} {list(img.shape)} "
                         f"with strides {list(img.stride())}")
    if in_place and (y.dtype != torch.float32 or not y.is_contiguous()):
        raise ValueError(f"{what}: the point list is written in place and must be float32 and contiguous, got {y.dtype} with strides {list(y.stride())}")
    require_device(y, None if isinstance(rows, int) else rows, img, what=what)


def rows_add_relu_raw_(y, rows, img):
    """In place, no autograd: y[p] = relu(y[p] + rows[img[p]]) (used inside hostnets' stack Function)."""
    _rows_args("rows_add_relu_raw_", y, rows, img)
    call("a3d_rows_add_relu_fwd", ptr(y), ptr(f32h(rows)), ptr(img), y.shape[0], y.shape[1], rows.shape[0], stream(), tag=f"[C{y.shape[1]}]")
    return y


def rows_segsum_raw(g, img, b):
    """[B,C] per-image sums of g [P,C] (no autograd); img non-decreasing."""
    _rows_args("rows_segsum_raw", g, int(b), img, in_place=False)
    _assert_sorted(img)
    g = f32c(g)
    out = torch.empty((b, g.shape[1]), dtype=torch.float32, device=g.device)
    call("a3d_rows_segsum", ptr(g), ptr(img), g.shape[0], g.shape[1], b, ptr(out), stream(), tag=f"[C{g.shape[1]}]")
    return out


def rows_add_relu_(y, rows, img):
    """In place: y[p] = relu(y[p] + rows[img[p]]);  y [P,C] fresh GEMM output, rows [B,C], img int64 [P], non-decreasing."""
    _rows_args("rows_add_relu_", y, rows, img)
    _assert_sorted(img)
    return _RowsAddReLU.apply(y, rows, img)


# ---------------------------------------------------------------------------------------------- antialias
class AAAnalysis:
    """Silhouette-crossing work list for one (rast, clip, topology); shared by every colour buffer.
    ``defer``: do not launch now -- the first composite_antialias over this analysis runs it inside its own first launch (possible when
    the rasteriser prepared the screen positions and counters for this clip); every other consumer calls ensure() first."""

    def __init__(self, rast, clip, topo: AATopology, defer=False):
        require_device(rast, clip, what="antialias")
        ensure_resolved(rast)  # (one dictionary miss when nothing is pending -- the render path resolves in its G-buffer launch before this)
        self.rast, self.clip, self.topo = f32c(rast.detach()), f32c(clip.detach()), topo
        B, H, W = rast.shape[:3]
        self.B, self.H, self.W = B, H, W
        shards = _lib.lib().a3d_aa_shards()  # the work list is kept in segments, each with its own append counter
        self.capacity = _lib.lib().a3d_aa_capacity(B, H, W)
        dev = rast.device
        self.work = torch.empty((self.capacity, 4), dtype=torch.int32, device=dev)
        prep = _aa_prepared.take(self.rast)  # (one analysis per prepared pair: the counters are consumed)
        self.prepared = prep is not None and prep[0] == _IdentityCache.key(self.clip)
        if self.prepared:
            self.screen, self.count = prep[1], prep[2]
        else:
            self.count = torch.empty((shards,), dtype=torch.int32, device=dev)
            self.screen = torch.empty((self.clip.shape[0], self.clip.shape[1], 2), dtype=torch.float32, device=dev)
        self.pending = True
        if not (defer and self.prepared and topo.tri.shape[0] > 0):
            self.ensure()

    def ride_args(self):
        """The a3d_aa_ride struct that makes a3d_composite_aa_fwd / a3d_mask_aa_fwd run the pending analysis in their first launch, or None.  The caller marks the
        analysis done (``pending = False``) once that call has SUCCEEDED: a refused call must not leave an unfilled work list behind
        that later consumers would take for finished.  Batches the riding form cannot address (B > 65535) run stand-alone now."""
        if self.pending and self.B > 65535:
            self.ensure()
        if not self.pending:
            return None
        topo, lists = self.topo, getattr(self.topo, "lists", None)
        return _lib.AaRide(size=ctypes.sizeof(_lib.AaRide), clip_batch=self.clip.shape[0], rast=ptr(self.rast), screen=ptr(self.screen),
                           tri=ptr(topo.tri), opp=ptr(topo.opp), off=ptr(None if lists is None else lists.off),
                           adj=ptr(None if lists is None else lists.adj), V=self.clip.shape[1], F=topo.tri.shape[0],
                           lists_stride=0 if lists is None else lists.stride)

    def ensure(self):
        """Run the analysis now if it has not run yet (stand-alone launch)."""
        if not self.pending:
            return self
        self.pending = False
        topo, lists = self.topo, getattr(self.topo, "lists", None)
        call("a3d_aa_analyze", ptr(self.rast), ptr(self.clip), self.clip.shape[0], ptr(topo.tri), ptr(topo.opp), self.B, self.clip.shape[1],
             topo.tri.shape[0], self.H, self.W, ptr(self.screen), ptr(self.work), self.capacity, ptr(self.count), int(self.prepared),
             ptr(None if lists is None else lists.off), ptr(None if lists is None else lists.adj), 0 if lists is None else lists.stride, stream())
        return self


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, clip, analysis):
        require_device(color, what="antialias")
        color = f32c(color)
        a = analysis.ensure()
        B, H, W, C = color.shape
        assert (B, H, W) == (a.B, a.H, a.W)
        out = torch.empty_like(color)
        call("a3d_aa_fwd", ptr(color), C, ptr(a.work), ptr(a.count), a.capacity, B, H, W, ptr(out), stream(), tag=f"[C{C}]")
        ctx.save_for_backward(color)
        ctx.analysis = a
        return out

    @staticmethod
    def backward(ctx, g_out):
        (color,) = ctx.saved_tensors
        a = ctx.analysis
        B, H, W, C = color.shape
        g_color = torch.empty_like(color)
        g_clip = torch.empty_like(a.clip)
        call("a3d_aa_bwd", ptr(f32h(g_out)), ptr(color), C, ptr(a.work), ptr(a.count), a.capacity, ptr(a.clip), a.clip.shape[0], ptr(a.topo.tri),
             B, a.clip.shape[1], a.topo.tri.shape[0], H, W, ptr(g_color), ptr(g_clip), stream(), tag=f"[C{C}]")
        return g_color, g_clip, None


def _image_gradient_in_place(g, H, W):
    """(tensor, floats between two pixels, channels) of an NHWC image gradient, read where it is when its pixels are evenly strided (a
    channel slice of a wider image: the losses write the gradient of 'dino_pred' into the 17-channel layout of the image it was sliced
    from), else a contiguous copy."""
    ok = g.dtype == torch.float32 and g.dim() == 4 and (g.shape[3] == 1 or g.stride(3) == 1) and g.stride(2) >= g.shape[3]
    ok = ok and (g.shape[1] == 1 or g.stride(1) == W * g.stride(2)) and (g.shape[0] == 1 or g.stride(0) == H * W * g.stride(2))
    if not ok:
        g = f32c(g)
    return g, g.stride(2), g.shape[3]


class _CaBuf:
    """One buffer of a compositor call, first or second alike: rows ``vals`` [>= P,C] (None: the call computes them itself, ``C`` given),
    ``null_vals`` [B,C] (supersampled calls only), ``background`` [1|B,h,w,<= C+1] or None, on the grid (B, h, w) of the images.  The only
    place that builds an a3d_ca_buffer.  The description holds numbers only: ``of`` hands the normalised tensors back, the node saves
    them and passes them in again.

    ``keep``: leading channels of the composited image that are materialised and handed out (None = all C + 1): render_mesh returns
    'dino_pred' and 'flow' without their alpha channel (render.py:320-331) -- here that channel is never written, the image comes out
    contiguous in the channels the caller keeps, and its gradient arrives without a SliceBackward (a zero fill and a strided copy of the
    whole image) in front of it.
    ``vals`` may have MORE rows than the list (the fields' padded point list): the extra rows are never read and their gradient rows are
    written as zeros by the same launches.
    ``bg_grad``: the background is a differentiable input of the node (spp 1 only): the backward allocates its gradient and asks the
    library for it (a3d_ca_buffer.g_null at spp 1); False: nothing is allocated and nothing more is launched."""
    __slots__ = ("C", "k", "rows", "grid", "spp", "bg_grad")

    @staticmethod
    def of(vals, null_vals, background, keep, grid, P, spp, C=None, bg_grad=False):
        """(description, (vals, null_vals, background) as float32 contiguous tensors); ``spp``: None or (s, aa)."""
        B, h, w = grid
        if vals is not None:
            vals = f32c(vals)
            assert vals.shape[0] >= P
            C = vals.shape[1]
        if spp is not None:
            null_vals = f32c(null_vals)
            assert null_vals.shape == (B, C)
        if background is not None:
            background = f32c(background)
            assert background.shape[1:3] == (h, w) and background.shape[3] <= C + 1 and background.shape[0] in (1, B)
        b = _CaBuf()
        b.C, b.k, b.rows, b.grid, b.spp = C, (C + 1 if keep is None else int(keep)), (P if vals is None else vals.shape[0]), grid, spp
        b.bg_grad = bool(bg_grad)
        assert 1 <= b.k <= C + 1 and not (b.bg_grad and (background is None or spp is not None))
        return b, (vals, null_vals, background)

    def struct(self, tensors, rast_full):
        vals, null_vals, bg = tensors
        st = _lib.CaBuffer(size=ctypes.sizeof(_lib.CaBuffer), C=self.C, vals=ptr(vals), bg=ptr(bg), bg_batch=0 if bg is None else bg.shape[0],
                           bg_channels=0 if bg is None else bg.shape[3])
        if self.spp is not None:  # (at spp 1 the supersampling fields stay zero: the library tells the modes apart by them)
            st.spp, st.aa = self.spp
            st.cover_rast, st.null_vals = ptr(rast_full), ptr(null_vals)
        return st

    def forward(self, tensors, rast_full, dev):
        """(the struct of the forward call, ``out``: only the channels handed out are materialised)."""
        out = torch.empty(self.grid + (self.k,), dtype=torch.float32, device=dev)
        st = self.struct(tensors, rast_full)
        st.out, st.out_channels = ptr(out), self.k
        return st, out

    def backward(self, tensors, g_out, rast_full, dev):
        """(the struct of the backward call, g_vals, g_null or None, the gradient image the struct points to, g_bg or None) for the saved
        ``tensors`` and the incoming gradient ``g_out``."""
        if g_out is None:
            # an output nobody differentiated: zeros in the shape of the image that was handed out, which is what autograd itself would
            # materialise (k channels; the channels past g_channels have no gradient anyway)
            g_out = torch.zeros(self.grid + (self.k,), dtype=torch.float32, device=dev)
        g_out, gs, gc = _image_gradient_in_place(g_out, self.grid[1], self.grid[2])
        g_vals = torch.empty((self.rows, self.C), dtype=torch.float32, device=dev)
        st = self.struct(tensors, rast_full)
        st.g_out, st.g_vals, st.g_stride, st.g_channels, st.vals_rows = ptr(g_out), ptr(g_vals), gs, gc, self.rows
        g_null = None
        if self.spp is not None:
            g_null = torch.empty_like(tensors[1])
            st.g_null = ptr(g_null)
        g_bg = None
        if self.bg_grad:  # (fully written by the call, its zeros included)
            g_bg = torch.empty_like(tensors[2])
            st.g_null = ptr(g_bg)  # (at spp 1 the field is the background's gradient: a3d.h)
        return st, g_vals, g_null, g_out, g_bg

    def tag(self, cut):
        """'C17', or 'C17>16' for a 17-channel composite of which 16 channels are materialised (``cut``: the tag says so)."""
        return f"C{self.C + 1}>{self.k}" if cut and self.k != self.C + 1 else f"C{self.C + 1}"


class _Source:
    """What the first buffer of a compositor call is made of.  Stateless: what a call must remember goes on its ``ctx`` or into the saved
    tensors.  ``forward`` -> (a3d_ca_shade of the forward call or None, the rows the call computes and keeps as the backward's value rows,
    further non-differentiable outputs, tensors to save); ``backward`` -> (a3d_ca_shade of the backward call or None, what ``finish``
    needs); ``finish`` -> the tail of the backward: the gradients of (gb, w2c, view, light, all_tex).  This one: plain value rows."""
    C = None  # channels of the first buffer when the call computes its rows
    name = None  # stands for the first buffer in the tag
    cut_in_tag = True  # a buffer's cut channels show in the tag ('C17>16')
    suffix = ""  # of the forward's tag
    what = "composite_antialias"

    def forward(self, ctx, tensors, pix, grid, dev):
        return None, None, (), ()

    def backward(self, ctx, kept, saved, pix, dev):
        return None, None

    def finish(self, ctx, state, g_vals, saved, pix, grid, dev):
        return (None,) * 5


class _Shaded(_Source):
    """The colour is kd * shading of a ShadeRecipe's tensors, computed inside the launches; the backward runs the shading adjoint too
    (a3d_shade_bwd_rows): g_gb [P,12], the gradient of the texture field's output rows [rows,T] and of w2c / view_pos / light in their
    own layouts."""
    C = 3
    suffix = "[+shade]"

    def __init__(self, two_sided):
        self.two_sided = int(two_sided)

    def forward(self, ctx, tensors, pix, grid, dev):
        gb, w2c, view, light, all_tex = tensors
        assert light is not None
        B, P = grid[0], pix.shape[0]
        ctx.view_shape = view.shape
        gb, w2c, view, light, all_tex = f32c(gb), f32c(w2c), f32c(view.reshape(-1, 3)), f32c(light), f32c(all_tex)
        assert gb.shape == (P, 12) and all_tex.shape[0] >= P and all_tex.shape[1] >= 3 and w2c.shape[1] == w2c.shape[2] and w2c.shape[1] in (3, 4)
        assert all(t.shape[0] in (1, B) for t in (w2c, view, light)) and light.shape[1] == 5
        # gradients of the per-image tensors: accumulated by the backward with atomics into ONE buffer (cleared by the forward's
        # first launch), handed out as views in the tensors' own shapes
        ctx.g_par = g_par = None
        if any(ctx.needs_input_grad[8:11]):
            ctx.g_par = g_par = torch.empty(w2c.numel() + view.numel() + light.numel(), dtype=torch.float32, device=dev)
        par = _shade_params(w2c, view, light)
        # (the colours the compose launch computes are kept, 12 B per point: the blend launch and the backward read them as value rows)
        kept = torch.empty((P, 3), dtype=torch.float32, device=dev) if KEEP_SHADED_COLOUR else None
        sh = _lib.CaShade(size=ctypes.sizeof(_lib.CaShade), kd_stride=all_tex.stride(0), gb=ptr(gb), par=None, kd=ptr(all_tex), clear=ptr(g_par),
                          n_clear=0 if g_par is None else g_par.numel(), two_sided=self.two_sided, params=ctypes.addressof(par), shaded_out=ptr(kept))
        sh.holds = par  # (``params`` is its address)
        return sh, kept, (), (gb, w2c, view, light, all_tex)

    def backward(self, ctx, kept, saved, pix, dev):
        gb, w2c, view, light, all_tex = saved
        par = _shade_params(w2c, view, light)
        if kept is not None:
            return None, par
        # (no kept colours: the backward's kernels re-derive them from the recipe)
        return _lib.CaShade(size=ctypes.sizeof(_lib.CaShade), kd_stride=all_tex.stride(0), gb=ptr(gb), par=None, kd=ptr(all_tex), clear=None, n_clear=0,
                            two_sided=self.two_sided, params=ctypes.addressof(par)), par

    def finish(self, ctx, par, g_vals, saved, pix, grid, dev):
        # the shading adjoint in the same node: g_vals -> G-buffer rows, texture rows (kd columns; the other columns and the padding rows
        # zero), camera / light tensors -- each in the layout its consumer reads
        gb, w2c, view, light, all_tex = saved
        g_par, ctx.g_par = ctx.g_par, None  # (cleared by the forward's first launch; serves ONE backward)
        if g_par is None:
            g_par = torch.zeros(w2c.numel() + view.numel() + light.numel(), dtype=torch.float32, device=dev)
        n0, n1 = w2c.numel(), w2c.numel() + view.numel()
        g_w2c, g_view, g_light = g_par[:n0].view(w2c.shape), g_par[n0:n1].view(view.shape), g_par[n1:].view(light.shape)
        g_struct = _shade_params(g_w2c, g_view, g_light)
        g_gb = torch.empty_like(gb)
        g_tex = torch.empty_like(all_tex)
        call("a3d_shade_bwd_rows", ptr(g_vals), ptr(gb), ctypes.addressof(par), ctypes.addressof(g_struct), ptr(pix), grid[1] * grid[2], ptr(all_tex),
             all_tex.stride(0), pix.shape[0], self.two_sided, ptr(g_gb), ptr(g_tex), all_tex.shape[1], all_tex.shape[0], stream())
        return g_gb, g_w2c, g_view.view(ctx.view_shape), g_light, g_tex


class _Depth(_Source):
    """The 'depth' render mode (a3d_ca_shade.depth_*, csrc/antialias.hip): per-image range over the point list, one normalised value per
    point, composited over zeros and antialiased by the same call; the backward runs the compositor's gather and blend adjoints and then
    the range / normalisation adjoint -> g_gb [P,12] (position columns only).  Further output: the [P] depth rows, not differentiable.
    (The mode is cut to 1 channel, render.py:324-325: the alpha is never written.)"""
    C = 1
    name = "depth"
    cut_in_tag = False
    what = "depth_composite_antialias"

    def forward(self, ctx, tensors, pix, grid, dev):
        B, P = grid[0], pix.shape[0]
        gb, w2c = f32c(tensors[0]), f32c(tensors[1])
        assert gb.shape == (P, 12) and w2c.dim() == 3 and w2c.shape[1:] == (4, 4) and w2c.shape[0] in (1, B)
        rows = torch.empty((P,), dtype=torch.float32, device=dev)
        state = torch.empty((B, 8), dtype=torch.int32, device=dev)
        return _depth_source(gb, w2c, pix, state, rows, None), None, (rows,), (gb, w2c, rows, state)

    def backward(self, ctx, kept, saved, pix, dev):
        gb, w2c, rows, state = saved
        g_gb = torch.empty_like(gb)
        slots = torch.empty((pix.shape[0], 4), dtype=torch.float32, device=dev)  # (cleared by the call)
        return _depth_source(gb, w2c, pix, state, rows, g_gb, slots), (g_gb, slots)

    def finish(self, ctx, state, g_vals, saved, pix, grid, dev):
        return (state[0], None, None, None, None)


_ROWS, _DEPTH, _SHADED = _Source(), _Depth(), (_Shaded(False), _Shaded(True))


class _Compositor(torch.autograd.Function):
    """The fused compositor (a3d_composite_aa_fwd / _bwd): one or two buffers (vals2 None = one) against the same pixel list and crossing
    records, in the same launches.  ``src`` (a _Source) says what the first buffer is made of.  ``opts`` = (pix, inv, background,
    background2, analysis, keep, keep2, spp): what autograd need not see -- a background that requires grad comes as ``bg_diff`` /
    ``bg2_diff`` instead (spp 1 only; its entry in ``opts`` is then None) and gets the adjoint of the uncovered pixels back
    (a3d_ca_buffer.g_null at spp 1); ``spp`` = (s, aa) puts the call in supersampled mode
    (a3d_ca_buffer.spp > 1): rows and backgrounds on the SHADING grid [B,h,w], composited with the coverage of ``rast_full``,
    antialiased with the full-resolution crossing records and averaged per s x s block -- without any full-resolution image -- with the
    per-image null rows as further differentiable inputs.  Returns (image, second image or None) + the source's further outputs."""

    @staticmethod
    def forward(ctx, src, opts, vals, null_vals, vals2, null_vals2, clip, gb, w2c, view, light, all_tex, rast_full, bg_diff=None, bg2_diff=None):
        pix, inv, bg, bg2, a, keep, keep2, spp = opts
        assert (bg is None or bg_diff is None) and (bg2 is None or bg2_diff is None) and (spp is None or (bg_diff is None and bg2_diff is None))
        ask, ask2 = bg_diff is not None and ctx.needs_input_grad[13], bg2_diff is not None and ctx.needs_input_grad[14]
        ctx.bg_dtypes = (None if bg_diff is None else bg_diff.dtype, None if bg2_diff is None else bg2_diff.dtype)
        bg, bg2 = (bg if bg_diff is None else bg_diff), (bg2 if bg2_diff is None else bg2_diff)
        require_device(vals, null_vals, vals2, null_vals2, pix, inv, rast_full, gb, w2c, all_tex, bg_diff, bg2_diff,
                       what=src.what if spp is None else "msaa_composite_antialias")
        P, dev = pix.shape[0], pix.device
        grid = (a.B, a.H, a.W)
        assert src.C is None or (vals is None and spp is None)
        if spp is not None:
            a.ensure()  # (the riding analysis is an spp 1 optimisation)
            s = int(spp[0])
            assert 2 <= s <= 8 and a.H % s == 0 and a.W % s == 0
            grid, rast_full, spp = (a.B, a.H // s, a.W // s), f32c(rast_full.detach()), (s, int(bool(spp[1])))
            assert rast_full.shape == (a.B, a.H, a.W, 4)
        assert pix.dtype == torch.int64 and inv.shape == (grid[0] * grid[1] * grid[2],) and inv.dtype == torch.int32
        first, t1 = _CaBuf.of(vals, null_vals, bg, keep, grid, P, spp, C=src.C, bg_grad=ask)
        second, t2 = (None, (None,) * 3) if vals2 is None else _CaBuf.of(vals2, null_vals2, bg2, keep2, grid, P, spp, bg_grad=ask2)
        sh, kept, outputs, src_saved = src.forward(ctx, (gb, w2c, view, light, all_tex), pix, grid, dev)
        cut = src.cut_in_tag and spp is None
        tag = ("" if spp is None else f"[spp{spp[0]}]") + "[" + (src.name or first.tag(cut)) + ("" if second is None else "+" + second.tag(cut)) + "]"
        ride = a.ride_args() if spp is None else None  # a deferred analysis runs inside the first launch of this call
        (sa, out), (sb, out2) = first.forward(t1, rast_full, dev), ((None, None) if second is None else second.forward(t2, rast_full, dev))
        call("a3d_composite_aa_fwd", ctypes.addressof(sa), None if sb is None else ctypes.addressof(sb), ptr(inv), ptr(a.work), ptr(a.count),
             a.capacity, a.B, a.H, a.W, None if ride is None else ctypes.addressof(ride), None if sh is None else ctypes.addressof(sh), stream(),
             tag=tag + src.suffix + ("[+analysis]" if ride is not None else ""))
        if ride is not None:
            a.pending = False  # (only now: the call above raises on a refused argument)
        # (the first buffer's rows in the backward: the caller's, or what the source kept of the ones the call computed -- or None)
        ctx.save_for_backward(pix, inv, rast_full, t1[0] if src.C is None else kept, t1[1], t1[2], *t2, *src_saved)
        ctx.analysis, ctx.tag, ctx.src, ctx.first, ctx.second = a, tag, src, first, second
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*outputs)
        return (out, out2) + outputs

    @staticmethod
    def backward(ctx, g_out, g_out2=None, *_):
        pix, inv, rast_full, *t = ctx.saved_tensors
        a, src, first, second, P, dev = ctx.analysis, ctx.src, ctx.first, ctx.second, pix.shape[0], pix.device
        sa, g_vals, g_null, g_out, g_bg = first.backward(t[0:3], g_out, rast_full, dev)
        sb, g_vals2, g_null2, g_out2, g_bg2 = (None,) * 5 if second is None else second.backward(t[3:6], g_out2, rast_full, dev)
        g_clip = torch.empty_like(a.clip)
        sh, state = src.backward(ctx, t[0], t[6:], pix, dev)
        call("a3d_composite_aa_bwd", ctypes.addressof(sa), None if sb is None else ctypes.addressof(sb), ptr(pix), P, ptr(inv), ptr(a.work),
             ptr(a.count), a.capacity, ptr(a.clip), a.clip.shape[0], ptr(a.topo.tri), a.B, a.clip.shape[1], a.topo.tri.shape[0], a.H, a.W, ptr(g_clip),
             None if sh is None else ctypes.addressof(sh), stream(), tag=ctx.tag)
        g_src = src.finish(ctx, state, g_vals, t[6:], pix, first.grid, dev)
        # (a background that came in another dtype went through f32c's cast: its gradient goes back in that dtype)
        g_bg, g_bg2 = (g if g is None or g.dtype == d else g.to(d) for g, d in zip((g_bg, g_bg2), ctx.bg_dtypes))
        return (None, None, None if src.C is not None else g_vals, g_null, g_vals2, g_null2, g_clip) + g_src + (None, g_bg, g_bg2)


def _shade_params(w2c, view, light):
    """a3d_shade_params over the tensors themselves: w2c [1|B,4,4] / [1|B,3,3], view [1|B,3], light [1|B,5] (contiguous float32)."""
    n = w2c.shape[1]
    return _lib.ShadeParams(size=ctypes.sizeof(_lib.ShadeParams), rot_row_stride=n, rot=ptr(w2c), view=ptr(view), light=ptr(light),
                            rot_image_stride=0 if w2c.shape[0] == 1 else n * n, view_image_stride=0 if view.shape[0] == 1 else 3,
                            light_image_stride=0 if light.shape[0] == 1 else 5)


def _depth_source(gb, w2c, pix, state, rows, g_gb, slots=None):
    """a3d_ca_shade carrying only the depth source: row 2 of w2c [1|B,4,4] read in place."""
    return _lib.CaShade(size=ctypes.sizeof(_lib.CaShade), depth_gb=ptr(gb), depth_w2c_row=w2c.data_ptr() + 8 * 4,
                        depth_w2c_stride=0 if w2c.shape[0] == 1 else 16, depth_pix=ptr(pix), depth_rows=pix.shape[0], depth_state=ptr(state),
                        depth_out=ptr(rows), g_depth_gb=ptr(g_gb), g_depth_slots=ptr(slots))


def _composite(src, pix, inv, clip, analysis, vals=None, vals2=None, background=None, background2=None, keep=None, keep2=None, null_vals=None,
               null_vals2=None, recipe=(None,) * 5, rast_full=None, msaa=None):
    """What the public functions below share: one clip batch, (image[, second image]) + further outputs; a background that requires grad
    goes to the node as a differentiable input (the others stay out of autograd's sight: nothing is allocated or launched for them) --
    at spp 1; in supersampled mode it is refused."""
    diff = [b if b is not None and b.requires_grad else None for b in (background, background2)]
    assert msaa is None or (diff[0] is None and diff[1] is None), ("msaa_composite_antialias: a background that requires grad gets no gradient in supersampled mode -- "
                                                            "composite with torch and call antialias (render_mesh sends such a call down its generic path)")
    if clip.dim() == 2:
        clip = clip[None]
    plain = [None if d is not None else b for b, d in zip((background, background2), diff)]
    o1, o2, *more = _Compositor.apply(src, (pix, inv, plain[0], plain[1], analysis, keep, keep2, msaa), vals, null_vals, vals2, null_vals2, clip, *recipe,
                                      rast_full, *diff)
    return (o1 if vals2 is None else (o1, o2)), more


def composite_antialias(vals, pix, inv, background, clip, analysis, vals2=None, background2=None, keep=None, keep2=None):
    """antialias(lerp(background, [vals, 1], coverage)) for a buffer given as rows ``vals`` [>= P,C] at the covered pixels ``pix`` (``inv`` =
    the pixel -> row map of covered_pixels(return_inverse=True)): [B,H,W,C+1].  ``background`` [1|B,H,W,<= C+1] (missing trailing channels
    = 0: the reference's 3-channel background as it is) or None (zeros).  A background that requires grad gets its gradient from the same
    backward call: the adjoint of the uncovered pixels -- the incoming gradient plus the blend adjoints of the crossing records -- summed
    over the images when it is shared; a covered pixel contributes exactly zero (a3d_ca_buffer.g_null at spp 1; one that does not require grad
    costs nothing).  With ``vals2`` (and ``background2``, differentiable alike) a second buffer over the same pixels is composited
    and antialiased by the same launches: returns the pair of images.  ``keep`` / ``keep2``: see _CaBuf."""
    return _composite(_ROWS, pix, inv, clip, analysis, vals, vals2, background, background2, keep, keep2)[0]


def shade_composite_antialias(recipe, pix, inv, background, clip, analysis, vals2=None, background2=None, keep2=None):
    """composite_antialias for the shaded colour of ``recipe`` (a ShadeRecipe) as first buffer: the colour is computed inside the launches,
    and one backward node runs compositor gather + shading adjoint (see _Shaded).  The backgrounds as in composite_antialias, their
    gradients included."""
    r = recipe
    if background is not None:
        background = f32c(background)
        if background.shape[3] == 4 and background.data_ptr() % 16:  # (an offset view: the compose kernel reads 4-channel texels as 16-byte loads)
            background = background.clone()  # (a differentiable copy: a background that requires grad keeps its graph)
    return _composite(_SHADED[bool(r.two_sided)], pix, inv, clip, analysis, None, vals2, background, background2, None, keep2,
                      recipe=(r.gb, r.w2c, r.view_pos, r.light, r.all_tex))[0]


def depth_composite_antialias(gb, w2c, pix, inv, clip, analysis, vals2=None, background2=None, keep2=None, return_rows=False):
    """The 'depth' render mode from the G-buffer rows ``gb`` [P,12] of the covered pixels ``pix`` / ``inv``: z = camera-space depth of the
    interpolated position (row 2 of ``w2c`` [1|B,4,4]), normalised per image with the extremes over ALL pixels of the frame (an uncovered
    pixel has z = w2c[b,2,3]), composited over zeros and antialiased: [B,H,W,1] (reference render.py:98-104, 311-315, 324-325).
    With ``vals2`` a second buffer rides in the same launches as in composite_antialias: returns the pair.  Differentiable in ``gb``
    (position columns) and ``clip`` (and ``vals2``); ``w2c`` gets no gradient.  ``return_rows``: also the [P] normalised depth rows."""
    assert not w2c.requires_grad, "depth_composite_antialias: w2c gets no gradient here (render_mesh takes the generic path for it)"
    res, (rows,) = _composite(_DEPTH, pix, inv, clip, analysis, None, vals2, None, background2, 1, keep2, recipe=(gb, w2c, None, None, None))
    return (res, rows) if return_rows else res


def msaa_composite_antialias(vals, null_vals, pix, inv, rast_full, background, clip, analysis, spp, antialias=True, vals2=None, null_vals2=None,
                             background2=None, keep=None, keep2=None):
    """render_mesh(spp = s > 1, msaa = True) of the reference behind the shading (render.py:217-219, 258-268, 318) for a buffer given as
    rows ``vals`` [>= P,C] at the covered texels ``pix`` of the shading-sample raster rast_full[:, ::s, ::s] (``inv`` [B*h*w] its pixel ->
    row map) and ``null_vals`` [B,C], the value of a shading sample that is NOT covered: avg_pool(antialias(lerp(background, up([v, 1]),
    coverage of ``rast_full``))) as [B,h,w,C+1].  ``analysis``: the AAAnalysis of (rast_full, clip), full resolution.  ``background``
    [1|B,h,w,<= C+1] on the shading grid (its nearest up-scale is what the reference composites over) or None; no gradient: one that
    requires grad is refused (the background's gradient exists at spp 1 only: composite_antialias).
    ``antialias`` False: composite and average only.  A second buffer and ``keep`` / ``keep2`` as in composite_antialias."""
    return _composite(_ROWS, pix, inv, clip, analysis, vals, vals2, background, background2, keep, keep2, null_vals,
                      null_vals2, rast_full=rast_full, msaa=(spp, antialias))[0]


def antialias(color, rast, clip, tri, analysis=None):
    """dr.antialias semantics; pass ``analysis`` (AAAnalysis) to share the geometry pass between buffers."""
    if clip.dim() == 2:
        clip = clip[None]
    if analysis is None:
        tri32 = tri_int32(tri)
        analysis = AAAnalysis(rast, clip, aa_topology(tri32, clip.shape[1]))
    return _Antialias.apply(color, clip, analysis)


# ---------------------------------------------------------------------------------------------- reconstruction losses
class _MaskAntialias(torch.autograd.Function):
    """lerp(bg, [1, .., 1], coverage) + antialias for a texture-less, light-less render (csrc/antialias.hip: a3d_mask_aa_*): the coverage
    comes from the raster texels, only the silhouette is differentiated (g_clip)."""

    @staticmethod
    def forward(ctx, rast, clip, bg, analysis, C):
        require_device(rast, clip, what="mask_antialias")
        a = analysis
        rast_c = f32c(rast.detach())
        if bg is not None:
            bg = f32c(bg)
            assert bg.shape[1:] == (a.H, a.W, C + 1) and bg.shape[0] in (1, a.B)
        out = torch.empty((a.B, a.H, a.W, C + 1), dtype=torch.float32, device=rast.device)
        ride = a.ride_args()
        call("a3d_mask_aa_fwd", ptr(rast_c), C, ptr(bg), 0 if bg is None else bg.shape[0], ptr(out), ptr(a.work), ptr(a.count), a.capacity, a.B, a.H,
             a.W, None if ride is None else ctypes.addressof(ride), stream(), tag=f"[C{C + 1}]" + ("[+analysis]" if ride is not None else ""))
        if ride is not None:
            a.pending = False
        ctx.save_for_backward(rast_c, bg)
        ctx.analysis, ctx.C = a, C
        return out

    @staticmethod
    def backward(ctx, g_out):
        rast_c, bg = ctx.saved_tensors
        a, C = ctx.analysis, ctx.C
        g_clip = torch.empty_like(a.clip)
        # the image usually went on as permute(0, 3, 1, 2) + a channel slice (Fauna.py:166-173): the engine then hands back a channels-FIRST
        # tensor seen through the inverse permute -- read where it is (its contiguous copy was 10 us of the Fauna step)
        first = g_out.dtype == torch.float32 and g_out.dim() == 4 and not g_out.is_contiguous() and g_out.permute(0, 3, 1, 2).is_contiguous()
        if not first:
            g_out = f32h(g_out)
        call("a3d_mask_aa_bwd", ptr(g_out), ptr(rast_c), C, ptr(bg), 0 if bg is None else bg.shape[0], ptr(a.work), ptr(a.count), a.capacity,
             ptr(a.clip), a.clip.shape[0], ptr(a.topo.tri), a.B, a.clip.shape[1], a.topo.tri.shape[0], a.H, a.W, ptr(g_clip), int(first), stream(),
             tag=f"[C{C + 1}]")
        return None, g_clip, None, None, None


def mask_antialias(rast, clip, background, analysis, channels=3):
    """[B,H,W,channels+1]: ones where ``rast`` is covered, ``background`` ([1|B,H,W,channels+1] or None = zeros) elsewhere, antialiased
    with ``analysis`` (an AAAnalysis of the same rast / clip; may still be pending: it then runs inside this op's first launch).  Only
    the silhouette is differentiated: a background that requires grad is refused."""
    assert background is None or not background.requires_grad, ("mask_antialias: the background gets no gradient here -- a call with a background that "
                                                                "requires grad goes through covered_pixels + composite_antialias (render_mesh: its covered-point path)")
    assert analysis.rast.data_ptr() == f32c(rast.detach()).data_ptr(), "the analysis must belong to this raster buffer"
    return _MaskAntialias.apply(rast.detach(), clip, background, analysis, int(channels))  # (coverage carries no gradient)


class _ReconLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, shaded, dino, image_gt, dino_gt, mask_gt, dt0, dt1, valid):
        require_device(shaded, image_gt, mask_gt, dt0, valid, what="reconstruction_losses")
        B, H, W = shaded.shape[:3]
        D = 0 if dino is None else dino.shape[3]
        assert shaded.shape == (B, H, W, 4) and shaded.is_contiguous() and image_gt.shape == (B, 3, H, W)
        ds = D if dino is None else dino.stride(2)  # floats between two pixels (D + 1: the renderer's 17-channel image read in place)
        assert dt0.shape == (B, H, W) and dt0.stride(2) == 1 and dt0.stride(1) == W
        assert dt1 is None or (dt1.shape == dt0.shape and dt1.stride() == dt0.stride())
        image_gt, mask_gt, valid = f32c(image_gt), f32c(mask_gt), f32c(valid)
        if D:
            assert dino.stride(3) == 1 and ds >= D and dino.stride(1) == W * ds and dino.stride(0) == H * W * ds and dino_gt.shape == (B, D, H, W)
            dino_gt = f32c(dino_gt)
        loss = torch.empty((B, _lib.lib().a3d_recon_losses_columns()), dtype=torch.float32, device=shaded.device)
        scratch = torch.empty(_lib.lib().a3d_recon_losses_scratch_bytes(B, H, W), dtype=torch.uint8, device=shaded.device)
        both = torch.empty(_lib.lib().a3d_recon_losses_mask_bytes(B, H, W), dtype=torch.uint8, device=shaded.device)
        call("a3d_recon_losses_fwd", ptr(shaded), ptr(dino), D, ds, ptr(image_gt), ptr(dino_gt), ptr(mask_gt), ptr(dt0), ptr(dt1), dt0.stride(0), ptr(valid),
             B, H, W, ptr(scratch), ptr(both), ptr(loss), stream())
        ctx.save_for_backward(shaded, dino, image_gt, dino_gt, mask_gt, dt0, dt1, valid, both)
        ctx.mark_non_differentiable(both)
        ctx.set_materialize_grads(False)  # (no zero tensor filled for the mask output's "gradient")
        return loss, both

    @staticmethod
    def backward(ctx, g_loss, _g_both=None):
        shaded, dino, image_gt, dino_gt, mask_gt, dt0, dt1, valid, both = ctx.saved_tensors
        B, H, W = shaded.shape[:3]
        D = 0 if dino is None else dino.shape[3]
        if g_loss is None:
            return (None,) * 8
        g_shaded = torch.empty_like(shaded)
        # the feature gradient in the layout of the image the features were sliced from (stride D + 1: the alpha slot stays unwritten, it
        # has no gradient): the compositor's backward reads it where it is, no zero-padded copy in between
        ds = dino.stride(2) if D else 0
        g_dino = torch.empty((B, H, W, ds), dtype=torch.float32, device=shaded.device)[..., :D] if D else None
        call("a3d_recon_losses_bwd", ptr(f32h(g_loss)), ptr(shaded), ptr(dino), D, ds, ds, ptr(image_gt), ptr(dino_gt), ptr(mask_gt), ptr(dt0), ptr(dt1),
             dt0.stride(0), ptr(valid), B, H, W, ptr(both), ptr(g_shaded), ptr(g_dino), stream())
        return g_shaded, g_dino, None, None, None, None, None, None


def reconstruction_losses(shaded_nchw, dino_nchw, image_gt, dino_gt, mask_gt, mask_dt, mask_valid, return_mask=False):
    """Per-frame [N,5] = (mask, mask_inv_dt, rgb, dino, mask_dt) losses of compute_reconstruction_losses (AnimalModel.py:260-307,
    background_mode 'none'; N = images x frames) from render_mesh's outputs: ``shaded_nchw`` [N,4,H,W] and ``dino_nchw`` [N,D,H,W] (or
    None) are the NCHW views render_mesh returns (NHWC in memory -- read in place, no copy); targets in the dataset's NCHW layout;
    mask_dt [N,2,H,W].  ``return_mask=True`` also returns the eroded common mask (uint8 [N*H*W]) that :func:`flow_loss` needs."""
    shaded = shaded_nchw.permute(0, 2, 3, 1)
    shaded = shaded if shaded.is_contiguous() else shaded.contiguous()
    dino = None
    if dino_nchw is not None:
        dino = dino_nchw.permute(0, 2, 3, 1)
        H, W, S = dino.shape[1], dino.shape[2], dino.stride(2)
        # (render_mesh's 'dino_pred' = the first 16 channels of its 17-channel image: evenly strided pixels are read in place)
        if not (dino.dtype == torch.float32 and dino.stride(3) == 1 and S >= dino.shape[3] and dino.stride(1) == W * S and dino.stride(0) == H * W * S):
            dino = dino.contiguous()
    loss, both = _ReconLosses.apply(shaded, dino, image_gt, dino_gt, mask_gt, mask_dt[:, 0], mask_dt[:, 1], mask_valid)
    return (loss, both) if return_mask else loss


class _FlowLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, flow_gt, both, B, F):
        require_device(flow, flow_gt, both, what="flow_loss")
        N, H, W = flow.shape[:3]
        assert N == B * F and F >= 2 and flow.shape[3] == 2 and flow.stride(3) == 1 and flow.stride(1) == W * flow.stride(2) \
            and flow.stride(0) == H * flow.stride(1), "flow must be the renderer's NHWC buffer (channel slice allowed)"
        flow_gt = f32c(flow_gt)
        assert flow_gt.shape == (B, F - 1, 2, H, W) and both.numel() == N * H * W
        loss = torch.empty((B, F - 1), dtype=torch.float32, device=flow.device)
        scale = torch.empty_like(loss)
        scratch = torch.empty(_lib.lib().a3d_flow_loss_scratch_bytes(B, F, H, W), dtype=torch.uint8, device=flow.device)
        call("a3d_flow_loss_fwd", ptr(flow), flow.stride(2), ptr(flow_gt), ptr(both), B, F, H, W, ptr(scratch), ptr(loss), ptr(scale), stream())
        ctx.save_for_backward(flow, flow_gt, both, scale)
        ctx.dims = (B, F, H, W)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        flow, flow_gt, both, scale = ctx.saved_tensors
        B, F, H, W = ctx.dims
        g_flow = torch.empty((B * F, H, W, 2), dtype=torch.float32, device=flow.device)
        call("a3d_flow_loss_bwd", ptr(f32h(g_loss)), ptr(scale), ptr(flow), flow.stride(2), ptr(flow_gt), ptr(both), B, F, H, W, ptr(g_flow), stream())
        return g_flow, None, None, None, None


def flow_loss(flow_nchw, flow_gt, both, batch, num_frames):
    """[B,F-1] flow loss between consecutive frames (AnimalModel.py:285-298) from render_mesh's 'flow' output [B*F,2,H,W] (the NCHW
    view of the renderer's NHWC buffer, read in place), flow_gt [B,F-1,2,H,W] and the eroded common mask of
    :func:`reconstruction_losses` (``return_mask=True``)."""
    return _FlowLoss.apply(flow_nchw.permute(0, 2, 3, 1), flow_gt, both, int(batch), int(num_frames))


# ---------------------------------------------------------------------------------------------- harmonic embedding
class _HarmonicEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, freq, symmetrize, ones):
        require_device(x, freq, what="harmonic_embed")
        x, freq = f32c(x), f32c(freq)
        P, n = x.shape[0], freq.shape[0]
        assert x.shape == (P, 3)
        out = torch.empty((P, 3 + 6 * n + int(ones)), dtype=torch.float32, device=x.device)
        call("a3d_harmonic_embed_fwd", ptr(x), ptr(freq), n, int(symmetrize), int(ones), P, ptr(out), stream())
        ctx.save_for_backward(x, freq)
        ctx.cfg = (int(symmetrize), int(ones))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, freq = ctx.saved_tensors
        g_x = torch.empty_like(x)
        call("a3d_harmonic_embed_bwd", ptr(f32h(g)), ptr(x), ptr(freq), freq.shape[0], ctx.cfg[0], ctx.cfg[1], x.shape[0], ptr(g_x), stream())
        return g_x, None, None, None


def harmonic_embed_raw(x, freq, symmetrize, ones):
    """harmonic_embed without an autograd node (inside hostnets' Functions)."""
    return _HarmonicEmbed.forward(_NoCtx(), x, freq, symmetrize, ones)


def harmonic_embed_bwd_raw(g, x, freq, symmetrize, ones):
    """g [P, 3 + 6n (+1)] -> J_e(x)^T g [P,3]: harmonic_embed's adjoint as a plain call (inside hostnets' Functions)."""
    require_device(g, x, freq, what="harmonic_embed_bwd")
    x, freq = f32c(x), f32c(freq)
    if tuple(g.shape) != (x.shape[0], 3 + 6 * freq.shape[0] + int(ones)):
        raise ValueError(f"harmonic_embed_bwd: g must be [{x.shape[0]},{3 + 6 * freq.shape[0] + int(ones)}], got {list(g.shape)}")
    g_x = torch.empty_like(x)
    call("a3d_harmonic_embed_bwd", ptr(f32h(g)), ptr(x), ptr(freq), freq.shape[0], int(symmetrize), int(ones), x.shape[0], ptr(g_x), stream())
    return g_x


class _NoCtx:
    """Stands in for the autograd context where a Function's forward is called as a plain function."""

    def save_for_backward(self, *tensors):
        pass


def harmonic_embed(x, freq, symmetrize=False, ones=False):
    """[P,3] -> [P, 3 + 6n (+1)] = [x (|x_0| if symmetrize), sin(x_c f_k), cos(x_c f_k), (1)] (csrc/embed.hip).  First-order
    differentiable only (double backward raises): the SDF regulariser, which differentiates the field twice, calls the kernels as plain
    functions (harmonic_embed_raw, harmonic_embed_bwd_raw, harmonic_embed_jvp) from hostnets' own Functions, or takes the torch path."""
    if x.dim() != 2 or x.shape[1] != 3 or freq.dim() != 1 or freq.shape[0] < 1:
        raise ValueError(f"harmonic_embed: expected x [P,3] and n >= 1 frequencies [n], got {list(x.shape)} and {list(freq.shape)}")
    if not (x.is_floating_point() and freq.is_floating_point()):
        raise ValueError(f"harmonic_embed: x and freq must be floating point, got {x.dtype} and {freq.dtype}")
    return _HarmonicEmbed.apply(x, freq, bool(symmetrize), bool(ones))


# ---------------------------------------------------------------------------------------------- fp32 MFMA GEMM + ReLU adjoint
def _rows256_out(what, out, m, device):
    """The [M,256] float32 result buffer: a fresh one, or the caller's ``out`` (a layer's slice of a stacked buffer)."""
    if out is None:
        return torch.empty((m, 256), dtype=torch.float32, device=device)
    if tuple(out.shape) != (m, 256) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{what}: out must be float32, contiguous and [{m},256] on {device}, got {out.dtype} {list(out.shape)} on {out.device}")
    return out


def gemm_nn_relumask(a, b, x=None, out=None):
    """(a [M,K] @ b [K,256]) * (x [M,256] > 0)  (x None: plain product) -- csrc/gemm.hip, fp32 MFMA.  No autograd: it is the
    input-gradient GEMM inside hostnets' stack backward.  The mask is read in place: float32, contiguous, and only for K >= 256."""
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] < 32 or a.shape[1] % 32 or tuple(b.shape) != (a.shape[1], 256):
        raise ValueError(f"gemm_nn_relumask: expected a [M,K] and b [K,256] with K a positive multiple of 32, got {list(a.shape)} and {list(b.shape)}")
    if x is not None and (tuple(x.shape) != (a.shape[0], 256) or x.dtype != torch.float32 or not x.is_contiguous() or a.shape[1] < 256):
        raise ValueError(f"gemm_nn_relumask: the mask must be float32, contiguous and [M,256] = [{a.shape[0]},256], with K >= 256; got {x.dtype} "
                         f"{list(x.shape)} with strides {list(x.stride())} and K = {a.shape[1]}")
    require_device(a, b, x, what="gemm_nn_relumask")
    a, b = f32c(a), f32c(b)
    M, K = a.shape
    c = _rows256_out("gemm_nn_relumask", out, M, a.device)
    call("a3d_gemm_nn_relumask", ptr(a), ptr(b), ptr(x), M, 256, K, ptr(c), stream())
    return c


def gemm_nt_relumask(a, w, x=None, out=None):
    """(a [M,K] @ w [256,K]^T) * (x [M,256] > 0)  (x None: plain product) -- csrc/gemm.hip, fp32 MFMA on 64 x 128 tiles, made for short
    point lists.  ``w`` is a Linear's [out,in] weight as stored; K a multiple of 4.  No autograd: it is the forward product with a foreign
    (frozen) ReLU mask inside hostnets' field-gradient adjoint."""
    if a.dim() != 2 or w.dim() != 2 or a.shape[1] < 4 or a.shape[1] % 4 or tuple(w.shape) != (256, a.shape[1]):
        raise ValueError(f"gemm_nt_relumask: expected a [M,K] and w [256,K] with K a positive multiple of 4, got {list(a.shape)} and {list(w.shape)}")
    if x is not None and (tuple(x.shape) != (a.shape[0], 256) or x.dtype != torch.float32 or not x.is_contiguous()):
        raise ValueError(f"gemm_nt_relumask: the mask must be float32, contiguous and [M,256] = [{a.shape[0]},256]; got {x.dtype} {list(x.shape)} "
                         f"with strides {list(x.stride())}")
    require_device(a, w, x, what="gemm_nt_relumask")
    a, w = f32c(a), f32c(w)
    M, K = a.shape
    c = _rows256_out("gemm_nt_relumask", out, M, a.device)
    call("a3d_gemm_nt_relumask", ptr(a), ptr(w), ptr(x), M, 256, K, ptr(c), stream(), tag=f"[K{K}]")
    return c


def gemm_tn_splitk(p, q):
    """[p_b^T @ q_b] [B,256,C] for p [B,M,256] and q [B,M,C] (C a multiple of 4, at most 256): the weight gradients of a short point list,
    all layers in one call -- csrc/gemm.hip, fp32 MFMA, split-K over the rows with the partial products added in a fixed order.  No autograd."""
    if p.dim() != 3 or q.dim() != 3 or p.shape[2] != 256 or tuple(q.shape[:2]) != tuple(p.shape[:2]) or not 4 <= q.shape[2] <= 256 or q.shape[2] % 4 \
            or not 1 <= p.shape[0] <= 64 or p.shape[1] < 1:
        raise ValueError(f"gemm_tn_splitk: expected p [B,M,256] and q [B,M,C] with 1 <= B <= 64, M >= 1 and C a multiple of 4 up to 256, got "
                         f"{list(p.shape)} and {list(q.shape)}")
    require_device(p, q, what="gemm_tn_splitk")
    p, q = f32c(p), f32c(q)
    B, M, C = q.shape
    scratch = torch.empty(_lib.lib().a3d_gemm_tn_splitk_scratch_bytes(M, C, B), dtype=torch.uint8, device=p.device)
    out = torch.empty((B, 256, C), dtype=torch.float32, device=p.device)
    call("a3d_gemm_tn_splitk", ptr(p), ptr(q), M, C, B, ptr(scratch), ptr(out), stream(), tag=f"[n{B}x{C}]")
    return out


def harmonic_embed_jvp(x, lam, freq, symmetrize=False, ones=False):
    """J_e(x) lam [P, 3 + 6n (+1)]: the tangent of :func:`harmonic_embed` along ``lam`` [P,3] (csrc/embed.hip).  No autograd."""
    if x.dim() != 2 or x.shape[1] != 3 or tuple(lam.shape) != tuple(x.shape) or freq.dim() != 1 or freq.shape[0] < 1:
        raise ValueError(f"harmonic_embed_jvp: expected x and lam [P,3] and n >= 1 frequencies [n], got {list(x.shape)}, {list(lam.shape)} and "
                         f"{list(freq.shape)}")
    require_device(x, lam, freq, what="harmonic_embed_jvp")
    x, lam, freq = f32c(x), f32c(lam), f32c(freq)
    P, n = x.shape[0], freq.shape[0]
    out = torch.empty((P, 3 + 6 * n + int(ones)), dtype=torch.float32, device=x.device)
    call("a3d_harmonic_embed_jvp", ptr(x), ptr(lam), ptr(freq), n, int(symmetrize), int(ones), P, ptr(out), stream())
    return out


def _field_grad_head_args(what, s, w, y):
    if y.dim() != 2 or y.shape[1] != _lib.FIELD_HEAD_WIDTH or y.shape[0] < 1 or s.numel() != y.shape[0] or w.numel() != _lib.FIELD_HEAD_WIDTH:
        raise ValueError(f"{what}: expected s [M] or [M,1], w [256] or [1,256] and [M,256] hidden vectors with M >= 1, got {list(s.shape)}, "
                         f"{list(w.shape)} and {list(y.shape)}")
    return int(y.shape[0])


def field_grad_head_fwd(s, w, y, out=None):
    """b [M,256] = (s[m] w[k]) * (y[m,k] > 0): the start of a scalar field's input-gradient chain (csrc/fieldhead.hip).  No autograd."""
    M = _field_grad_head_args("field_grad_head_fwd", s, w, y)
    require_device(s, w, y, what="field_grad_head_fwd")
    s, w, y = f32c(s), f32c(w), f32c(y)
    b = _rows256_out("field_grad_head_fwd", out, M, y.device)
    call("a3d_field_grad_head_fwd", ptr(s), ptr(w), ptr(y), M, ptr(b), stream())
    return b


def field_grad_head_bwd(s, t, w, need_s=False):
    """(g_w [1,256] = sum_m s[m] t[m,:], g_s [M,1] = t @ w^T or None) -- the adjoint of :func:`field_grad_head_fwd` behind the frozen mask;
    per-work-group partial sums added in a fixed order (no atomics, the same bits on every run).  No autograd."""
    M = _field_grad_head_args("field_grad_head_bwd", s, w, t)
    require_device(s, t, w, what="field_grad_head_bwd")
    s, t, w = f32c(s), f32c(t), f32c(w)
    scratch = torch.empty(_lib.lib().a3d_field_grad_head_scratch_bytes(M), dtype=torch.uint8, device=t.device)
    g_w = torch.empty((1, _lib.FIELD_HEAD_WIDTH), dtype=torch.float32, device=t.device)
    g_s = torch.empty((M, 1), dtype=torch.float32, device=t.device) if need_s else None
    call("a3d_field_grad_head_bwd", ptr(s), ptr(t), ptr(w), M, ptr(scratch), ptr(g_w), ptr(g_s), stream())
    return g_w, g_s


def _field_head_args(what, h, weight, scale, act):
    if h.dim() != 2 or weight.dim() != 2 or h.shape[1] != _lib.FIELD_HEAD_WIDTH or weight.shape[1] != _lib.FIELD_HEAD_WIDTH \
            or not 1 <= weight.shape[0] <= _lib.FIELD_HEAD_MAX_C or not 1 <= h.shape[0] < 1 << 31:
        raise ValueError(f"{what}: expected h [M,{_lib.FIELD_HEAD_WIDTH}] with M >= 1 and weight [C <= {_lib.FIELD_HEAD_MAX_C},{_lib.FIELD_HEAD_WIDTH}], "
                         f"got {list(h.shape)} and {list(weight.shape)}")
    if act not in (_lib.FIELD_HEAD_ACT_NONE, _lib.FIELD_HEAD_ACT_SIGMOID):
        raise ValueError(f"{what}: act is 0 (none) or 1 (sigmoid), got {act!r}")
    if scale is not None and tuple(scale.shape) != (weight.shape[0],):
        raise ValueError(f"{what}: scale / lo must be [C] = [{weight.shape[0]}], got {list(scale.shape)}")
    return int(h.shape[0]), int(weight.shape[0])


def field_head_fwd(h, weight, lo=None, scale=None, act=0):
    """s = act(h [M,256] @ weight [C,256]^T), out = s * scale + lo  (csrc/fieldhead.hip, fp32 MFMA, one pass over h).  ``act`` 0: none,
    1: sigmoid; ``lo`` / ``scale`` [C] or both None.  -> (s, out), s None when there is neither an activation nor the map.
    No autograd: it is the output stage inside hostnets' stack Function."""
    require_device(h, weight, lo, scale, what="field_head_fwd")
    if (lo is None) != (scale is None):
        raise ValueError("field_head_fwd: lo and scale come together")
    M, C = _field_head_args("field_head_fwd", h, weight, scale, act)
    if lo is not None and tuple(lo.shape) != (C,):
        raise ValueError(f"field_head_fwd: scale / lo must be [C] = [{C}], got {list(lo.shape)}")
    h, weight = f32c(h), f32c(weight)
    out = torch.empty((M, C), dtype=torch.float32, device=h.device)
    s = torch.empty((M, C), dtype=torch.float32, device=h.device) if (act or scale is not None) else None
    call("a3d_field_head_fwd", ptr(h), ptr(weight), None if lo is None else ptr(f32h(lo)), None if scale is None else ptr(f32h(scale)), int(act), M, C,
         ptr(s), ptr(out), stream(), tag=f"[C{C}]")
    return s, out


def field_head_bwd(g_out, s, h, weight, scale=None, act=0):
    """The adjoint of field_head_fwd and of the ReLU that produced h, one pass over h: with ga = g_out * scale * act'(s),
    g_h = (ga @ weight) * (h > 0) [M,256] and g_w = ga^T @ h [C,256] (per-work-group partial sums added in a fixed order by a second
    launch: no atomics, the same bits on every run).  ``s`` is what the forward returned (None without the sigmoid).  No autograd."""
    require_device(g_out, s, h, weight, scale, what="field_head_bwd")
    M, C = _field_head_args("field_head_bwd", h, weight, scale, act)
    if tuple(g_out.shape) != (M, C) or (act and (s is None or tuple(s.shape) != (M, C))):
        raise ValueError(f"field_head_bwd: g_out and s must be [M,C] = [{M},{C}], got {list(g_out.shape)} and {None if s is None else list(s.shape)}")
    g_out, h, weight = f32c(g_out), f32c(h), f32c(weight)
    scratch = torch.empty(_lib.lib().a3d_field_head_scratch_bytes(M, C), dtype=torch.uint8, device=h.device)
    g_h = torch.empty((M, _lib.FIELD_HEAD_WIDTH), dtype=torch.float32, device=h.device)
    g_w = torch.empty((C, _lib.FIELD_HEAD_WIDTH), dtype=torch.float32, device=h.device)
    call("a3d_field_head_bwd", ptr(g_out), None if not act else ptr(f32h(s)), ptr(h), ptr(weight), None if scale is None else ptr(f32h(scale)), int(act),
         M, C, ptr(scratch), ptr(g_h), ptr(g_w), stream(), tag=f"[C{C}]")
    return g_h, g_w


# ---------------------------------------------------------------------------------------------- texture sampling
_TEX_FILTERS = {"nearest": 0, "linear": 1, "linear-mipmap-nearest": 2, "linear-mipmap-linear": 3}
_TEX_BOUNDARIES = {"wrap": 0, "clamp": 1, "zero": 2, "cube": 3}
TEX_MAX_LEVELS = _lib.TEX_MAX_LEVELS


def texture_filter_mode(filter_mode, uv_da=None, mip_level_bias=None):
    """'auto' -> 'linear-mipmap-linear' when uv_da or mip_level_bias is given, 'linear' otherwise."""
    if filter_mode == "auto":
        return "linear-mipmap-linear" if (uv_da is not None or mip_level_bias is not None) else "linear"
    if filter_mode not in _TEX_FILTERS:
        raise ValueError(f"texture: unknown filter_mode {filter_mode!r}")
    return filter_mode


def texture_mip_sizes(height, width, max_mip_level=None):
    """[(h, w)] of the mip chain from level 0: every dimension > 1 halves; the chain stops at 1 x 1, at level ``max_mip_level``, at the
    first level with an odd dimension > 1, or at 16 levels (A3D_TEX_MAX_LEVELS)."""
    sizes = [(int(height), int(width))]
    top = TEX_MAX_LEVELS - 1 if max_mip_level is None else min(int(max_mip_level), TEX_MAX_LEVELS - 1)
    while len(sizes) - 1 < top:
        h, w = sizes[-1]
        if (h == 1 and w == 1) or (h > 1 and h % 2) or (w > 1 and w % 2):
            break
        sizes.append((max(h // 2, 1), max(w // 2, 1)))
    return sizes


def _tex_hw(t, cube):
    """(tex_batch, height, width, C) of a level [Bt,H,W,C] / cube [Bt,6,S,S,C]."""
    if cube:
        if t.dim() != 5 or t.shape[1] != 6 or t.shape[2] != t.shape[3]:
            raise ValueError(f"texture: a cube level must have shape [Bt, 6, S, S, C], got {list(t.shape)}")
        return t.shape[0], t.shape[2], t.shape[3], t.shape[4]
    if t.dim() != 4:
        raise ValueError(f"texture: a 2-D level must have shape [Bt, H, W, C], got {list(t.shape)}")
    return t.shape[0], t.shape[1], t.shape[2], t.shape[3]


def _tex_desc(levels, C, tex_batch, filt, boundary, grads=None):
    d = _lib.TexDesc(size=ctypes.sizeof(_lib.TexDesc), C=C, tex_batch=tex_batch, filter=filt, boundary=boundary, levels=len(levels))
    cube = boundary == _TEX_BOUNDARIES["cube"]
    for l, t in enumerate(levels):
        d.height[l], d.width[l] = (t.shape[2], t.shape[3]) if cube else (t.shape[1], t.shape[2])
        d.level[l] = t.data_ptr()
        if grads is not None and grads[l] is not None:
            d.grad[l] = grads[l].data_ptr()
    return d


class _TextureMip(torch.autograd.Function):
    """levels 1.. of the box-filter chain of ``tex`` (a3d_texture_mip_fwd); the backward pushes their gradients down to ``tex``."""

    @staticmethod
    def forward(ctx, tex, sizes, cube):
        require_device(tex, what="texture_construct_mip")
        tex = f32c(tex)
        Bt, _, _, C = _tex_hw(tex, cube)
        lead = (Bt, 6) if cube else (Bt,)
        levels = [tex] + [torch.empty(lead + (h, w, C), dtype=torch.float32, device=tex.device) for h, w in sizes[1:]]
        call("a3d_texture_mip_fwd", ctypes.byref(_tex_desc(levels, C, Bt, 1, 3 if cube else 1)), stream())
        ctx.shapes, ctx.cube = [tuple(t.shape) for t in levels], cube
        return tuple(levels[1:])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g_levels):
        dev = g_levels[0].device if g_levels[0] is not None else torch.device("cuda", torch.cuda.current_device())
        grads = [torch.zeros(ctx.shapes[0], dtype=torch.float32, device=dev)]
        for shape, g in zip(ctx.shapes[1:], g_levels):  # (mip_bwd adds into every level below the coarsest: own copies)
            grads.append(torch.zeros(shape, dtype=torch.float32, device=dev) if g is None else f32c(g).clone())
        C, Bt = ctx.shapes[0][-1], ctx.shapes[0][0]
        call("a3d_texture_mip_bwd", ctypes.byref(_tex_desc(grads, C, Bt, 1, 3 if ctx.cube else 1, grads)), stream())
        return grads[0], None, None


class TextureMip:
    """A mip stack built by texture_construct_mip (dr.texture_construct_mip): pass it as ``mip=``.  Its levels are constants."""

    def __init__(self, levels, cube):
        self.levels, self.cube = list(levels), cube


def texture_construct_mip(tex, max_mip_level=None, cube_mode=False):
    """The box-filter mip chain of ``tex`` (levels 1..; see texture_mip_sizes), on the GPU, without gradients."""
    Bt, H, W, C = _tex_hw(tex, cube_mode)
    with torch.no_grad():
        levels = _TextureMip.apply(tex.detach(), texture_mip_sizes(H, W, max_mip_level), bool(cube_mode)) if (H, W) != (1, 1) else ()
    return TextureMip(levels if isinstance(levels, tuple) else (levels,), bool(cube_mode))


class _Texture(torch.autograd.Function):
    @staticmethod
    def forward(ctx, filt, boundary, uv, uv_da, bias, *levels):
        require_device(uv, uv_da, bias, *levels, what="texture")
        cube = boundary == _TEX_BOUNDARIES["cube"]
        uv, uv_da, bias = f32c(uv), None if uv_da is None else f32c(uv_da), None if bias is None else f32c(bias)
        if uv_da is not None and not cube and uv_da.data_ptr() % 16:  # (the kernels read a 2-D uv_da row as one float4)
            uv_da = uv_da.clone()
        levels = [f32c(t) for t in levels]
        Bt, _, _, C = _tex_hw(levels[0], cube)
        B = uv.shape[0]
        H = uv.shape[1] if uv.dim() == 4 else int(math.prod(uv.shape[1:-1]))
        W = uv.shape[2] if uv.dim() == 4 else 1
        out = torch.empty(tuple(uv.shape[:-1]) + (C,), dtype=torch.float32, device=uv.device)
        if out.numel():
            call("a3d_texture_fwd", ctypes.byref(_tex_desc(levels, C, Bt, filt, boundary)), ptr(uv), ptr(uv_da), ptr(bias), B, H, W, ptr(out),
                 stream(), tag=f"[C{C}]")
        ctx.save_for_backward(uv, uv_da, bias, *levels)
        ctx.cfg = (filt, boundary, C, Bt, B, H, W)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        uv, uv_da, bias, *levels = ctx.saved_tensors
        filt, boundary, C, Bt, B, H, W = ctx.cfg
        mipmap_linear = filt == _TEX_FILTERS["linear-mipmap-linear"]
        g_uv = torch.empty_like(uv)
        g_da = torch.empty_like(uv_da) if uv_da is not None and mipmap_linear else None
        g_bias = torch.empty_like(bias) if bias is not None and mipmap_linear else None
        grads = [torch.zeros_like(t) for t in levels]
        if g_out.numel():
            call("a3d_texture_bwd", ctypes.byref(_tex_desc(levels, C, Bt, filt, boundary, grads)), ptr(f32h(g_out)), ptr(uv), ptr(uv_da), ptr(bias),
                 B, H, W, ptr(g_uv), ptr(g_da), ptr(g_bias), stream(), tag=f"[C{C}]")
        else:
            g_uv.zero_()
        if uv_da is not None and g_da is None:
            g_da = torch.zeros_like(uv_da)
        if bias is not None and g_bias is None:
            g_bias = torch.zeros_like(bias)
        return (None, None, g_uv, g_da, g_bias, *grads)


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode="auto", boundary_mode="wrap", max_mip_level=None):
    """dr.texture on the GPU (csrc/texture.hip): [B,H,W,C] samples of ``tex`` at ``uv``.

    This is the project's specification of nvdiffrast's operator, written from its published interface and UNPINNED against upstream
    (no nvdiffrast build to compare with).

    Shapes.  2-D: tex [Bt,Th,Tw,C] (Bt = 1 or B), uv [B,H,W,2], uv_da [B,H,W,4] = (du/dX, du/dY, dv/dX, dv/dY), mip_level_bias [B,H,W].
    Cube (boundary_mode='cube'): tex [Bt,6,S,S,C], uv [B,H,W,3] (a direction, any length), uv_da [B,H,W,6] = (dx/dX, dx/dY, dy/dX, dy/dY,
    dz/dX, dz/dY).  Any C.  Texel centres at (i + 0.5) / size.

    filter_mode: 'nearest' | 'linear' | 'linear-mipmap-nearest' | 'linear-mipmap-linear'; 'auto' = 'linear-mipmap-linear' when uv_da or
    mip_level_bias is given, else 'linear'.  boundary_mode: 'wrap' | 'clamp' | 'zero' (per mip level) or 'cube', seamless:
      - face = the largest |component| of uv (ties x before y before z), faces +x, -x, +y, -y, +z, -z; face coordinates
        +x (-z,-y), -x (z,-y), +y (x,z), -y (x,-z), +z (x,-y), -z (-x,-y), over |major| -- the inverse of the reference's cube_to_dir
        (model/render/util.py:96-103); -1..1 maps to column / row 0..S (texel i centred at -1 + (2i+1)/S).
      - a bilinear tap outside the face in one coordinate: the direction of that virtual texel centre on the extended face plane picks
        the face it is fetched from (clamped into range); a tap outside in both (a cube corner) is the mean of the quad's other three.
    Level of detail: 2-D, J = rows (du/dX, du/dY) * Tw and (dv/dX, dv/dY) * Th; cube, the face-coordinate derivatives of uv_da by the
    quotient rule at S/2 texels per unit.  level = 0.5 log2(lambda_max(J J^T)) + bias (without uv_da: level = bias), clamped to
    [0, L-1]; a zero J gives level 0.  The level follows this for every finite uv_da, also where J J^T lies beyond the fp32 range
    (|J| above ~6e9 or below ~1e-19 texels per pixel).  'linear-mipmap-nearest' takes level floor(level + 0.5), 'linear-mipmap-linear' blends the two
    neighbouring levels by the fraction.
    Mip stack: mip=None (mipmap modes) builds it on the device (texture_mip_sizes: halve every dimension > 1 with a box mean, stop at
    1 x 1, at max_mip_level or at an odd dimension > 1), differentiably back to ``tex``; mip=[tensors] is a custom stack whose level i
    must have the size the halving rule gives (ValueError otherwise) and each of which receives its own gradient; mip=TextureMip
    (texture_construct_mip) holds constants.
    Gradients: tex and every mip tensor always; uv except under 'nearest' (zeros there), with the level treated as a constant (so in
    cube mode g_uv is orthogonal to uv); uv_da and mip_level_bias only under 'linear-mipmap-linear' and where the level is not clamped.
    A zero cube direction samples 0.  A 2-D uv of any finite size samples as specified: under wrap it is taken modulo 1, and under
    clamp / zero a uv far outside the texture reads the edge texels, or nothing.  Non-finite uv or uv_da values are outside this
    specification: they give NaN or level-0 results, never an access outside the texture."""
    filter_mode = texture_filter_mode(filter_mode, uv_da, mip_level_bias)
    if boundary_mode not in _TEX_BOUNDARIES:
        raise ValueError(f"texture: unknown boundary_mode {boundary_mode!r}")
    cube = boundary_mode == "cube"
    Bt, H, W, C = _tex_hw(tex, cube)
    if uv.shape[-1] != (3 if cube else 2) or uv.dim() < 2:
        raise ValueError(f"texture: uv must have shape [B, ..., {3 if cube else 2}], got {list(uv.shape)}")
    if Bt not in (1, uv.shape[0]):
        raise ValueError(f"texture: texture batch {Bt} must be 1 or the uv batch {uv.shape[0]}")
    if uv_da is not None and tuple(uv_da.shape) != tuple(uv.shape[:-1]) + (6 if cube else 4,):
        raise ValueError(f"texture: uv_da must have shape {list(uv.shape[:-1]) + [6 if cube else 4]}, got {list(uv_da.shape)}")
    if mip_level_bias is not None and tuple(mip_level_bias.shape) != tuple(uv.shape[:-1]):
        raise ValueError(f"texture: mip_level_bias must have shape {list(uv.shape[:-1])}, got {list(mip_level_bias.shape)}")
    levels = [tex]
    if filter_mode in ("linear-mipmap-nearest", "linear-mipmap-linear"):
        sizes = texture_mip_sizes(H, W, max_mip_level)
        if mip is None:
            if len(sizes) > 1:
                levels += list(_TextureMip.apply(tex, sizes, cube))
        else:
            stack = list(mip.levels) if isinstance(mip, TextureMip) else list(mip)
            if isinstance(mip, TextureMip) and mip.cube != cube:
                raise ValueError("texture: the mip stack was built for the other boundary mode (cube_mode)")
            if max_mip_level is not None:
                stack = stack[:max(int(max_mip_level), 0)]
            if len(stack) > len(sizes) - 1:
                raise ValueError(f"texture: a custom mip stack of {len(stack)} levels; the halving rule from {H} x {W} gives {len(sizes) - 1}")
            for i, t in enumerate(stack):
                bt, h, w, c = _tex_hw(t, cube)
                if (h, w) != sizes[i + 1] or c != C or bt != Bt:
                    raise ValueError(f"texture: mip level {i + 1} has shape {list(t.shape)}; the halving rule gives {sizes[i + 1]} "
                                     f"(batch {Bt}, {C} channels)")
            levels += stack
    return _Texture.apply(_TEX_FILTERS[filter_mode], _TEX_BOUNDARIES[boundary_mode], uv, uv_da, mip_level_bias, *levels)


def cube_box_down(cubemap):
    """[6,S,S,C] -> [6,S/2,S/2,C]: the 2 x 2 box mean of every face (a3d_texture_mip_fwd on a one-step cube stack); no autograd."""
    require_device(cubemap, what="cube_box_down")
    if cubemap.dim() != 4 or cubemap.shape[0] != 6 or cubemap.shape[1] != cubemap.shape[2] or cubemap.shape[1] % 2:
        raise ValueError(f"cube_box_down: the map must have shape [6, S, S, C] with S even, got {list(cubemap.shape)}")
    fine = f32c(cubemap.detach())[None]
    S, C = fine.shape[2], fine.shape[4]
    coarse = torch.empty((1, 6, S // 2, S // 2, C), dtype=torch.float32, device=fine.device)
    call("a3d_texture_mip_fwd", ctypes.byref(_tex_desc([fine, coarse], C, 1, 1, 3)), stream())
    return coarse[0]


def cube_box_down_adjoint(g_coarse):
    """The adjoint of cube_box_down: [6,S,S,C] -> [6,2S,2S,C], every fine texel gets a quarter of its parent (a3d_texture_mip_bwd)."""
    require_device(g_coarse, what="cube_box_down_adjoint")
    coarse = f32c(g_coarse.detach())[None].clone()
    S, C = coarse.shape[2], coarse.shape[4]
    fine = torch.zeros((1, 6, 2 * S, 2 * S, C), dtype=torch.float32, device=coarse.device)
    call("a3d_texture_mip_bwd", ctypes.byref(_tex_desc([fine, coarse], C, 1, 1, 3, [fine, coarse])), stream())
    return fine[0]


# ---------------------------------------------------------------------------------------------- environment probes
def envmap_device_ok(t):
    """True when ``t`` can take the generated-coordinate resamplers below: a CUDA float32 tensor."""
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32


def _envmap_res(res, what):
    if len(res) != 2 or int(res[0]) < 1 or int(res[1]) < 1:
        raise ValueError(f"{what}: res must be [height, width] with both >= 1, got {res!r}")
    return int(res[0]), int(res[1])


class _EnvResample(torch.autograd.Function):
    """a3d_texture_fwd / a3d_texture_bwd with uv == NULL (include/a3d.h, generated coordinates): ``tex`` is [1,H,W,C] with boundary
    wrap (-> the cube [6,h,w,C]) or [1,6,S,S,C] with boundary cube (-> the lat-long map [1,h,w,C]).  One launch each way; the
    gradient goes to the map only (float atomics after the in-wave merge: its last bits depend on the order)."""

    @staticmethod
    def forward(ctx, tex, boundary, B, h, w):
        require_device(tex, what="envmap resample")
        tex = f32c(tex)
        C = tex.shape[-1]
        out = torch.empty((B, h, w, C), dtype=torch.float32, device=tex.device)
        call("a3d_texture_fwd", ctypes.byref(_tex_desc([tex], C, 1, _TEX_FILTERS["linear"], boundary)), None, None, None, B, h, w, ptr(out), stream(),
             tag=f"[gen C{C}]")
        ctx.cfg = (boundary, tuple(tex.shape), B, h, w)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        boundary, shape, B, h, w = ctx.cfg
        g_out = f32c(g_out)
        g_tex = torch.zeros(shape, dtype=torch.float32, device=g_out.device)
        call("a3d_texture_bwd", ctypes.byref(_tex_desc([g_tex], shape[-1], 1, _TEX_FILTERS["linear"], boundary, [g_tex])), ptr(g_out), None, None,
             None, B, h, w, None, None, None, stream(), tag=f"[gen C{shape[-1]}]")
        return g_tex, None, None, None, None


def latlong_to_cubemap(latlong, res):
    """[H,W,C] lat-long map -> [6,res[0],res[1],C] cube, the reference's util.latlong_to_cubemap (model/render/util.py:105-118) in one
    launch (csrc/texture.hip with generated coordinates; the arithmetic is spelled out in include/a3d.h).  CUDA float32; differentiable
    in the map."""
    if not envmap_device_ok(latlong) or latlong.dim() != 3:
        raise ValueError("latlong_to_cubemap: the map must be a CUDA float32 tensor of shape [H, W, C]")
    h, w = _envmap_res(res, "latlong_to_cubemap")
    return _EnvResample.apply(latlong[None], _TEX_BOUNDARIES["wrap"], 6, h, w)


def cubemap_to_latlong(cubemap, res):
    """[6,S,S,C] cube -> [res[0],res[1],C] lat-long map, the reference's util.cubemap_to_latlong (model/render/util.py:120-133) in one
    launch.  CUDA float32; differentiable in the cube."""
    if not envmap_device_ok(cubemap) or cubemap.dim() != 4 or cubemap.shape[0] != 6 or cubemap.shape[1] != cubemap.shape[2]:
        raise ValueError("cubemap_to_latlong: the map must be a CUDA float32 tensor of shape [6, S, S, C]")
    h, w = _envmap_res(res, "cubemap_to_latlong")
    return _EnvResample.apply(cubemap[None], _TEX_BOUNDARIES["cube"], 1, h, w)[0]


# ---------------------------------------------------------------------------------------------- environment light
ENV_MAX_RES = 4096  # ENV_MAX_N of csrc/envlight.hip
ENV_MAX_DIFFUSE_RES = 256  # ENV_MAX_DIFFUSE_N: the diffuse filter is all pairs, 36 N^4 (the light runs it at 16)
_env_area_cache = {}


def cubemap_axis_area(res, device=None, dtype=torch.float32):
    """The N per-axis factors of the texel solid angle, area(x, y) = axis[x] * axis[y]: with H = N // 2 and x' = |x - H|,
    axis[x] = atan((x' + 1) / H) - atan(x' / H), and 1 when N == 1.  Computed in float64 (the difference of two fp32 atans loses about
    log2(N) bits), cached per (N, device) as float32.  This is the formula the reference's environment lights were trained with, kept
    as it stands: for even N the texels left of the centre get x' = H - x (1..H, not 0..H-1), so the areas are not mirror-symmetric
    and sum to more than 4 pi (1.08 x at N = 16)."""
    res = int(res)
    if res == 1:
        axis = torch.ones(1, dtype=torch.float64)
    else:
        H = res // 2
        xp = (torch.arange(res, dtype=torch.float64) - H).abs()
        axis = torch.atan((xp + 1) / H) - torch.atan(xp / H)
    if device is None:
        return axis.to(dtype)
    key = (res, str(torch.device(device)))
    if key not in _env_area_cache:
        _env_area_cache[key] = axis.to(torch.float32).to(device)
    return _env_area_cache[key]


def _env_check_map(t, channels, what, max_res=ENV_MAX_RES):
    if t.dim() != 4 or t.shape[0] != 6 or t.shape[1] != t.shape[2] or t.shape[3] != channels or t.shape[1] < 1:
        raise ValueError(f"{what}: expected a cube map of shape [6, N, N, {channels}], got {list(t.shape)}")
    if t.shape[1] > max_res:
        raise ValueError(f"{what}: face size {t.shape[1]} is above the supported {max_res}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: expected a float32 tensor, got {t.dtype}")


def _env_desc(N, src, dst, area, bounds=None, roughness=1.0, cutoff=0.0):
    return _lib.EnvDesc(size=ctypes.sizeof(_lib.EnvDesc), N=N, roughness=roughness, costheta_cutoff=cutoff, src=ptr(src), dst=ptr(dst),
                        bounds=ptr(bounds), area=ptr(area))


class _DiffuseCubemap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cubemap):
        cubemap = f32c(cubemap)
        N = cubemap.shape[1]
        out = torch.empty_like(cubemap)
        call("a3d_cubemap_diffuse_fwd", ctypes.byref(_env_desc(N, cubemap, out, cubemap_axis_area(N, cubemap.device))), stream())
        ctx.N = N
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        g_out = f32c(g_out)
        g_in = torch.empty_like(g_out)
        call("a3d_cubemap_diffuse_bwd", ctypes.byref(_env_desc(ctx.N, g_out, g_in, cubemap_axis_area(ctx.N, g_out.device))), stream())
        return g_in


def diffuse_cubemap(cubemap):
    """The cosine-lobe irradiance filter of a cube map (csrc/envlight.hip), [6,N,N,3] float32 on the GPU -> the same shape; the
    arithmetic of the reference plugin's diffuse_cubemap (renderutils/ops.py:404-411), restated:

    Texel (x, y) of face f points along d = normalize(cube_to_dir(f, fx, fy)), fx = 2 (x + 0.5) / N - 1, fy = 2 (y + 0.5) / N - 1:
    face 0 (1,-fy,-fx), 1 (-1,-fy,fx), 2 (fx,1,fy), 3 (fx,-1,-fy), 4 (fx,-fy,1), 5 (-fx,-fy,-1) -- the cube convention of
    texture(boundary_mode='cube').  area(q) is the texel solid angle of cubemap_axis_area().

        out[p] = sum over ALL 6 N^2 texels q of in[q] * clamp(dot(d_p, d_q), 0, 0.999) * area(q) / pi

    Gradient to the map: g_in[q] = area(q) / pi * sum_p g_out[p] * clamp(dot(d_p, d_q), 0, 0.999), computed as a gather (one lane per
    q, no atomics): two calls on the same input return the same bits.
    Every texel is filtered against every texel (36 N^4 pairs), so N <= 256 (ValueError above: mip the map down first, as
    EnvironmentLight.build_mips does to 16)."""
    _env_check_map(cubemap, 3, "diffuse_cubemap", ENV_MAX_DIFFUSE_RES)
    require_device(cubemap, what="diffuse_cubemap")
    return _DiffuseCubemap.apply(cubemap)


def specular_bounds(res, costheta_cutoff, device):
    """int16 [6,N,N,6,4]: for every output texel p and source face s, (xmin, xmax, ymin, ymax) over the texels q of face s with
    dot(d_q, d_p) >= costheta_cutoff, and (N-1, 0, N-1, 0) where there is none.  Found by the exhaustive test on the device (a one-off
    per (N, cutoff)); the directions and the dot are the filter's own, so the table is exact for it."""
    res = int(res)
    if not 1 <= res <= 32767:
        raise ValueError(f"specular_bounds: res must be 1 .. 32767 (the table is int16), got {res}")
    if not -1.0 <= float(costheta_cutoff) <= 1.0:
        raise ValueError(f"specular_bounds: costheta_cutoff must be a cosine, got {costheta_cutoff}")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.A3DError(f"specular_bounds: device {device}; the HIP hot path only runs on a ROCm device (no CPU fallback)")
    with torch.cuda.device(device):
        bounds = torch.empty((6, res, res, 6, 4), dtype=torch.int16, device=device)
        call("a3d_cubemap_specular_bounds", ctypes.byref(_env_desc(res, None, None, None, bounds, 1.0, float(costheta_cutoff))), stream())
    return bounds


class _SpecularCubemap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cubemap, roughness, costheta_cutoff, bounds):
        cubemap = f32c(cubemap)
        N = cubemap.shape[1]
        out = torch.empty((6, N, N, 4), dtype=torch.float32, device=cubemap.device)
        call("a3d_cubemap_specular_fwd", ctypes.byref(_env_desc(N, cubemap, out, cubemap_axis_area(N, cubemap.device), bounds, roughness,
                                                                costheta_cutoff)), stream(), tag=f"[N{N}]")
        ctx.cfg = (N, roughness, costheta_cutoff)
        ctx.save_for_backward(bounds)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        N, roughness, costheta_cutoff = ctx.cfg
        bounds, = ctx.saved_tensors
        g_out = f32c(g_out)
        g_in = torch.empty((6, N, N, 3), dtype=torch.float32, device=g_out.device)
        call("a3d_cubemap_specular_bwd", ctypes.byref(_env_desc(N, g_out, g_in, cubemap_axis_area(N, g_out.device), bounds, roughness,
                                                                costheta_cutoff)), stream(), tag=f"[N{N}]")
        return g_in, None, None, None


def specular_cubemap_raw(cubemap, roughness, costheta_cutoff, bounds):
    """The GGX-lobe filter of a cube map (csrc/envlight.hip): [6,N,N,3] float32 on the GPU -> [6,N,N,4] = (weighted colour sum, weight
    sum); the arithmetic of the reference plugin's specular_cubemap_fwd (renderutils/ops.py:413-425), restated.  Directions and area(q)
    as in diffuse_cubemap().  With a2 = roughness^4 and c = costheta_cutoff, over all q with dot(d_q, d_p) >= c:

        h = normalize(d_q + d_p),  t = clamp(dot(d_p, h), 0, 1),  D = a2 / (pi * ((t * a2 - t) * t + 1)^2)
        w = max(dot(d_q, d_p), 0) * D * area(q) / 4,              out[p] = (sum w * in[q], sum w)

    ``bounds`` = specular_bounds(N, c, device): the filter visits the texels inside those rectangles and applies the cone test itself.
    Gradient to the map only: g_in[q] = sum_p g_out[p][0:3] * w(p, q); channel 3 of g_out is ignored (the weight sum does not depend
    on the map).  w(p, q) = f(p, q) * area(q) with f and the cone test symmetric in p and q, so the backward is a gather through the
    same table (one lane per q, no atomics): two calls on the same input return the same bits.
    fp32 note: at t near 1 the denominator is about a2, so D carries the rounding of t magnified by up to 4 / a2 (1e5 at roughness
    0.08): a raw value agrees with exact arithmetic to about 1e-2 there.  The magnification is common to both components of a texel,
    so it cancels in colour / weight, which is what specular_cubemap returns."""
    _env_check_map(cubemap, 3, "specular_cubemap_raw")
    N = cubemap.shape[1]
    if not float(roughness) > 0.0:
        raise ValueError(f"specular_cubemap_raw: roughness must be positive, got {roughness}")
    if not -1.0 <= float(costheta_cutoff) <= 1.0:
        raise ValueError(f"specular_cubemap_raw: costheta_cutoff must be a cosine, got {costheta_cutoff}")
    if not torch.is_tensor(bounds) or bounds.dtype != torch.int16 or tuple(bounds.shape) != (6, N, N, 6, 4) or not bounds.is_contiguous():
        raise ValueError(f"specular_cubemap_raw: bounds must be a contiguous int16 tensor of shape [6, {N}, {N}, 6, 4] (specular_bounds)")
    require_device(cubemap, bounds, what="specular_cubemap_raw")
    return _SpecularCubemap.apply(cubemap, float(roughness), float(costheta_cutoff), bounds)


# ---------------------------------------------------------------------------------------------- shading BSDFs, HDR image loss
# name -> (op code, channels per input, channels of the result, stem of the entry points, KernelTimer tag): every element-wise operator
# over an a3d_bsdf_desc.  BSDF_OPS / TANGENT_OPS: the rows whose codes include/a3d_bsdf.h / include/a3d_tangent.h define
PIXEL_OPS = {"lambert": (0, (3, 3), 1, "a3d_bsdf", "[lambert]"), "frostbite_diffuse": (1, (3, 3, 3, 1), 1, "a3d_bsdf", "[frostbite_diffuse]"),
             "pbr_specular": (2, (3, 3, 3, 3, 1), 3, "a3d_bsdf", "[pbr_specular]"), "pbr_bsdf": (3, (3, 3, 3, 3, 3, 3), 3, "a3d_bsdf", "[pbr_bsdf]"),
             "image_loss": (4, (1, 1), 1, "a3d_image_loss", None),  # (_ImageLoss tags its calls with the variant)
             "shading_normal": (_lib.SHADING_NORMAL_OP, (3, 3, 3, 3, 3, 3), 3, "a3d_shading_normal", "")}
BSDF_OPS = {name: row[:3] for name, row in PIXEL_OPS.items() if row[0] != _lib.SHADING_NORMAL_OP}
TANGENT_OPS = {name: row[:3] for name, row in PIXEL_OPS.items() if row[0] == _lib.SHADING_NORMAL_OP}
IMAGE_LOSSES = {"l1": 0, "mse": 1, "smape": 2, "relmse": 3}
BSDF_MIN_RUN = 256  # a gradient is reduced inside the launch when its input is constant over runs of at least this many pixels


class _BsdfPlan:
    """How a broadcast element-wise call is handed to the library: the leading shape of the result with neighbouring dimensions merged
    where every input allows it, per input the element strides along those dimensions (0 = broadcast) and the channel stride, and the
    segment length: the shortest run of pixels over which an outer-broadcast input ([B,1,1,3], [1,1,1,3]) is constant."""

    _geometry = {}  # (name, shapes, strides) -> the plan's geometry: a training loop calls with the same few layouts every step

    def __init__(self, name, inputs):
        self.code, chans, self.c_out, self.entry, self.tag = PIXEL_OPS[name]
        self.inputs, self.chans = inputs, chans
        key = (name, tuple((t.shape, t.stride()) for t in inputs))
        geo = self._geometry.get(key)
        if geo is None:
            if len(self._geometry) > 256:
                self._geometry.clear()
            geo = self._geometry[key] = self._plan(name, inputs, chans)
        self.lead, self.shape, self.strides, self.cstrides, self.n, self.run, self.seg = geo

    @staticmethod
    def _plan(name, inputs, chans):
        assert len(inputs) == len(chans)
        for t, c in zip(inputs, chans):
            if t.dim() < 1 or t.shape[-1] not in (1, c):
                raise ValueError(f"{name}: the last dimension of an input must be {c} (or 1), got shape {list(t.shape)}")
        lead = tuple(torch.broadcast_shapes(*[t.shape[:-1] for t in inputs]))
        nd = len(lead)
        strides, bcast = [], []  # per input and leading dimension: element stride (0 where the input has size 1), and "has size 1 there"
        for t in inputs:
            pad = nd - (t.dim() - 1)
            one = [d < pad or t.shape[d - pad] == 1 for d in range(nd)]
            bcast.append(one)
            strides.append([0 if one[d] else t.stride(d - pad) for d in range(nd)])
        # drop dimensions of size 1; merge dimension d into d - 1 where, for every input, stride[d - 1] == stride[d] * size[d] AND the
        # input is broadcast (size 1) along both or along neither: the gradient of an input follows its SHAPE, not its strides -- a
        # light.expand(B, 1, 1, 3) has stride 0 along B too, but wants B rows of gradient
        shape, st, bc = [], [[] for _ in inputs], [[] for _ in inputs]
        for d in range(nd):
            n = lead[d]
            if n == 1:
                continue
            if shape and all(s[-1] == strides[i][d] * n and bc[i][-1] == bcast[i][d] for i, s in enumerate(st)):
                shape[-1] *= n
                for i, s in enumerate(st):
                    s[-1] = strides[i][d]
            else:
                shape.append(n)
                for i, s in enumerate(st):
                    s.append(strides[i][d])
                    bc[i].append(bcast[i][d])
        if not shape:
            shape, st, bc = [1], [[0] for _ in inputs], [[False] for _ in inputs]
        if len(shape) > _lib.BSDF_MAX_DIMS:
            raise _lib.A3DError(f"{name}: the inputs' strides leave {len(shape)} leading dimensions that cannot be merged; at most "
                                f"{_lib.BSDF_MAX_DIMS} are supported (make the most irregular input contiguous)")
        cstrides = [0 if t.shape[-1] == 1 else t.stride(-1) for t in inputs]
        n = math.prod(shape)
        # run[i]: pixels over which input i is constant because it has SIZE 1 along a trailing block of dimensions (and only there), else None
        run = []
        for b in bc:
            k = len(shape)
            while k > 0 and b[k - 1]:
                k -= 1
            r = math.prod(shape[k:])
            run.append(r if (k < len(shape) and not any(b[:k]) and r >= BSDF_MIN_RUN) else None)
        runs = [r for r in run if r]
        return lead, shape, st, cstrides, n, run, (min(runs) if runs else max(n, 1))

    def desc(self):
        d = _lib.BsdfDesc(size=ctypes.sizeof(_lib.BsdfDesc), op=self.code, ndim=len(self.shape), seg=self.seg)
        for j, n in enumerate(self.shape):
            d.shape[j] = n
        for i, t in enumerate(self.inputs):
            getattr(d, "in")[i] = t.data_ptr()
            d.cstride[i] = self.cstrides[i]
            for j, s in enumerate(self.strides[i]):
                d.stride[4 * i + j] = s
        return d

    def rows(self):
        return (self.n // self.seg) * (-(-self.seg // _lib.BSDF_TILE))

    def grads(self, d, needs, device):
        """Gradient buffers for the inputs that want one, set into the descriptor -> a function that turns them into the tensors autograd
        expects once the call has been enqueued."""
        finish = []
        for i, (t, c) in enumerate(zip(self.inputs, self.chans)):
            if not needs[i]:
                finish.append(None)
                continue
            if self.run[i]:  # constant over runs: partial rows + the finishing launch
                rows = torch.empty((self.rows(), c), dtype=torch.float64, device=device)  # (the sums are carried in double)
                final = torch.empty((self.n // self.run[i], c), dtype=torch.float32, device=device)
                d.g_mode[i], d.seg_div[i], d.g_in[i], d.g_final[i] = 2, self.run[i] // self.seg, rows.data_ptr(), final.data_ptr()
                finish.append((final, rows))
            else:  # one row per pixel; any other broadcast pattern (inner dimensions, [1,H,W,3]) is summed by torch afterwards
                g = torch.empty((self.n, c), dtype=torch.float32, device=device)
                d.g_mode[i], d.g_in[i] = 1, g.data_ptr()
                finish.append((g, None))

        def collect():
            out = []
            for i, (t, c) in enumerate(zip(self.inputs, self.chans)):
                if finish[i] is None:
                    out.append(None)
                    continue
                g, rows = finish[i]
                if rows is None:
                    pad = (1,) * (len(self.lead) - (t.dim() - 1))
                    g = g.view(*self.lead, c).sum_to_size(*pad, *t.shape[:-1], t.shape[-1])
                elif t.shape[-1] != c:
                    g = g.sum(-1, keepdim=True)
                out.append(g.reshape(t.shape))
            return out

        return collect


class _Pixel(torch.autograd.Function):
    """ops.bsdf and ops.shading_normal: one launch forward, one backward, through the entry points PIXEL_OPS names."""

    @staticmethod
    def forward(ctx, name, min_roughness, variant, *inputs):
        plan = _BsdfPlan(name, inputs)
        out = torch.empty((*plan.lead, plan.c_out), dtype=torch.float32, device=inputs[0].device)
        if plan.n:
            d = plan.desc()
            d.variant, d.min_roughness, d.out = variant, min_roughness, out.data_ptr()
            call(plan.entry + "_fwd", ctypes.byref(d), stream(), tag=plan.tag)
        ctx.cfg = (name, min_roughness, variant)
        ctx.save_for_backward(*inputs)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        name, min_roughness, variant = ctx.cfg
        inputs = ctx.saved_tensors
        plan = _BsdfPlan(name, inputs)
        needs = ctx.needs_input_grad[3:]
        if not plan.n:
            return (None, None, None) + tuple(torch.zeros_like(t) if n else None for t, n in zip(inputs, needs))
        g_out = f32c(g_out)
        d = plan.desc()
        d.variant, d.min_roughness, d.g_out = variant, min_roughness, g_out.data_ptr()
        collect = plan.grads(d, needs, g_out.device)
        call(plan.entry + "_bwd", ctypes.byref(d), stream(), tag=plan.tag)
        return (None, None, None) + tuple(collect())


def bsdf(name, inputs, min_roughness=0.08, lobe=0):
    """lambert / frostbite_diffuse / pbr_specular / pbr_bsdf of renderutils as ONE launch forward and one backward (csrc/bsdf.hip,
    include/a3d_bsdf.h); the arithmetic is the torch twin's of model/render/renderutils/ops.py, operation by operation.

    ``inputs``: float32 tensors on the GPU in the reference's argument order, [..., 3] (or [..., 1] for linearRoughness / alpha),
    broadcastable against each other in every leading dimension; any strides.  Nothing is expanded: the kernels read through strides.
    Returns [..., 1] (lambert, frostbite_diffuse) or [..., 3] in the broadcast leading shape.
    Gradients: every input that requires one gets it, in its own shape (zeros included).  An input that is broadcast along trailing
    leading dimensions only ([B,1,1,3], [1,1,1,3]: camera, light, a constant colour) has its gradient summed inside the launch
    (registers -> wave -> work-group -> one partial row per work-group, then a finishing launch over the rows; no atomics, bit-identical
    run to run); any other broadcast pattern gets one row per pixel from the launch and a torch sum afterwards."""
    inputs = tuple(inputs)
    for t in inputs:
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: expected float32 tensors, got {t.dtype}")
    require_device(*inputs, what=name)
    return _Pixel.apply(name, float(min_roughness), int(lobe), *inputs)


def _flat_loss_desc(img, target):
    """The descriptor of image_loss for two contiguous images of one shape, written down directly (one dimension of n elements, unit
    strides): the common call, and one whose kernels take tens of microseconds -- the general plan would cost as much again."""
    n = img.numel()
    d = _lib.BsdfDesc(size=ctypes.sizeof(_lib.BsdfDesc), op=4, ndim=1, seg=n)
    d.shape[0] = n
    ins = getattr(d, "in")
    ins[0], ins[1] = img.data_ptr(), target.data_ptr()
    d.stride[0] = d.stride[4] = d.cstride[0] = d.cstride[1] = 1
    return d, n


class _ImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, target, variant):
        flat = img.shape == target.shape and img.is_contiguous() and target.is_contiguous()
        if flat:
            d, n = _flat_loss_desc(img, target)
            rows = -(-n // _lib.BSDF_TILE)
        else:
            plan = _BsdfPlan("image_loss", (img.unsqueeze(-1), target.unsqueeze(-1)))
            d, rows = plan.desc(), plan.rows()
        out = torch.empty((), dtype=torch.float32, device=img.device)
        scratch = torch.empty((rows,), dtype=torch.float64, device=img.device)
        d.variant, d.out, d.scratch = variant, out.data_ptr(), scratch.data_ptr()
        call("a3d_image_loss_fwd", ctypes.byref(d), stream(), tag=_LOSS_TAGS[variant])
        ctx.variant, ctx.flat = variant, flat
        ctx.save_for_backward(img, target)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        img, target = ctx.saved_tensors
        g_out = f32c(g_out)
        if ctx.flat:
            d, _ = _flat_loss_desc(img, target)
            d.variant, d.g_out = ctx.variant, g_out.data_ptr()
            gi = gt = None
            if ctx.needs_input_grad[0]:
                gi = torch.empty_like(img)
                d.g_mode[0], d.g_in[0] = 1, gi.data_ptr()
            if ctx.needs_input_grad[1]:
                gt = torch.empty_like(target)
                d.g_mode[1], d.g_in[1] = 1, gt.data_ptr()
            call("a3d_image_loss_bwd", ctypes.byref(d), stream(), tag=_LOSS_TAGS[ctx.variant])
            return gi, gt, None
        plan = _BsdfPlan("image_loss", (img.unsqueeze(-1), target.unsqueeze(-1)))
        d = plan.desc()
        d.variant, d.g_out = ctx.variant, g_out.data_ptr()
        collect = plan.grads(d, ctx.needs_input_grad[:2], g_out.device)
        call("a3d_image_loss_bwd", ctypes.byref(d), stream(), tag=_LOSS_TAGS[ctx.variant])
        gi, gt = collect()
        return (None if gi is None else gi.squeeze(-1)), (None if gt is None else gt.squeeze(-1)), None


_LOSS_TAGS = [f"[{v}]" for v in range(8)]


def image_loss(img, target, loss="l1", tonemapper="none"):
    """The HDR image loss of renderutils as a scalar (the mean over all elements), csrc/bsdf.hip: 'l1' | 'mse' | 'smape' | 'relmse'
    (any other name is l1, as in the reference), after the optional tone map 'log_srgb' = srgb(log(clamp(x, 0, 65535) + 1)).  The forward
    sums per work-group and finishes over the partial sums in a fixed order (no atomics); the backward is element-wise.  img and target
    are float32 on the GPU, broadcastable against each other, any strides."""
    if img.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"image_loss: expected float32 tensors, got {img.dtype} and {target.dtype}")
    require_device(img, target, what="image_loss")
    if img.dim() == 0 or target.dim() == 0:
        img, target = img.reshape(-1) if img.dim() == 0 else img, target.reshape(-1) if target.dim() == 0 else target
    if img.numel() == 0 or target.numel() == 0:
        return (img * target).mean()  # (the mean of nothing: nan, as torch's)
    return _ImageLoss.apply(img, target, IMAGE_LOSSES.get(loss, 0) + 4 * (tonemapper == "log_srgb"))


# ---------------------------------------------------------------------------------------------- tangent frame (include/a3d_tangent.h)
def shading_normal(pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm, two_sided_shading=True, opengl=True):
    """prepare_shading_normal of renderutils WITH a tangent-space perturbation as one launch forward and one backward (csrc/tangent.hip,
    include/a3d_tangent.h); the arithmetic is the torch statements of model/render/renderutils/ops.py, operation by operation.

    Six float32 tensors on the GPU, [..., 3], broadcastable against each other in every leading dimension, any strides (a channel slice
    ``all_tex[..., 6:9]`` is read in place).  Returns [..., 3] in the broadcast leading shape.  Gradients as ops.bsdf's: an input that is
    broadcast along trailing leading dimensions only (view_pos [B,1,1,3], a constant perturbation [1,1,1,3]) is summed inside the launch
    in double, without atomics, bit-identical run to run.  The forward is float32; the backward carries its arithmetic in double."""
    inputs = (pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm)
    for t in inputs:
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"shading_normal: expected float32 tensors, got {getattr(t, 'dtype', type(t))}")
    require_device(*inputs, what="shading_normal")
    return _Pixel.apply("shading_normal", 0.0, int(bool(two_sided_shading)) + 2 * int(bool(opengl)), *inputs)  # (no min_roughness: the field stays 0)


def _tangent_atlas(v_tex, B):
    """(v_tex as the kernel reads it, elements between the images' atlases): [1,Nuv,2] and stride-0 views of it are passed on as they
    are (batch stride 0), never expanded in memory."""
    if v_tex.shape[0] not in (1, B):
        raise ValueError(f"vertex_tangents: v_tex has {v_tex.shape[0]} atlases for {B} meshes")
    if v_tex.shape[0] == 1 or v_tex.stride(0) == 0:
        return f32c(v_tex[0:1]), 0
    v_tex = f32c(v_tex)
    return v_tex, v_tex.stride(0)


class _Tangents(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v_pos, v_nrm, v_tex, tri32, tex32, adjacency):
        v_pos, v_nrm = f32c(v_pos), f32c(v_nrm)
        B, V, F = v_pos.shape[0], v_pos.shape[1], tri32.shape[0]
        v_tex, tex_stride = _tangent_atlas(v_tex, B)
        v_tng = torch.empty_like(v_pos)
        call("a3d_tangents_fwd", ptr(v_pos), ptr(v_tex), tex_stride, ptr(v_nrm), ptr(tri32), ptr(tex32), ptr(adjacency.off), ptr(adjacency.adj),
             adjacency.stride, B, V, F, ptr(v_tng), stream(), tag=f"[B{B}]")
        ctx.save_for_backward(v_pos, v_nrm, v_tex, tri32, tex32)
        ctx.adjacency, ctx.tex_stride = adjacency, tex_stride
        return v_tng

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_tng):
        v_pos, v_nrm, v_tex, tri32, tex32 = ctx.saved_tensors
        B, V, F = v_pos.shape[0], v_pos.shape[1], tri32.shape[0]
        g_tng = f32c(g_tng)
        scratch = torch.empty((B, V, 3), dtype=torch.float64, device=v_pos.device)
        g_pos, g_nrm = torch.empty_like(v_pos), torch.empty_like(v_pos)
        call("a3d_tangents_bwd", ptr(g_tng), ptr(v_pos), ptr(v_tex), ctx.tex_stride, ptr(v_nrm), ptr(tri32), ptr(tex32), ptr(ctx.adjacency.off),
             ptr(ctx.adjacency.adj), ctx.adjacency.stride, B, V, F, ptr(scratch), ptr(g_pos), ptr(g_nrm), stream(), tag=f"[B{B}]")
        return g_pos, g_nrm, None, None, None, None


def vertex_tangents(v_pos, v_tex, v_nrm, t_pos_idx, t_tex_idx):
    """Per-vertex tangents [B,V,3] of compute_tangents (reference mesh.py:310-350) for a mesh whose normals are indexed by t_pos_idx:
    one launch forward, two backward (csrc/tangent.hip), gradients to v_pos and v_nrm, none to the static atlas v_tex ([1,Nuv,2], a
    stride-0 expansion of it, or [B,Nuv,2]).  The vertex -> face lists are vertex_face_adjacency's, built once per triangle list."""
    for t in (v_pos, v_tex, v_nrm):
        if t.dtype != torch.float32:
            raise ValueError(f"vertex_tangents: expected float32 tensors, got {t.dtype}")
    if v_tex.requires_grad and torch.is_grad_enabled():
        raise ValueError("vertex_tangents: v_tex receives no gradient from the kernels (the atlas is static); detach it or use the torch statements")
    tri32, tex32 = tri_int32(t_pos_idx), tri_int32(t_tex_idx)
    require_device(v_pos, v_tex, v_nrm, tri32, tex32, what="vertex_tangents")
    if v_pos.dim() != 3 or v_pos.shape != v_nrm.shape or v_pos.shape[2] != 3 or tex32.shape != tri32.shape or v_tex.dim() != 3 or v_tex.shape[2] != 2:
        raise ValueError(f"vertex_tangents: v_pos {list(v_pos.shape)}, v_nrm {list(v_nrm.shape)}, v_tex {list(v_tex.shape)}, "
                         f"t_pos_idx {list(tri32.shape)}, t_tex_idx {list(tex32.shape)}")
    if tri32.shape[0] == 0 or v_pos.shape[0] == 0 or v_pos.shape[1] == 0:
        return torch.full_like(v_pos, float("nan")) + 0 * (v_pos + v_nrm)  # (no face anywhere: 0 / 0 at every vertex, as the torch statements)
    return _Tangents.apply(v_pos, v_nrm, v_tex, tri32, tex32, vertex_face_adjacency(tri32, v_pos.shape[1]))


# ---------------------------------------------------------------------------------------------- mesh regularisers (include/a3d_reg.h)
class EdgeTopology:
    """The per-occurrence edge table of one triangle list (a3d_edge_topology): int32 [3F,2] rows (A3D_EDGE_* bits, partner face) and the
    number of unique edges as a device int32 that is never read back.  Built from the vertex -> face lists in one launch."""

    def __init__(self, tri32: torch.Tensor, num_vertices: int, adjacency=None):
        require_device(tri32, what="edge_topology")
        F, V = tri32.shape[0], int(num_vertices)
        self.tri, self.num_vertices = tri32, V
        self.adjacency = adjacency if adjacency is not None else vertex_face_adjacency(tri32, V)
        self.table = torch.empty((3 * F, 2), dtype=torch.int32, device=tri32.device)
        self.num_edges = torch.empty(1, dtype=torch.int32, device=tri32.device)
        call("a3d_edge_topology", ptr(tri32), F, V, ptr(self.adjacency.off), ptr(self.adjacency.adj), self.adjacency.stride, ptr(self.table),
             ptr(self.num_edges), stream())


_edge_cache = _IdentityCache()


def edge_topology(tri32: torch.Tensor, num_vertices: int) -> EdgeTopology:
    """EdgeTopology of a non-empty triangle list, built on first use and cached per list (as the vertex -> face lists it is built from)."""
    hit = _edge_cache.peek(tri32)
    if hit is None or hit.num_vertices != num_vertices:
        hit = _edge_cache.put(tri32, EdgeTopology(tri32, num_vertices))
    return hit


def _reg_partials(v_pos, n):
    return torch.empty(_lib.lib().a3d_reg_partials(v_pos.shape[0], n), dtype=torch.float64, device=v_pos.device)


class _Laplace(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v_pos, tri32, adjacency):
        v_pos = f32c(v_pos)
        B, V, F = v_pos.shape[0], v_pos.shape[1], tri32.shape[0]
        scaled = torch.empty((B, V, 3), dtype=torch.float64, device=v_pos.device)
        loss = torch.empty((), dtype=torch.float32, device=v_pos.device)
        call("a3d_laplace_fwd", ptr(v_pos), ptr(tri32), ptr(adjacency.off), ptr(adjacency.adj), adjacency.stride, B, V, F, ptr(scaled),
             ptr(_reg_partials(v_pos, V)), ptr(loss), stream(), tag=f"[B{B}]")
        ctx.save_for_backward(scaled, tri32)
        ctx.adjacency = adjacency
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        scaled, tri32 = ctx.saved_tensors
        B, V, F = scaled.shape[0], scaled.shape[1], tri32.shape[0]
        g_v = torch.empty((B, V, 3), dtype=torch.float32, device=scaled.device)
        call("a3d_laplace_bwd", ptr(f32h(g_loss)), ptr(scaled), ptr(tri32), ptr(ctx.adjacency.off), ptr(ctx.adjacency.adj), ctx.adjacency.stride,
             B, V, F, ptr(g_v), stream(), tag=f"[B{B}]")
        return g_v, None, None


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v_pos, tri32, edges):
        v_pos = f32c(v_pos)
        B, V, F = v_pos.shape[0], v_pos.shape[1], tri32.shape[0]
        stand_in = torch.empty((B, 3), dtype=torch.float64, device=v_pos.device)
        loss = torch.empty((), dtype=torch.float32, device=v_pos.device)
        call("a3d_normal_consistency_fwd", ptr(v_pos), ptr(tri32), ptr(edges.table), ptr(edges.num_edges), B, V, F, ptr(stand_in),
             ptr(_reg_partials(v_pos, F)), ptr(loss), stream(), tag=f"[B{B}]")
        ctx.save_for_backward(v_pos, stand_in, tri32)
        ctx.edges = edges
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        v_pos, stand_in, tri32 = ctx.saved_tensors
        B, V, F = v_pos.shape[0], v_pos.shape[1], tri32.shape[0]
        edges, adjacency = ctx.edges, ctx.edges.adjacency
        scratch = torch.empty((B, F, 9), dtype=torch.float64, device=v_pos.device)
        g_v = torch.empty_like(v_pos)
        call("a3d_normal_consistency_bwd", ptr(f32h(g_loss)), ptr(v_pos), ptr(tri32), ptr(edges.table), ptr(edges.num_edges), ptr(adjacency.off),
             ptr(adjacency.adj), adjacency.stride, ptr(stand_in), B, V, F, ptr(scratch), ptr(g_v), stream(), tag=f"[B{B}]")
        return g_v, None, None


class _EdgeLength(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v_pos, tri32, edges):
        v_pos = f32c(v_pos)
        B, V, F = v_pos.shape[0], v_pos.shape[1], tri32.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=v_pos.device)
        call("a3d_edge_length_fwd", ptr(v_pos), ptr(tri32), ptr(edges.table), ptr(edges.num_edges), B, V, F, ptr(_reg_partials(v_pos, F)),
             ptr(loss), stream(), tag=f"[B{B}]")
        ctx.save_for_backward(v_pos, tri32)
        ctx.edges = edges
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        v_pos, tri32 = ctx.saved_tensors
        B, V, F = v_pos.shape[0], v_pos.shape[1], tri32.shape[0]
        edges, adjacency = ctx.edges, ctx.edges.adjacency
        g_v = torch.empty_like(v_pos)
        call("a3d_edge_length_bwd", ptr(f32h(g_loss)), ptr(v_pos), ptr(tri32), ptr(edges.table), ptr(edges.num_edges), ptr(adjacency.off),
             ptr(adjacency.adj), adjacency.stride, B, V, F, ptr(g_v), stream(), tag=f"[B{B}]")
        return g_v, None, None


def _reg_args(what, v_pos, t_pos_idx):
    """(tri32, empty) after the checks the three regularisers share: v_pos float32 [B,V,3], t_pos_idx an integer [1,F,3] or [F,3], both on
    the current device."""
    if not torch.is_tensor(v_pos) or v_pos.dtype != torch.float32:
        raise ValueError(f"{what}: expected a float32 v_pos, got {getattr(v_pos, 'dtype', type(v_pos))}")
    if not torch.is_tensor(t_pos_idx) or t_pos_idx.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: expected int32 / int64 indices, got {getattr(t_pos_idx, 'dtype', type(t_pos_idx))}")
    if v_pos.dim() != 3 or v_pos.shape[2] != 3 or t_pos_idx.dim() not in (2, 3) or t_pos_idx.shape[-1] != 3 or (t_pos_idx.dim() == 3 and t_pos_idx.shape[0] != 1):
        raise ValueError(f"{what}: v_pos {list(v_pos.shape)}, t_pos_idx {list(t_pos_idx.shape)}; expected [B,V,3] and [1,F,3]")
    tri32 = tri_int32(t_pos_idx)
    require_device(v_pos, tri32, what=what)
    return tri32, tri32.shape[0] == 0 or v_pos.shape[0] == 0 or v_pos.shape[1] == 0


def laplace_regularizer(v_pos, t_pos_idx):
    """laplace_regularizer_const (reference regularizer.py:40-61, with the [B,F,1] index its normaliser evidently means): the mean square
    of the umbrella term, two launches forward and one backward (csrc/regularizer.hip), double sums in a fixed order -> a float32 scalar
    with the same bits on every run.  v_pos float32 [B,V,3] on the GPU, t_pos_idx [1,F,3]."""
    tri32, empty = _reg_args("laplace_regularizer", v_pos, t_pos_idx)
    if v_pos.numel() == 0:
        return (v_pos ** 2).mean()  # (the mean of nothing: nan, as the torch statements)
    if empty:
        return (v_pos * 0).mean()  # (no face: every term is 0 / 1)
    return _Laplace.apply(v_pos, tri32, vertex_face_adjacency(tri32, v_pos.shape[1]))


def normal_consistency(v_pos, t_pos_idx):
    """normal_consistency (reference regularizer.py:66-84): mean over the unique edges of (1 - n_col0 . n_col1) / 2, with
    compute_edge_to_face_mapping's columns as the CPU's sequential index put leaves them (face 0 where no face wrote).  Two launches each
    way plus one a3d_edge_topology launch on first use of a triangle list; the number of edges stays on the device."""
    tri32, empty = _reg_args("normal_consistency", v_pos, t_pos_idx)
    if empty:
        return v_pos.sum() * float("nan")  # (no edge, or no image: the mean of nothing)
    return _NormalConsistency.apply(v_pos, tri32, edge_topology(tri32, v_pos.shape[1]))


def avg_edge_length(v_pos, t_pos_idx):
    """avg_edge_length (reference regularizer.py:31-34): the mean length of the unique edges over the batch.  Two launches forward, one
    backward, plus one a3d_edge_topology launch on first use of a triangle list."""
    tri32, empty = _reg_args("avg_edge_length", v_pos, t_pos_idx)
    if empty:
        return v_pos.sum() * float("nan")
    return _EdgeLength.apply(v_pos, tri32, edge_topology(tri32, v_pos.shape[1]))


# ---------------------------------------------------------------------------------------------- environment-lit shading (include/a3d_envshade.h)
class _EnvShadePlan:
    """How the five per-pixel inputs of env_shade reach the library: per input the element strides between pixels and between images
    (0 = broadcast), or "copy" where the strides cannot say it (a row stride that is not W pixel strides, a channel stride other than 1,
    an input broadcast along H or W only), and the filled descriptors.  Cached per (shapes, strides): a training loop calls with the
    same few layouts every step, and a call then copies a descriptor and sets its pointers."""

    _geometry = {}

    def __init__(self, inputs):
        key = tuple((tuple(t.shape), t.stride()) for t in inputs)
        geo = self._geometry.get(key)
        if geo is None:
            if len(self._geometry) > 256:
                self._geometry.clear()
            geo = self._geometry[key] = self._plan(inputs) + ({},)
        self.bhw, self.strides, self.templates = geo

    @staticmethod
    def _plan(inputs):
        for t in inputs:
            if t.dim() != 4 or t.shape[-1] != 3:
                raise ValueError(f"env_shade: a per-pixel input must have shape [B, H, W, 3], got {list(t.shape)}")
        B, H, W = torch.broadcast_shapes(*[t.shape[:-1] for t in inputs])
        strides = []
        for t in inputs:
            b, h, w, _ = t.shape
            img = 0 if b == 1 else t.stride(0)
            if h == 1 and w == 1:
                pix = 0
            elif (h, w) != (H, W) or (h > 1 and w > 1 and t.stride(1) != w * t.stride(2)):
                pix = None
            else:
                pix = t.stride(2) if w > 1 else t.stride(1)
            ok = pix is not None and t.stride(3) == 1 and pix >= 0 and img >= 0
            strides.append((pix, img) if ok else None)  # None: an expanded contiguous copy, strides (3, 3 H W)
        return (B, H, W), strides

    def resolve(self, inputs):
        """-> the tensors the descriptor points at: the inputs, or an expanded contiguous copy where the strides cannot say the layout."""
        B, H, W = self.bhw
        return [t if s is not None else t.expand(B, H, W, 3).contiguous() for t, s in zip(inputs, self.strides)]

    def desc(self, cfg, maps, tensors):
        """The descriptor of a call: every field that follows from (cfg, map sizes, shapes, strides) is filled once per plan and copied;
        a call sets its pointers."""
        diffuse, fg, mtx, spec = maps
        key = (cfg, diffuse.shape[1], None if fg is None else (fg.shape[1], fg.shape[2]), None if mtx is None else mtx.shape[0],
               tuple(t.shape[1] for t in spec))
        tmpl = self.templates.get(key)
        if tmpl is None:
            specular, lo, hi, n_spec = cfg
            B, H, W = self.bhw
            tmpl = _lib.EnvShadeDesc(size=ctypes.sizeof(_lib.EnvShadeDesc), levels=n_spec, diffuse_size=diffuse.shape[1], specular=int(specular),
                                     mtx_batch=0 if mtx is None else mtx.shape[0], B=B, H=H, W=W, min_roughness=lo, max_roughness=hi)
            if fg is not None:
                tmpl.fg_height, tmpl.fg_width = fg.shape[1], fg.shape[2]
            for l, t in enumerate(spec):
                tmpl.spec_size[l] = t.shape[1]
            for i, st in enumerate(self.strides):
                tmpl.pixel_stride[i], tmpl.image_stride[i] = st if st is not None else (3, 3 * H * W)
            if len(self.templates) > 16:
                self.templates.clear()
            self.templates[key] = tmpl
        d = _lib.EnvShadeDesc.from_buffer_copy(tmpl)
        d.diffuse, d.fg, d.mtx = diffuse.data_ptr(), ptr(fg), ptr(mtx)
        for l, t in enumerate(spec):
            d.spec[l] = t.data_ptr()
        ins = getattr(d, "in")
        for i, t in enumerate(tensors):
            ins[i] = t.data_ptr()
        return d


class _EnvShade(torch.autograd.Function):
    """ops.env_shade: one launch forward (a3d_env_shade_fwd), one backward (a3d_env_shade_bwd); nothing is saved but the inputs."""

    @staticmethod
    def forward(ctx, cfg, diffuse, fg, mtx, pos, nrm, kd, ks, view, *spec):
        ctx.set_materialize_grads(False)
        inputs = (pos, nrm, kd, ks, view)
        plan = _EnvShadePlan(inputs)
        B, H, W = plan.bhw
        out = torch.empty((B, H, W, 3), dtype=torch.float32, device=pos.device)
        tensors = plan.resolve(inputs)
        if out.numel():
            d = plan.desc(cfg, (diffuse, fg, mtx, spec), tensors)
            d.out = out.data_ptr()
            call("a3d_env_shade_fwd", ctypes.byref(d), stream())
        ctx.cfg, ctx.shapes, ctx.n_spec, ctx.plan = cfg, [t.shape for t in inputs], len(spec), plan
        ctx.save_for_backward(diffuse, fg, mtx, *tensors, *spec)  # (the tensors the kernel read: a copy made above is not made again)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        none = (None,) * (9 + ctx.n_spec)
        if g_out is None:
            return none
        diffuse, fg, mtx, *rest = ctx.saved_tensors
        tensors, spec = rest[:5], rest[5:]
        needs = ctx.needs_input_grad
        dev = g_out.device
        plan = ctx.plan  # (the forward's: the saved tensors are the ones it resolved, its strides are theirs)
        B, H, W = plan.bhw
        need_in = [needs[4] or needs[8], needs[5], needs[6], needs[7]]  # g_view is -g_pos
        g_dif = torch.zeros_like(diffuse) if needs[1] else None
        g_spec = [torch.zeros_like(t) if needs[9 + l] and ctx.cfg[0] else None for l, t in enumerate(spec)]
        g_in = [torch.empty((B, H, W, 3), dtype=torch.float32, device=dev) if n else None for n in need_in]
        if g_out.numel():
            d = plan.desc(ctx.cfg, (diffuse, fg, mtx, spec), tensors)
            d.g_out = f32h(g_out).data_ptr()
            d.g_diffuse = ptr(g_dif)
            for l, g in enumerate(g_spec):
                d.g_spec[l] = ptr(g)
            for j, g in enumerate(g_in):
                d.g_in[j] = ptr(g)
            call("a3d_env_shade_bwd", ctypes.byref(d), stream())
        fit = lambda g, shape: g.sum_to_size(shape)
        g_pos, g_nrm, g_kd, g_ks = g_in
        return (None, g_dif, None, None,
                fit(g_pos, ctx.shapes[0]) if needs[4] else None, fit(g_nrm, ctx.shapes[1]) if needs[5] else None,
                fit(g_kd, ctx.shapes[2]) if needs[6] else None, fit(g_ks, ctx.shapes[3]) if needs[7] else None,
                fit(-g_pos, ctx.shapes[4]) if needs[8] else None,
                *[(torch.zeros_like(t) if g is None else g) if needs[9 + l] else None for l, (t, g) in enumerate(zip(spec, g_spec))])


def env_shade(diffuse, specular_levels, fg, gb_pos, gb_normal, kd, ks, view_pos, mtx=None, specular=True, min_roughness=0.08, max_roughness=0.5):
    """EnvironmentLight.shade (model/render/light.py, reference light.py:90-128) as ONE launch forward and one backward (csrc/envshade.hip,
    include/a3d_envshade.h): the statements of light.py operation by operation in float32, the three lookups by ops.texture's own device
    code (its docstring is their specification).

    diffuse [6,S,S,3]; specular_levels: at least 3 maps [6,S_l,S_l,3] under the halving rule; fg [1,Hf,Wf,2] (light._fg_lut); all float32
    on the GPU, contiguous (a copy is made otherwise).  gb_pos, gb_normal, kd, ks, view_pos: float32 [b,h,w,3], each either the full
    [B,H,W,3] or broadcast over the image ([B,1,1,3], [1,1,1,3]) or the batch; read in place through their strides (a slice
    ``all_tex[..., 3:6]`` is not copied).  mtx: None or a float32 [1,4,4] / [B,4,4] lookup transform, whose 3 x 3 part rotates both
    lookup directions; it receives no gradient.  min_roughness / max_roughness: the lo / hi of the level rule (get_mip).  -> [B,H,W,3].

    Gradients: gb_pos, gb_normal, kd, ks, one row per pixel, bit-identical run to run; view_pos = the sum of -g_pos over what it is
    broadcast along; diffuse and every specular level, summed in LDS per work-group where the level is at most 16 x 16 and with
    ops.texture's in-wave merge otherwise (float atomics: the last bits depend on the order).  Subgradients at the clamps are autograd's.
    The FG table gets none.  No double backward."""
    spec = list(specular_levels)
    pix = (gb_pos, gb_normal, kd, ks, view_pos)
    maps = [diffuse] + spec + ([fg] if fg is not None else []) + ([mtx] if mtx is not None else [])
    for t in list(pix) + maps:
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"env_shade: expected float32 tensors, got {getattr(t, 'dtype', type(t))}")
    for t in [diffuse] + spec:
        if t.dim() != 4 or t.shape[0] != 6 or t.shape[1] != t.shape[2] or t.shape[3] != 3:
            raise ValueError(f"env_shade: a map must have shape [6, S, S, 3], got {list(t.shape)}")
    if specular and (fg is None or fg.dim() != 4 or fg.shape[0] != 1 or fg.shape[3] != 2):
        raise ValueError(f"env_shade: the FG table must have shape [1, H, W, 2], got {None if fg is None else list(fg.shape)}")
    require_device(*pix, *maps, what="env_shade")
    b = torch.broadcast_shapes(*[t.shape[:-1] for t in pix])[0] if all(t.dim() == 4 for t in pix) else 0
    if mtx is not None and (mtx.dim() != 3 or tuple(mtx.shape[1:]) != (4, 4) or mtx.shape[0] not in (1, b)):
        raise ValueError(f"env_shade: the lookup transform must be [1,4,4] or [{b},4,4], got {list(mtx.shape)}")
    cfg = (bool(specular), float(min_roughness), float(max_roughness), len(spec))
    return _EnvShade.apply(cfg, diffuse.contiguous(), None if fg is None else fg.contiguous(), None if mtx is None else mtx.detach().contiguous(),
                           *pix, *[t.contiguous() for t in spec])


# ---------------------------------------------------------------------------------------------- SDF sign-agreement regulariser (include/a3d_sdfreg.h)
def edge_incidence(edges32: torch.Tensor, num_vertices: int):
    """(off int32 [Nv + 1], inc int32 [2 Ne]) of an int32 edge list [Ne,2] with indices in [0, Nv): the entries 2 * edge + side of vertex
    v are inc[off[v] : off[v + 1]], in ascending order -- every (edge, side) once, under the vertex edges32[edge, side].  A stable sort
    over both endpoints; runs wherever the list lives (one host synchronisation on the GPU: the counts)."""
    ends = edges32.reshape(-1).long()
    inc = torch.sort(ends, stable=True).indices.to(torch.int32)
    off = torch.zeros(int(num_vertices) + 1, dtype=torch.int64, device=ends.device)
    off[1:] = torch.cumsum(torch.bincount(ends, minlength=int(num_vertices)), 0)
    return off.to(torch.int32), inc.contiguous()


class SdfEdges:
    """What sdf_bce_reg_loss keeps per edge tensor: the contiguous, 16-byte aligned int32 rows the kernels stream, the smallest and largest
    index in them (read back once, when the entry is made), and -- from the first backward on -- the vertex -> (edge, side) list."""

    def __init__(self, edges32: torch.Tensor, lo=None, hi=None):
        if edges32.data_ptr() % 16:
            edges32 = edges32.clone()
        self.edges32 = edges32
        if lo is None or hi is None:
            lo, hi = (int(v) for v in torch.stack(torch.aminmax(edges32)).tolist())
        self.lo, self.hi = int(lo), int(hi)
        self._incidence = None

    def check(self, num_vertices: int):
        if self.lo < 0 or self.hi >= num_vertices:
            raise IndexError(f"sdf_bce_reg_loss: edge indices span [{self.lo}, {self.hi}], the SDF has {num_vertices} values")

    def incidence(self, num_vertices: int):
        if self._incidence is None or self._incidence[0] != num_vertices:
            self._incidence = (num_vertices,) + edge_incidence(self.edges32, num_vertices)
        return self._incidence[1:]


_sdf_edges_cache = _IdentityCache(maxsize=2)  # (an entry pins its edge tensor and the int32 rows: 24 B per edge)


def register_grid_edges(all_edges: torch.Tensor, edges32: torch.Tensor, num_vertices: int):
    """A tet grid's own lists (TetGridTopology): sdf_bce_reg_loss on ``all_edges`` streams the existing ``edges32``, no copy, and the
    index range is known by construction.  The entry rides on the tensor object itself, so it lives exactly as long as the grid does."""
    if edges32.is_cuda and edges32.shape[0] > 0:
        all_edges._a3d_sdf_edges = (_IdentityCache.key(all_edges), SdfEdges(edges32, 0, int(num_vertices) - 1))


def sdf_edges(all_edges: torch.Tensor) -> SdfEdges:
    """The cached SdfEdges of an integer [Ne,2] edge tensor, keyed by identity; made (int32 copy, index range) on first use."""
    own = getattr(all_edges, "_a3d_sdf_edges", None)
    if own is not None and own[0] == _IdentityCache.key(all_edges):
        return own[1]
    return _sdf_edges_cache.get(all_edges, lambda t: SdfEdges(t.to(torch.int32).contiguous()))


class _SdfBceReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sdf, cached):
        flat = f32c(sdf).reshape(-1)
        Nv, Ne = flat.shape[0], cached.edges32.shape[0]
        blocks = -(-Ne // _lib.SDF_BCE_BLOCK_EDGES)
        partials = torch.empty(_lib.SDF_BCE_PARTIAL_WORDS * blocks, dtype=torch.float64, device=flat.device)
        state = torch.empty(2, dtype=torch.float64, device=flat.device)
        loss = torch.empty((), dtype=torch.float32, device=flat.device)
        call("a3d_sdf_bce_fwd", ptr(flat), Nv, ptr(cached.edges32), Ne, ptr(partials), ptr(state), ptr(loss), stream())
        ctx.save_for_backward(flat, state)
        ctx.cached, ctx.shape = cached, sdf.shape
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        flat, state = ctx.saved_tensors
        Nv, Ne = flat.shape[0], ctx.cached.edges32.shape[0]
        off, inc = ctx.cached.incidence(Nv)
        g_sdf = torch.empty_like(flat)
        call("a3d_sdf_bce_bwd", ptr(f32h(g_loss)), ptr(flat), Nv, ptr(ctx.cached.edges32), Ne, ptr(off), ptr(inc), ptr(state), ptr(g_sdf), stream())
        return g_sdf.reshape(ctx.shape), None


def sdf_bce_reg_loss(sdf, all_edges):
    """sdf_bce_reg_loss (reference dmtet.py:161-169) of a float32 SDF [Nv] or [Nv,1] over an integer edge tensor [Ne,2], both on the
    current device: two launches forward and one backward (csrc/sdfreg.hip), double sums in a fixed order, no host synchronisation once
    the edge tensor is cached -> a 0-dim float32 tensor with the same bits on every run.  The int32 rows and the index range of an edge
    tensor are cached by identity (a tet grid's own all_edges uses its edges32); an index outside [0, Nv) raises IndexError here, before
    any launch.  The vertex -> (edge, side) list of the backward is built at the first backward of an edge tensor."""
    if not torch.is_tensor(sdf) or sdf.dtype != torch.float32 or not (sdf.dim() == 1 or (sdf.dim() == 2 and sdf.shape[1] == 1)):
        raise ValueError(f"sdf_bce_reg_loss: expected a float32 sdf [Nv] or [Nv,1], got {getattr(sdf, 'dtype', type(sdf))} {list(getattr(sdf, 'shape', []))}")
    if not torch.is_tensor(all_edges) or all_edges.dtype not in (torch.int32, torch.int64) or all_edges.dim() != 2 or all_edges.shape[1] != 2:
        raise ValueError(f"sdf_bce_reg_loss: expected int32 / int64 edges [Ne,2], got {getattr(all_edges, 'dtype', type(all_edges))} "
                         f"{list(getattr(all_edges, 'shape', []))}")
    if sdf.shape[0] == 0 or all_edges.shape[0] == 0:
        raise ValueError("sdf_bce_reg_loss: empty sdf or edge list")
    require_device(sdf, all_edges, what="sdf_bce_reg_loss")
    cached = sdf_edges(all_edges)
    cached.check(sdf.shape[0])
    return _SdfBceReg.apply(sdf, cached)


# ---------------------------------------------------------------------------------------------- exact Euclidean distance transform (include/a3d_edt.h)
def distance_transform(src, scale=1.0, squared=False, return_indices=False, thresholds=None):
    """The exact Euclidean distance of every pixel to the nearest ZERO pixel of its image (csrc/edt.hip: two launches, integers until the
    final store, no atomics, no host synchronisation; the same bits on every run).  No autograd node: the result never requires grad.

    ``src`` uint8 / bool [M,H,W] (non-zero is != 0) -> [M,H,W]; or float32 [N,H,W] with ``thresholds = (t_in, t_out)`` -> [N,2,H,W], both
    channels of the reference's compute_distance_transform from one read of the mask: channel 0 is non-zero where m >= t_in, channel 1
    where m <= t_out, a NaN is zero in both (the reference's np.uint8(m) / np.uint8(1 - m) on a mask in [0,1] is (1, 0)).
    Returns float32 ``(float)(sqrt((double)d2) / scale)`` -- one float64 root, one float64 divide, one rounding -- or, with
    ``squared``, the int32 squared distance d2 itself (above sides of 1024 neighbouring d2 share a float32 root).  With
    ``return_indices`` also int32 ``idx``: the flat index qy * W + qx of a nearest zero pixel, the smallest one among equally near.
    An image WITHOUT a zero pixel gets d2 = H * H + W * W everywhere and idx = -1: finite on purpose (scipy's distance_transform_edt
    returns arbitrary values there; it is the one input on which the two differ).  1 <= H, W <= 4096, M * H * W < 2^31."""
    if not torch.is_tensor(src) or src.dim() != 3:
        raise ValueError(f"distance_transform: expected a [M,H,W] tensor, got {list(getattr(src, 'shape', [])) or type(src)}")
    if src.dtype in (torch.uint8, torch.bool):
        if thresholds is not None:
            raise ValueError("distance_transform: thresholds belong to a float32 mask; a uint8 / bool source is non-zero where != 0")
        kind, channels, t_in, t_out = _lib.EDT_SRC_U8, 1, 0.0, 0.0
    elif src.dtype == torch.float32:
        if thresholds is None or len(thresholds) != 2:
            raise ValueError("distance_transform: a float32 mask needs thresholds=(t_in, t_out)")
        kind, channels, (t_in, t_out) = _lib.EDT_SRC_F32, 2, (float(t) for t in thresholds)
    else:
        raise ValueError(f"distance_transform: expected uint8, bool or float32, got {src.dtype}")
    n, h, w = (int(v) for v in src.shape)
    m = n * channels
    if n < 1 or not (1 <= h <= _lib.EDT_MAX_SIDE and 1 <= w <= _lib.EDT_MAX_SIDE) or m * h * w >= 1 << 31:
        raise ValueError(f"distance_transform: {list(src.shape)} is outside 1 <= H, W <= {_lib.EDT_MAX_SIDE}, M * H * W < 2^31")
    if not float(scale) > 0.0 or math.isinf(float(scale)):
        raise ValueError(f"distance_transform: scale must be positive and finite, got {scale}")
    require_device(src, what="distance_transform")
    src = src.detach().contiguous()
    if src.dtype == torch.bool:
        src = src.view(torch.uint8)
    shape = (n, 2, h, w) if channels == 2 else (n, h, w)
    scratch = torch.empty(_lib.lib().a3d_edt_scratch_bytes(m, h, w), dtype=torch.uint8, device=src.device)
    out = torch.empty(shape, dtype=torch.int32 if squared else torch.float32, device=src.device)
    idx = torch.empty(shape, dtype=torch.int32, device=src.device) if return_indices else None
    call("a3d_edt_fwd", ptr(src), kind, t_in, t_out, m, h, w, float(scale), ptr(scratch), None if squared else ptr(out), ptr(out) if squared else None,
         ptr(idx), stream())
    return (out, idx) if return_indices else out


# ---------------------------------------------------------------------------------------------- keypoint-transfer evaluation (include/a3d_eval.h)
def vertex_visibility(rast, tri, num_vertices):
    """rast [B,H,W,4] (channel 3: triangle id + 1, 0 = empty), tri [F,3] -> float32 [B, num_vertices]: 1 where the vertex is a corner of
    a triangle that owns at least one pixel of the image, else 0 (the reference's visualize_results.py:238-246 without its per-image
    mask compaction, sort and host synchronisation).  csrc/keypoints.hip: one thread per pixel, plain stores of 1, the same bits on
    every run.  No autograd node: the result never requires grad.  A raster buffer from rasterize(defer_resolve=True) is resolved
    first.  An id above F or a triangle corner outside [0, num_vertices) is skipped on the device and reported at the next host
    read-back of the path (_lib.defer_check)."""
    if not torch.is_tensor(rast) or rast.dim() != 4 or rast.shape[3] != 4 or not rast.is_floating_point():
        raise ValueError(f"vertex_visibility: expected a float rast [B,H,W,4], got {getattr(rast, 'dtype', type(rast))} {list(getattr(rast, 'shape', []))}")
    if not torch.is_tensor(tri) or tri.dtype not in (torch.int32, torch.int64) or not (tri.dim() == 2 or (tri.dim() == 3 and tri.shape[0] == 1)) or tri.shape[-1] != 3:
        raise ValueError(f"vertex_visibility: expected int32 / int64 triangles [F,3], got {getattr(tri, 'dtype', type(tri))} {list(getattr(tri, 'shape', []))}")
    B, H, W = (int(v) for v in rast.shape[:3])
    V, F = int(num_vertices), int(tri.shape[-2])
    if min(B, H, W, V, F) < 1 or B * H * W >= 1 << 31 or B * V >= 1 << 31:
        raise ValueError(f"vertex_visibility: rast {list(rast.shape)}, {F} triangles, {V} vertices: every count must be >= 1, B * H * W and B * V < 2^31")
    require_device(rast, tri, what="vertex_visibility")
    ensure_resolved(rast)
    rast = f32c(rast.detach())
    tri32 = tri_int32(tri)
    vis = torch.empty((B, V), dtype=torch.float32, device=rast.device)
    ok = torch.empty(1, dtype=torch.int32, device=rast.device)
    call("a3d_vertex_visibility_fwd", ptr(rast), ptr(tri32), B, H, W, F, V, ptr(vis), ptr(ok), stream())
    _lib.defer_check(ok[0], "vertex_visibility: a triangle id above F in rast, or a triangle corner outside [0, num_vertices) (skipped)")
    return vis


def nearest_visible_vertex(uv, visibility, keypoints):
    """uv [N,V,2], visibility [N,V] (0 = invisible), keypoints [N,K,2] in the same frame -> int64 [N,K]: per keypoint the index of the
    visible vertex with the smallest float32 d2 = dx * dx + dy * dy (dx = x - kp.x, dy = y - kp.y, each one operation, no FMA), an
    invisible vertex read as (+inf, +inf) like the reference's source_verts[visibility == 0] = np.inf (evaluate.py:464); the lowest
    index among equals, a NaN d2 below every number, 0 when nothing is visible: np.argmin's rules on the reference's matrix, without
    the [N,K,V] matrix.  csrc/keypoints.hip; the same bits on every run.  No autograd node: the result never requires grad."""
    for name, t, last in (("uv", uv, 2), ("visibility", visibility, None), ("keypoints", keypoints, 2)):
        if not torch.is_tensor(t) or not t.is_floating_point() or t.dim() != (2 if last is None else 3) or (last is not None and t.shape[2] != last):
            raise ValueError(f"nearest_visible_vertex: expected float {name} {'[N,V]' if last is None else '[N,*,2]'}, got "
                             f"{getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', []))}")
    N, V, K = int(uv.shape[0]), int(uv.shape[1]), int(keypoints.shape[1])
    if tuple(visibility.shape) != (N, V) or keypoints.shape[0] != N:
        raise ValueError(f"nearest_visible_vertex: uv {list(uv.shape)}, visibility {list(visibility.shape)} and keypoints {list(keypoints.shape)} do not belong together")
    if min(N, V, K) < 1 or V > 1 << 30 or N * V >= 1 << 31 or N * K >= 1 << 31:
        raise ValueError(f"nearest_visible_vertex: N = {N}, V = {V}, K = {K}: every count must be >= 1, V <= 2^30, N * V and N * K < 2^31")
    require_device(uv, visibility, keypoints, what="nearest_visible_vertex")
    uv, visibility, keypoints = f32c(uv.detach()), f32c(visibility.detach()), f32c(keypoints.detach())
    keys = torch.empty((N, K), dtype=torch.int64, device=uv.device)
    idx = torch.empty((N, K), dtype=torch.int32, device=uv.device)
    call("a3d_nearest_visible_vertex_fwd", ptr(uv), ptr(visibility), ptr(keypoints), N, V, K, ptr(keys), ptr(idx), stream())
    return idx.long()


# ---------------------------------------------------------------------------------------------- articulation glue (csrc/articulation.h)
def _dense_strides(t):
    """The strides of ``t`` when its elements are dense in some order and do not overlap (NCHW, a permuted NHWC view, ...), else None."""
    dims = sorted((d for d in range(t.dim()) if t.shape[d] > 1), key=t.stride)
    expect = 1
    for d in dims:
        if t.stride(d) != expect:
            return None
        expect *= t.shape[d]
    return tuple(max(int(s), 1) if t.shape[d] > 1 else expect for d, s in enumerate(t.stride()))


def _bone_inputs_launch(bones, mvp, w2c, feat, patch_feat, z_offset, spatial_scale):
    N, K = int(mvp.shape[0]), int(bones.shape[1])
    D = 0 if feat is None else int(feat.shape[1])
    C, h, w = (0, 1, 1) if patch_feat is None else (int(v) for v in patch_feat.shape[1:])
    bones, mvp, w2c = f32c(bones), f32c(mvp), f32c(w2c)
    feat = None if feat is None else f32c(feat)
    if patch_feat is not None and patch_feat.dtype != torch.float32:
        patch_feat = patch_feat.float()  # (keeps the strides of a dense tensor; never a .contiguous() copy of a float32 one)
    strides =(0, 0, 0, 0) if patch_feat is None else tuple(int(s) for s in patch_feat.stride())
    pos_in = torch.empty((N, K, 9), dtype=torch.float32, device=mvp.device)
    bones_feat = torch.empty((N, K, D + C), dtype=torch.float32, device=mvp.device) if D + C else None
    call("a3d_bone_inputs_fwd", ptr(bones), int(bones.shape[0] == 1 and N != 1), ptr(mvp), ptr(w2c), float(z_offset), float(spatial_scale), ptr(feat),
         ptr(patch_feat), *strides, N, K, D, C, h, w, ptr(bones_feat), ptr(pos_in), stream())
    return bones_feat, pos_in


class _BoneInputs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bones, mvp, w2c, feat, patch_feat, z_offset, spatial_scale):
        bones_feat, pos_in = _bone_inputs_launch(bones, mvp, w2c, feat, patch_feat, z_offset, spatial_scale)
        ctx.mark_non_differentiable(pos_in)
        ctx.save_for_backward(pos_in)
        ctx.D = 0 if feat is None else int(feat.shape[1])
        ctx.patch = None if patch_feat is None else (tuple(patch_feat.shape), _dense_strides(patch_feat))
        return bones_feat, pos_in

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, _g_pos):
        (pos_in,) = ctx.saved_tensors
        N, K, D = int(pos_in.shape[0]), int(pos_in.shape[1]), ctx.D
        want_feat = D > 0 and ctx.needs_input_grad[3]
        want_patch = ctx.patch is not None and ctx.needs_input_grad[4]
        if not (want_feat or want_patch):
            return (None,) * 7
        C, h, w = (0, 1, 1) if ctx.patch is None else ctx.patch[0][1:]
        g_feat = torch.empty((N, D), dtype=torch.float32, device=pos_in.device) if want_feat else None
        g_patch, gs = None, (0, 0, 0, 0)
        if want_patch:  # every element is written by the kernel: no zero-fill here
            shape, strides = ctx.patch
            g_patch = (torch.empty(shape, dtype=torch.float32, device=pos_in.device) if strides is None else
                       torch.empty_strided(shape, strides, dtype=torch.float32, device=pos_in.device))
            gs = tuple(max(int(s), 1) for s in g_patch.stride())
        call("a3d_bone_inputs_bwd", ptr(f32h(g_out)), ptr(pos_in), N, K, D, C, h, w, ptr(g_feat), ptr(g_patch), *gs, stream())
        return None, None, None, g_feat, g_patch, None, None


class _ConstrainAngles(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, S, multiplier, want_reg):
        x = f32c(x)
        N, K = int(x.shape[0]), int(x.shape[1])
        angles = torch.empty_like(x)
        reg = torch.empty((), dtype=torch.float32, device=x.device) if want_reg else None
        call("a3d_constrain_angles_fwd", ptr(x), ptr(S), float(multiplier), N, K, ptr(angles), ptr(reg), stream())
        ctx.save_for_backward(x, S)
        ctx.multiplier = float(multiplier)
        ctx.set_materialize_grads(False)
        return (angles, reg) if want_reg else angles

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_angles, g_reg=None):
        x, S = ctx.saved_tensors
        if g_angles is None and g_reg is None:
            return None, None, None, None
        g_x = torch.empty_like(x)
        call("a3d_constrain_angles_bwd", None if g_angles is None else ptr(f32h(g_angles)), None if g_reg is None else ptr(f32h(g_reg)), ptr(x), ptr(S),
             ctx.multiplier, int(x.shape[0]), int(x.shape[1]), ptr(g_x), stream())
        return g_x, None, None, None


def _float_tensor(t, dims, last, what):
    if not torch.is_tensor(t) or not t.is_floating_point() or t.dim() != dims or tuple(t.shape[dims - len(last):]) != tuple(last):
        raise ValueError(f"{what}, got {getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', []))}")


def bone_inputs_limits_ok(N, K, D, C, h, w):
    """Whether the descriptor kernels take these sizes (csrc/articulation.h)."""
    return (1 <= K <= _lib.ARTICULATION_MAX_BONES and 0 <= N <= _lib.ARTICULATION_MAX_IMAGES and
            (C == 0 or (1 <= h <= _lib.ARTICULATION_MAX_SIDE and 1 <= w <= _lib.ARTICULATION_MAX_SIDE)) and
            max(N * K * (D + C), N * K * 9, N * C * h * w) < 1 << 31)


def bone_inputs(bones, mvp, w2c, cam_pos_z_offset, spatial_scale, feat=None, patch_feat=None):
    """The per-bone descriptors of the articulation network (reference InstancePredictorBase.py:337-382): bones [N,K,2,3] or [1,K,2,3]
    (shared by the images), mvp and w2c [N,4,4], feat [N,D] or None, patch_feat [N,C,h,w] of any strides or None, all on the current
    device -> (bones_feat [N,K,D+C] or None when neither is given, bones_pos_in [N,K,9]).  One launch forward, one backward
    (csrc/articulation.hip), no memset, no atomics, the same bits on every run.  Gradients reach feat and patch_feat only;
    bones_pos_in never requires grad.  The gradient of patch_feat has its strides when it is dense in some order, else it is contiguous.
    A midpoint whose projected coordinate is not finite samples 0 and scatters nothing; a finite coordinate of any size is classified
    inside or outside the image in floating point.  Limits: 1 <= K <= 64, 1 <= h, w <= 4096, N <= 65535, every count below 2^31."""
    _float_tensor(bones, 4, (2, 3), "bone_inputs: expected float bones [N,K,2,3] or [1,K,2,3]")
    _float_tensor(mvp, 3, (4, 4), "bone_inputs: expected a float mvp [N,4,4]")
    _float_tensor(w2c, 3, (4, 4), "bone_inputs: expected a float w2c [N,4,4]")
    N, K = int(mvp.shape[0]), int(bones.shape[1])
    if w2c.shape[0] != N or bones.shape[0] not in (1, N):
        raise ValueError(f"bone_inputs: bones {list(bones.shape)}, mvp {list(mvp.shape)} and w2c {list(w2c.shape)} do not belong together")
    if feat is not None:
        _float_tensor(feat, 2, (), "bone_inputs: expected a float feat [N,D]")
    if patch_feat is not None:
        _float_tensor(patch_feat, 4, (), "bone_inputs: expected a float patch_feat [N,C,h,w]")
    if (feat is not None and feat.shape[0] != N) or (patch_feat is not None and patch_feat.shape[0] != N):
        raise ValueError(f"bone_inputs: feat / patch_feat do not have the {N} images of mvp")
    D = 0 if feat is None else int(feat.shape[1])
    C, h, w = (0, 1, 1) if patch_feat is None else (int(v) for v in patch_feat.shape[1:])
    if (feat is not None and D < 1) or (patch_feat is not None and min(C, h, w) < 1) or N < 1 or not bone_inputs_limits_ok(N, K, D, C, h, w):
        raise ValueError(f"bone_inputs: N = {N}, K = {K}, D = {D}, patch_feat [{C},{h},{w}] is outside 1 <= K <= {_lib.ARTICULATION_MAX_BONES}, "
                         f"1 <= h, w <= {_lib.ARTICULATION_MAX_SIDE}, 1 <= N <= {_lib.ARTICULATION_MAX_IMAGES}, every count below 2^31")
    if not (math.isfinite(float(cam_pos_z_offset)) and math.isfinite(float(spatial_scale)) and float(spatial_scale) != 0.0):
        raise ValueError(f"bone_inputs: cam_pos_z_offset {cam_pos_z_offset} / spatial_scale {spatial_scale} must be finite, the scale not 0")
    require_device(bones, mvp, w2c, feat, patch_feat, what="bone_inputs")
    bones, mvp, w2c = bones.detach(), mvp.detach(), w2c.detach()
    if D + C == 0:
        with torch.no_grad():
            return _bone_inputs_launch(bones.float(), mvp.float(), w2c.float(), None, None, cam_pos_z_offset, spatial_scale)
    return _BoneInputs.apply(bones, mvp, w2c, feat, patch_feat, float(cam_pos_z_offset), float(spatial_scale))


def constrain_angles(x, scale, multiplier, return_reg=False):
    """angles = scale[k,c] * tanh(multiplier * x) for x [N,K,3] and a float32 table scale [K,3], both on the current device, and with
    ``return_reg`` also reg = mean(angles^2) (a 0-dim float32 tensor: the reference's arti_reg_loss), differentiable through the same
    backward kernel.  One launch forward, one backward (csrc/articulation.hip: one work-group, double sums in a fixed order, the same
    bits on every run).  The backward recomputes tanh from x, so a zero of ``scale`` gives exactly 0 out and exactly 0 gradient, also
    at x = +-inf.  Limits: 1 <= K <= 64, N * K * 3 <= 2^20."""
    _float_tensor(x, 3, (3,), "constrain_angles: expected a float x [N,K,3]")
    N, K = int(x.shape[0]), int(x.shape[1])
    if not torch.is_tensor(scale) or scale.dtype != torch.float32 or tuple(scale.shape) != (K, 3):
        raise ValueError(f"constrain_angles: expected a float32 scale [{K},3], got {getattr(scale, 'dtype', type(scale))} {list(getattr(scale, 'shape', []))}")
    if N < 1 or not 1 <= K <= _lib.ARTICULATION_MAX_BONES or N * K * 3 > _lib.ARTICULATION_MAX_ANGLES:
        raise ValueError(f"constrain_angles: x {list(x.shape)} is outside N >= 1, 1 <= K <= {_lib.ARTICULATION_MAX_BONES}, N * K * 3 <= 2^20")
    if not math.isfinite(float(multiplier)):
        raise ValueError(f"constrain_angles: multiplier {multiplier} is not finite")
    require_device(x, scale, what="constrain_angles")
    return _ConstrainAngles.apply(x, scale.detach().contiguous(), float(multiplier), bool(return_reg))


# ---------------------------------------------------------------------------------------------- camera-pose glue (csrc/pose.h)
_POSE_TABLES = OrderedDict()  # (the values of a small host table, device) -> its float32 copy on that device


def pose_table(t, device):
    """orthant_signs / max_trans_xyz_range as a contiguous float32 tensor on ``device``: a tensor that is already there is taken as it
    is; a host table is copied once per distinct content and kept (these are a model's constants)."""
    if t.device == device:
        return f32c(t.detach())
    host = f32c(t.detach().cpu())
    key = (host.numpy().tobytes(), tuple(host.shape), str(device))
    if key not in _POSE_TABLES:
        if len(_POSE_TABLES) >= 32:
            _POSE_TABLES.popitem(last=False)
        _POSE_TABLES[key] = host.to(device)
    return _POSE_TABLES[key]


_POSE_PROJ = {}


def _proj_host(proj16):
    """The 16 floats of a projection as the host array the pose entry points read during the call (kept: a model has one or two)."""
    if proj16 not in _POSE_PROJ:
        if len(_POSE_PROJ) >= 32:
            _POSE_PROJ.clear()
        _POSE_PROJ[proj16] = (ctypes.c_float * 16)(*proj16)
    return _POSE_PROJ[proj16]


class _PoseCameras(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, signs, trans, rand_perm, best_perm, oct, zeroy, temp, naive_weight, best_below, offset_z, proj16):
        raw = f32c(raw)
        N, W = int(raw.shape[0]), int(raw.shape[1])
        H = (W - 3) // 4
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=raw.device)
        poses_raw, pose_raw, pose, mvp, w2c, campos = new(N, W), new(N, 6), new(N, 12), new(N, 4, 4), new(N, 4, 4), new(N, 3)
        rot_prob, rot_logit, rots_probs = new(N), new(N), new(N, H)
        rot_idx = torch.empty((N,), dtype=torch.int64, device=raw.device)
        rand_flag = torch.empty((N,), dtype=torch.int64, device=raw.device)
        common = (ptr(raw), ptr(signs), ptr(trans), ptr(rand_perm), ptr(best_perm), N, H, int(oct), int(zeroy), float(temp), float(naive_weight),
                  float(1 - naive_weight), int(best_below), float(offset_z), _proj_host(proj16))
        call("a3d_pose_cameras_fwd", *common, ptr(poses_raw), ptr(pose_raw), ptr(pose), ptr(mvp), ptr(w2c), ptr(campos), ptr(rot_idx),
             ptr(rot_prob), ptr(rot_logit), ptr(rots_probs), ptr(rand_flag), stream())
        ctx.save_for_backward(raw, signs, trans, rand_perm, best_perm)
        ctx.common = common[5:]
        ctx.mark_non_differentiable(rot_idx, rand_flag)
        ctx.set_materialize_grads(False)
        return poses_raw, pose_raw, pose, mvp, w2c, campos, rot_idx, rot_prob, rot_logit, rots_probs, rand_flag

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_poses_raw, g_pose_raw, g_pose, g_mvp, g_w2c, g_campos, _g_idx, g_rot_prob, g_rot_logit, g_rots_probs, _g_flag):
        grads = (g_poses_raw, g_pose_raw, g_pose, g_mvp, g_w2c, g_campos, g_rot_prob, g_rot_logit, g_rots_probs)
        if not ctx.needs_input_grad[0] or all(g is None for g in grads):
            return (None,) * 12
        raw, signs, trans, rand_perm, best_perm = ctx.saved_tensors
        g_raw = torch.empty_like(raw)
        call("a3d_pose_cameras_bwd", ptr(raw), ptr(signs), ptr(trans), ptr(rand_perm), ptr(best_perm), *ctx.common,
             *(None if g is None else ptr(f32h(g)) for g in grads), ptr(g_raw), stream())
        return (g_raw,) + (None,) * 11


class _CamerasFromPose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pose, offset_z, proj16):
        pose = f32c(pose)
        N = int(pose.shape[0])
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=pose.device)
        mvp, w2c, campos = new(N, 4, 4), new(N, 4, 4), new(N, 3)
        call("a3d_cameras_from_pose_fwd", ptr(pose), N, float(offset_z), _proj_host(proj16), ptr(mvp), ptr(w2c), ptr(campos), stream())
        ctx.save_for_backward(pose)
        ctx.consts = (float(offset_z), proj16)
        ctx.set_materialize_grads(False)
        return mvp, w2c, campos

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mvp, g_w2c, g_campos):
        if g_mvp is None and g_w2c is None and g_campos is None:
            return None, None, None
        (pose,) = ctx.saved_tensors
        g_pose = torch.empty_like(pose)
        call("a3d_cameras_from_pose_bwd", ptr(pose), int(pose.shape[0]), ctx.consts[0], _proj_host(ctx.consts[1]),
             *(None if g is None else ptr(f32h(g)) for g in (g_mvp, g_w2c, g_campos)), ptr(g_pose), stream())
        return g_pose, None, None


def _pose_proj(proj16, who):
    proj16 = tuple(float(v) for v in proj16)
    if len(proj16) != 16 or not all(math.isfinite(v) for v in proj16):
        raise ValueError(f"{who}: expected the 16 finite numbers of a row-major projection")
    return proj16


def predict_cameras(raw, orthant_signs, max_trans, rand_perm, best_perm, oct, zeroy, temp, naive_weight, best_below, offset_z, proj16):
    """Heads, pick and cameras of the pose path in one launch (reference InstancePredictorBase.py:257-304, 623-663, 606-620): raw
    [N,4H+3], orthant_signs [H,3] and max_trans [3] float32, rand_perm / best_perm [N] int64 or both None, all on the current device;
    temp, naive_weight in [0,1], best_below (image n keeps its best hypothesis where best_perm[n] < best_below), offset_z (added to the
    translation's z) and the 16 numbers of the projection on the host -> (poses_raw, pose_raw, pose, mvp, w2c, campos, rot_idx,
    rot_prob, rot_logit, rots_probs, rand_pose_flag).  One launch backward (csrc/pose.hip), which takes the gradients of all nine float
    outputs and returns the gradient of raw; no memset, no atomics, the same bits on every run.  Limits: 1 <= H <= 8, 1 <= N <= 65535."""
    _float_tensor(raw, 2, (), "predict_cameras: expected a float raw [N,4H+3]")
    N, W = int(raw.shape[0]), int(raw.shape[1])
    H = (W - 3) // 4
    if W != 4 * H + 3 or not 1 <= H <= _lib.POSE_MAX_HYPOS or not 1 <= N <= _lib.POSE_MAX_IMAGES:
        raise ValueError(f"predict_cameras: raw {list(raw.shape)} is outside [N,4H+3] with 1 <= H <= {_lib.POSE_MAX_HYPOS}, 1 <= N <= {_lib.POSE_MAX_IMAGES}")
    for t, shape, name in ((orthant_signs, (H, 3), "orthant_signs"), (max_trans, (3,), "max_trans")):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"predict_cameras: expected a contiguous float32 {name} {list(shape)}, got {getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', []))}")
    if (rand_perm is None) != (best_perm is None):
        raise ValueError("predict_cameras: rand_perm and best_perm are given together or not at all")
    for t, name in ((rand_perm, "rand_perm"), (best_perm, "best_perm")):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != (N,)):
            raise ValueError(f"predict_cameras: expected an int64 {name} [{N}], got {getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', []))}")
    if not (math.isfinite(float(temp)) and float(temp) > 0 and 0.0 <= float(naive_weight) <= 1.0 and math.isfinite(float(offset_z))) \
            or not 0 <= int(best_below) <= N:
        raise ValueError(f"predict_cameras: temp {temp}, naive_weight {naive_weight}, best_below {best_below}, offset_z {offset_z}: expected "
                         f"temp > 0, 0 <= naive_weight <= 1, 0 <= best_below <= {N}, a finite offset")
    proj16 = _pose_proj(proj16, "predict_cameras")
    require_device(raw, orthant_signs, max_trans, rand_perm, best_perm, what="predict_cameras")
    if rand_perm is not None:
        rand_perm, best_perm = rand_perm.contiguous(), best_perm.contiguous()
    return _PoseCameras.apply(raw, orthant_signs.detach(), max_trans.detach(), rand_perm, best_perm, bool(oct), bool(zeroy), float(temp),
                              float(naive_weight), int(best_below), float(offset_z), proj16)


def cameras_from_pose(pose, offset_z, proj16):
    """pose [N,12] (a row-major 3x3 R, then t) on the current device -> (mvp, w2c [N,4,4], campos [N,3]): w2c = [[R^T, t + (0, 0,
    offset_z)], [0,0,0,1]], mvp = proj @ w2c, campos = -R (t + (0, 0, offset_z)) (reference InstancePredictorBase.py:606-620).  One
    launch forward, one backward (csrc/pose.hip); the gradient goes to pose.  Limit: 1 <= N <= 65535."""
    _float_tensor(pose, 2, (12,), "cameras_from_pose: expected a float pose [N,12]")
    if not 1 <= int(pose.shape[0]) <= _lib.POSE_MAX_IMAGES or not math.isfinite(float(offset_z)):
        raise ValueError(f"cameras_from_pose: pose {list(pose.shape)} / offset_z {offset_z} is outside 1 <= N <= {_lib.POSE_MAX_IMAGES}, a finite offset")
    proj16 = _pose_proj(proj16, "cameras_from_pose")
    require_device(pose, what="cameras_from_pose")
    return _CamerasFromPose.apply(pose, float(offset_z), proj16)


def random_view_cameras(w2c_pred, rand_degree, delta_angle, proj16):
    """Fauna's random-view cameras (reference Fauna.py:112-142) for the first b = len(rand_degree) images of w2c_pred [>= b,4,4] on the
    current device; rand_degree an integer tensor on any device (copied over without a synchronisation when it is on the host), the
    float32 delta_angle = 2 pi / bins and the projection on the host -> (mvp, w2c [b,4,4], campos [b,3]), none requiring grad.  One
    launch (csrc/pose.hip).  Limit: 1 <= b <= 65535."""
    _float_tensor(w2c_pred, 3, (4, 4), "random_view_cameras: expected a float w2c_pred [N,4,4]")
    if not torch.is_tensor(rand_degree) or rand_degree.is_floating_point() or rand_degree.dim() != 1 \
            or not 1 <= int(rand_degree.shape[0]) <= min(int(w2c_pred.shape[0]), _lib.POSE_MAX_IMAGES):
        raise ValueError(f"random_view_cameras: expected an integer rand_degree [b], 1 <= b <= min({w2c_pred.shape[0]}, {_lib.POSE_MAX_IMAGES}), got "
                         f"{getattr(rand_degree, 'dtype', type(rand_degree))} {list(getattr(rand_degree, 'shape', []))}")
    if not math.isfinite(float(delta_angle)):
        raise ValueError(f"random_view_cameras: delta_angle {delta_angle} is not finite")
    proj16 = _pose_proj(proj16, "random_view_cameras")
    require_device(w2c_pred, what="random_view_cameras")
    b = int(rand_degree.shape[0])
    w2c_pred = f32c(w2c_pred.detach())
    degree = rand_degree.detach().to(device=w2c_pred.device, dtype=torch.int64, non_blocking=True).contiguous()
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=w2c_pred.device)
    mvp, w2c, campos = new(b, 4, 4), new(b, 4, 4), new(b, 3)
    call("a3d_random_view_cameras", ptr(w2c_pred), ptr(degree), b, float(delta_angle), _proj_host(proj16), ptr(mvp), ptr(w2c), ptr(campos), stream())
    return mvp, w2c, campos


# ---------------------------------------------------------------------------------------------- mixed precision
def _amp_wrap_functions():
    """Every autograd.Function of this module runs its forward with autocast OFF on float32 copies of half-precision inputs, and its
    backward in the same state (torch.amp.custom_fwd / custom_bwd): the kernels are float32, so are their outputs and the gradients
    they return -- autograd casts a gradient back to the dtype of a bf16 / fp16 input.  What the reference does by hand with .float()
    at the nvdiffrast boundary (render.py:265,292) under Trainer.py:208-218's autocast."""
    from torch.amp import custom_bwd, custom_fwd

    for obj in list(globals().values()):
        if isinstance(obj, type) and issubclass(obj, torch.autograd.Function) and obj is not torch.autograd.Function and obj.__module__ == __name__:
            obj.forward = staticmethod(custom_fwd(obj.forward, device_type="cuda", cast_inputs=torch.float32))
            obj.backward = staticmethod(custom_bwd(obj.backward, device_type="cuda"))


_amp_wrap_functions()

if _lib.GUARD:  # A3D_GUARD in the environment: guarded allocations from the first call on (see _lib.set_guard)
    _lib.set_guard(_lib.GUARD)
