"""Keypoint-transfer evaluation on the GPU (csrc/keypoints.hip through ops.vertex_visibility, ops.nearest_visible_vertex and
3danimals_amd/evaluation.py) against the restatement of tests/keypoints_ref.py and what was recorded of the reference
(tests/golden/keypoints.npz).  Visibilities and indices are compared with torch.equal; the float64 pair stage within 1e-12 relative.

The whole file runs under guard level 2 (_lib.set_guard: canaries around, and poison inside, every buffer the ops allocate); the one
test that forbids host synchronisation switches it off for its forbidden region, since the guard's own check synchronises."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden, kuhn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoints_cases as C  # noqa: E402
import keypoints_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _ops():
    return importlib.import_module("3danimals_amd.ops")


def _L():
    return importlib.import_module("3danimals_amd._lib")


def _E():
    return importlib.import_module("3danimals_amd.evaluation")


@pytest.fixture(scope="module", autouse=True)
def guard_level_2():
    L = _L()
    _ops()
    L.poll_deferred()
    prev = L.set_guard(2)
    yield
    L.set_guard(prev)


@pytest.fixture(scope="module")
def G():
    return golden("keypoints.npz")


# ------------------------------------------------------------------------------------------------ visibility
def grid_mesh(V):
    """(clip [2,V,4], tri [F,3] int32): a triangulated n x n grid of vertices plus one vertex no triangle refers to (V = n * n + 1), or
    one triangle (V = 3).  Image 0 shows the grid pushed to the right, a part of it off screen; image 1 shows it folded along x = 0,
    the right half in front of the left one -- another subset of the vertices."""
    if V == 3:
        xy = torch.tensor([[[-0.8, -0.7], [0.9, -0.6], [0.1, 0.8]], [[-0.8, -0.7], [0.9, -0.6], [0.1, 0.8]]])
        xy[1, :, 0] += 3.0  # image 1: off screen
        clip = torch.cat([xy, torch.zeros(2, 3, 1), torch.ones(2, 3, 1)], -1)
        return clip, torch.tensor([[0, 1, 2]], dtype=torch.int32)
    n = int(round((V - 1) ** 0.5))
    assert n * n + 1 == V
    t = torch.linspace(-0.9, 0.9, n)
    y, x = torch.meshgrid(t, t, indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)
    g = torch.Generator().manual_seed(V)
    z = 0.1 * torch.rand(n * n, generator=g)
    img0 = torch.stack([x + 0.8, y, z, torch.ones_like(x)], -1)
    img1 = torch.stack([x.abs() * 0.9 - 0.05, y * 0.7, z + 0.3 * (x < 0), torch.ones_like(x)], -1)
    clip = torch.stack([img0, img1])
    clip = torch.cat([clip, torch.tensor([[[0.0, 0.0, -0.5, 1.0]]]).expand(2, 1, 4)], 1)  # the unreferenced vertex, in front of everything
    i = torch.arange(n - 1)
    a = (i[:, None] * n + i[None, :]).reshape(-1)
    tri = torch.cat([torch.stack([a, a + 1, a + n], -1), torch.stack([a + 1, a + n + 1, a + n], -1)]).to(torch.int32)
    return clip, tri


@pytest.mark.parametrize("resolution", ((33, 70), (64, 64)))
@pytest.mark.parametrize("V", (3, 65, 257))
def test_visibility_equals_the_restatement_on_the_gpus_own_raster(V, resolution):
    ops = _ops()
    clip, tri = grid_mesh(V)
    clip, tri = clip.cuda(), tri.cuda()
    rast = ops.rasterize(clip, tri, resolution)
    vis = ops.vertex_visibility(rast, tri, V)
    assert vis.shape == (2, V) and vis.dtype == torch.float32 and not vis.requires_grad
    want = torch.from_numpy(R.visibility(rast.cpu().numpy(), tri.cpu().numpy(), V))
    print(f"V={V} {resolution}: visible per image {vis.sum(1).tolist()}, {int((vis.cpu() != want).sum())} differ")
    assert torch.equal(vis.cpu(), want)
    assert float(want[0].sum()) >= 3 and not torch.equal(want[0], want[1])  # image 1 shows another subset
    if V > 3:
        assert 0 < float(want[1].sum()) < V - 1 and float(want[0].sum()) < V - 1 and want[0, -1] == 0 and want[1, -1] == 0
    else:
        assert float(want[1].sum()) == 0  # nothing leaks from image 0
    again = ops.vertex_visibility(rast, tri.long(), V)  # int64 triangles; two runs give equal bits
    assert torch.equal(again, vis)


@pytest.fixture(scope="module")
def sphere():
    """A Kuhn-8 DMTet sphere (542 vertices), posed under two cameras."""
    ops = _ops()
    pkg = importlib.import_module("3danimals_amd")
    T = importlib.import_module("3danimals_amd.model.geometry.dmtet").TetGridTopology
    pos, tets = kuhn(8, scale=5.0)
    sdf = 1.9 - pos.norm(dim=-1)  # 542 surface vertices
    topo = T(tets.cuda(), positions=pos.cuda())
    verts, faces, _, _ = ops.dmtet_extract(pos.cuda(), sdf.cuda(), topo)
    mvp, _, _ = pkg.synthetic.random_cameras(2, seed=3)
    v_pos = verts[None].repeat(2, 1, 1).contiguous()
    v_pos[1, :, 0] += 0.4
    return v_pos, faces, mvp.cuda()


def test_project_and_occlude_on_a_posed_dmtet_sphere(sphere):
    ops, E, L = _ops(), _E(), _L()
    v_pos, faces, mvp = sphere
    V = v_pos.shape[1]
    print(f"sphere: {V} vertices, {faces.shape[0]} triangles")
    assert V == 542 and faces.shape[0] > V
    uv, vis = E.project_and_occlude(v_pos, faces, mvp, (64, 64))  # (under the guard: every call is followed by a canary check)
    clip = ops.xfm_points(v_pos, mvp)
    assert uv.shape == (2, V, 2) and torch.equal(uv, clip[..., :2] / clip[..., 3:]) and not uv.requires_grad and not vis.requires_grad
    rast = ops.rasterize(clip, faces, (64, 64))
    want = torch.from_numpy(R.visibility(rast.cpu().numpy(), faces.cpu().numpy(), V))
    assert torch.equal(vis.cpu(), want)
    share = want.mean(1)
    print(f"visible share per image {share.tolist()}")
    assert 0.15 < float(share.min()) and float(share.max()) < 0.8 and not torch.equal(want[0], want[1])  # a sphere shows about half of itself
    # 33 x 70: no covered-pixel list, odd rows
    uv2, vis2 = E.project_and_occlude(v_pos, faces, mvp, (33, 70))
    rast2 = ops.rasterize(clip, faces, (33, 70))
    assert torch.equal(uv2, uv) and torch.equal(vis2.cpu(), torch.from_numpy(R.visibility(rast2.cpu().numpy(), faces.cpu().numpy(), V)))
    # ... and it synchronises nowhere (the guard's check does: off for this region)
    L.set_guard(0)
    try:
        E.project_and_occlude(v_pos, faces, mvp, (64, 64))  # (every kernel loaded, every cache warm)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            uv3, vis3 = E.project_and_occlude(v_pos, faces, mvp, (64, 64))
        finally:
            torch.cuda.set_sync_debug_mode("default")
    finally:
        L.set_guard(2)
    assert torch.equal(uv3, uv) and torch.equal(vis3, vis)
    L.poll_deferred()  # nothing was skipped on the device


def _occlusion_scene():
    """Triangle 0 in front covers triangle 1 entirely; they share vertex 0.  Triangle 2 is off screen, vertex 8 belongs to nothing."""
    xy = torch.tensor([[-0.9, -0.9], [0.9, -0.9], [0.0, 0.9], [0.1, -0.5], [-0.1, 0.2], [3.0, 3.0], [3.5, 3.0], [3.0, 3.5], [0.0, 0.0]])
    z = torch.tensor([0.0, 0.0, 0.0, 0.5, 0.5, 0.0, 0.0, 0.0, -0.9])
    clip = torch.cat([xy, z[:, None], torch.ones(9, 1)], -1)[None]
    tri = torch.tensor([[0, 1, 2], [0, 3, 4], [5, 6, 7]], dtype=torch.int32)
    return clip.cuda(), tri.cuda()


def test_known_answers_without_the_restatement():
    ops = _ops()
    clip, tri = _occlusion_scene()
    rast = ops.rasterize(clip, tri, (64, 64))
    ids = rast[..., 3]
    assert set(ids.unique().tolist()) == {0.0, 1.0}  # the back triangle owns no pixel
    vis = ops.vertex_visibility(rast, tri, 9)
    assert vis.tolist() == [[1, 1, 1, 0, 0, 0, 0, 0, 0]]  # the shared vertex reads 1, the back triangle's own ones 0, so does the unreferenced one
    # the LAST triangle (id = F) alone on screen
    last = torch.tensor([[5, 6, 7], [5, 6, 7], [0, 1, 2]], dtype=torch.int32).cuda()
    rast = ops.rasterize(clip, last, (64, 64))
    assert set(rast[..., 3].unique().tolist()) == {0.0, 3.0}
    assert ops.vertex_visibility(rast, last, 9).tolist() == [[1, 1, 1, 0, 0, 0, 0, 0, 0]]
    # a triangle that owns exactly one pixel: around the centre of pixel (32, 32) of 64 x 64, and of the last pixel (63, 63)
    for px in (32, 63):
        c = (px + 0.5) / 32 - 1
        one = torch.tensor([[c - 0.01, c - 0.01, 0, 1], [c + 0.01, c - 0.01, 0, 1], [c, c + 0.01, 0, 1], [0.5, 0.5, 0, 1]])[None].cuda()
        rast = ops.rasterize(one, tri[:1], (64, 64))
        assert int((rast[..., 3] > 0).sum()) == 1
        assert ops.vertex_visibility(rast, tri[:1], 4).tolist() == [[1, 1, 1, 0]]
    # nothing on screen
    rast = ops.rasterize(clip + torch.tensor([5.0, 0, 0, 0]).cuda(), tri, (33, 70))
    assert int((rast[..., 3] > 0).sum()) == 0
    vis = ops.vertex_visibility(rast, tri, 9)
    assert vis.shape == (1, 9) and bool((vis == 0).all())
    _L().poll_deferred()


def test_a_deferred_resolve_raster_is_resolved_first(sphere):
    ops = _ops()
    v_pos, faces, mvp = sphere
    clip = ops.xfm_points(v_pos, mvp)
    want = ops.vertex_visibility(ops.rasterize(clip, faces, (64, 64)), faces, v_pos.shape[1])
    rast = ops.rasterize(clip, faces, (64, 64), defer_resolve=True)
    got = ops.vertex_visibility(rast, faces, v_pos.shape[1])
    assert torch.equal(got, want) and float(got.sum()) > 0
    assert ops._pending_resolve.peek(rast) is None
    # a raster buffer handed over in float16 (whole numbers up to 2048 are exact there) is read as its float32 values
    assert faces.shape[0] < 2048
    assert torch.equal(ops.vertex_visibility(ops.rasterize(clip, faces, (64, 64)).half(), faces, v_pos.shape[1]), want)


def test_data_that_is_out_of_range_is_skipped_and_reported_at_the_next_read_back():
    ops, L = _ops(), _L()
    L.poll_deferred()
    clip, tri = _occlusion_scene()
    rast = ops.rasterize(clip, tri, (64, 64))
    # a corner outside [0, V): only triangle 0 is on screen, and it refers to vertex 2
    vis = ops.vertex_visibility(rast, tri, 2)
    assert vis.tolist() == [[0, 0]]  # the pixel is skipped as a whole
    with pytest.raises(L.A3DError, match="vertex_visibility"):
        L.poll_deferred()
    # an id above F: the raster buffer shows triangle 3 of a list that is handed over with two rows
    last = torch.tensor([[5, 6, 7], [5, 6, 7], [0, 1, 2]], dtype=torch.int32).cuda()
    rast = ops.rasterize(clip, last, (64, 64))
    vis = ops.vertex_visibility(rast, last[:2].contiguous(), 9)
    assert bool((vis == 0).all())
    with pytest.raises(L.A3DError, match="vertex_visibility"):
        L.read_back(vis.sum())
    # ids that are no whole numbers, negative or NaN
    bad = torch.zeros(1, 8, 8, 4, device="cuda")
    bad[0, 0, 0, 3], bad[0, 1, 1, 3], bad[0, 2, 2, 3], bad[0, 3, 3, 3] = 1.5, -1.0, float("nan"), 1.0
    vis = ops.vertex_visibility(bad, tri, 9)
    assert vis.tolist() == [[1, 1, 1, 0, 0, 0, 0, 0, 0]]
    with pytest.raises(L.A3DError, match="vertex_visibility"):
        L.poll_deferred()
    ops.vertex_visibility(torch.zeros(1, 8, 8, 4, device="cuda"), tri, 9)
    L.poll_deferred()  # clean data: nothing to report


# ------------------------------------------------------------------------------------------------ nearest visible vertex
@pytest.mark.parametrize("name", C.ALL)
def test_nearest_visible_vertex_equals_the_restatement_and_the_reference(name, G):
    ops, L = _ops(), _L()
    case = C.make_case(name)
    n, v = case["uv"].shape[:2]
    assert L.lib().a3d_nearest_visible_vertex_slab(n, v) == C.SLAB  # V = 5000: twenty work-groups of 256 vertices per image
    uv, vis, kp = (torch.from_numpy(case[k]).cuda() for k in ("uv", "vis", "kp"))
    got = ops.nearest_visible_vertex(uv, vis, kp)
    assert got.dtype == torch.int64 and got.shape == kp.shape[:2] and not got.requires_grad
    want = R.nearest_visible_vertex(case["uv"], case["vis"], case["kp"])
    print(f"{name}: {int((got.cpu().numpy() != want).sum())} of {want.size} indices differ from the float32 restatement")
    assert np.array_equal(got.cpu().numpy(), want)
    if name in C.FINITE:
        assert np.array_equal(got.cpu().numpy(), G[f"{name}_idx"])
    assert torch.equal(ops.nearest_visible_vertex(uv, vis, kp), got)  # two runs give equal bits


@pytest.mark.parametrize("name", list(C.TRIPS))
def test_slabs_of_several_trips_per_thread_equal_the_restatement(name):
    """N * V large enough for slabs of 2, 5 and the most (32) trips of 256 vertices: the loop over a thread's own vertices."""
    ops, L = _ops(), _L()
    case = C.make_trips_case(name)
    n, v, k, trips = C.TRIPS[name]
    assert L.lib().a3d_nearest_visible_vertex_slab(n, v) == 256 * trips
    got = ops.nearest_visible_vertex(*(torch.from_numpy(case[key]).cuda() for key in ("uv", "vis", "kp"))).cpu().numpy()
    want = R.nearest_visible_vertex(case["uv"], case["vis"], case["kp"])
    print(f"{name}: {int((got != want).sum())} of {want.size} indices differ from the float32 restatement")
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], 5 + np.arange(k)) and got[1, 0] <= min(256 * trips, v) - 1


def test_nearest_visible_vertex_named_answers():
    ops = _ops()

    def run(name):
        case = C.make_case(name)
        return case, ops.nearest_visible_vertex(*(torch.from_numpy(case[k]).cuda() for k in ("uv", "vis", "kp"))).cpu().numpy()

    j = np.arange(16)
    _, got = run("duplicates_across_slabs")
    assert np.array_equal(got[0], 10 + j) and np.array_equal(got[1], 300 + 3 * j) and np.array_equal(got[2], 10 + j + (1 + j) * C.SLAB)
    assert (run("only_last_visible")[1] == 4999).all()
    _, got = run("none_visible")
    assert (got[[0, 2]] == 0).all() and (got[1] == 4000).all()
    case, got = run("invisible_is_nearest")
    assert (got != 7 + 300 * j).all() and (np.take_along_axis(case["vis"], got, 1) == 1).all()
    case, got = run("nan_keypoint")
    assert got[0, 3] == 0 and got[1, 5] == 0 and (got[2] == 0).all() and case["vis"][0, 0] == 0
    _, got = run("nan_vertex")
    assert (got[0] == 4321).all() and (got[1] != 100).all() and (got[2] == 255).all()
    _, got = run("inf_coordinates")
    assert (got[0] != 17).all() and (got[0] != 18).all() and got[1, 2] == 0 and got[2, 4] == 2000


def test_half_precision_inputs_are_read_as_their_float32_values():
    ops = _ops()
    case = C.make_case("coarse_V257_K17")  # (multiples of 2^-3 up to 2: exact in bfloat16)
    uv, vis, kp = (torch.from_numpy(case[k]).cuda() for k in ("uv", "vis", "kp"))
    want = ops.nearest_visible_vertex(uv, vis, kp)
    assert torch.equal(ops.nearest_visible_vertex(uv.bfloat16(), vis.half(), kp.bfloat16()), want)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert torch.equal(ops.nearest_visible_vertex(uv, vis, kp), want)
    # views that are not contiguous
    wide = torch.cat([uv, uv + 1], -1)
    assert torch.equal(ops.nearest_visible_vertex(wide[..., :2], vis, kp), want)


# ------------------------------------------------------------------------------------------------ the pair stage
def test_keypoint_transfer_pck_equals_the_reference(G):
    E = _E()
    c = {k: torch.from_numpy(v).cuda() for k, v in C.make_pck_case().items()}
    assert c["uv"].shape[0] == 6 and c["pairs"].shape == (40, 2) and bool((c["pairs"][:, 0] == c["pairs"][:, 1]).any())
    for pad, tag in ((0, ""), (C.PCK_PAD, "_pad")):
        pck, err, visible, vert_idx = E.keypoint_transfer_pck(c["uv"], c["vis"], c["kp"], c["kp_visible"], c["boxes"], c["pairs"], box_pad_frac=pad)
        assert err.is_cuda and err.dtype == torch.float64 and err.shape == visible.shape == (40, 16) and vert_idx.dtype == torch.int64
        assert np.array_equal(vert_idx.cpu().numpy(), G["pck_vert_idx"])
        rel = float((np.abs(err.cpu().numpy() - G[f"pck{tag}_err"]) / G[f"pck{tag}_err"].clip(1e-300)).max())
        print(f"pad {pad}: pck {pck!r} (reference {float(G[f'pck{tag}_value'])!r}), largest relative error of kps_err {rel:.3e}")
        np.testing.assert_allclose(err.cpu().numpy(), G[f"pck{tag}_err"], rtol=1e-12, atol=0)
        assert np.array_equal(visible.cpu().numpy(), G["pck_visible"]) and np.array_equal(visible.sum(0).cpu().numpy(), G["pck_count"])
        if not tag:
            assert np.array_equal(((err < 0.1) * visible).sum(0).cpu().numpy(), G["pck_correct"])
        assert isinstance(pck, float) and pck == float(G[f"pck{tag}_value"])
    # transfer_keypoints, single and batched, on the device; its arguments stay as they were
    keep = c["uv"].clone()
    s, t = c["pairs"][:, 0], c["pairs"][:, 1]
    pred, aux = E.transfer_keypoints(c["uv"][s], c["vis"][s], c["uv"][t], c["kp"][s])
    assert pred.shape == (40, 16, 2) and np.array_equal(aux["vert_idx"].cpu().numpy(), G["pck_vert_idx"][s.cpu().numpy()])
    one, aux1 = E.transfer_keypoints(c["uv"][0], c["vis"][0], c["uv"][5], c["kp"][0])
    assert torch.equal(one, pred[1]) and torch.equal(aux1["vert_idx"], aux["vert_idx"][1]) and torch.equal(c["uv"], keep)


# ------------------------------------------------------------------------------------------------ the ABI
def test_refusals_through_the_abi_leave_the_outputs_untouched():
    L = _L()
    lib = L.lib()
    B, H, W, F, V = 1, 8, 8, 2, 5
    rast = torch.zeros(B, H, W, 4, device="cuda")
    rast[0, 2, 3, 3] = 2.0
    tri = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32, device="cuda")
    vis = torch.full((B, V), -7.0, device="cuda")
    ok = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    good = dict(rast=rast.data_ptr(), tri=tri.data_ptr(), B=B, H=H, W=W, F=F, V=V, vis=vis.data_ptr(), ok=ok.data_ptr())
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(F=0), dict(V=0), dict(rast=None), dict(tri=None), dict(vis=None), dict(ok=None)):
        assert lib.a3d_vertex_visibility_fwd(*dict(good, **bad).values(), L.stream()) == -1, bad
        msg = lib.a3d_last_error().decode()
        assert "a3d_vertex_visibility_fwd" in msg and "invalid argument" in msg, (bad, msg)
    torch.cuda.synchronize()
    assert bool((vis == -7.0).all()) and int(ok) == -7
    assert lib.a3d_vertex_visibility_fwd(*good.values(), L.stream()) == 0
    torch.cuda.synchronize()
    assert vis.tolist() == [[0, 0, 1, 1, 1]] and int(ok) == 1

    N, Vn, K = 2, 70, 3
    uv = torch.rand(N, Vn, 2, device="cuda")
    seen = torch.ones(N, Vn, device="cuda")
    kp = uv[:, [5, 69, 0]].contiguous()
    keys = torch.full((N, K), -7, dtype=torch.int64, device="cuda")
    idx = torch.full((N, K), -7, dtype=torch.int32, device="cuda")
    assert lib.a3d_nearest_visible_vertex_scratch_bytes(N, K) == keys.numel() * 8
    good = dict(uv=uv.data_ptr(), vis=seen.data_ptr(), kp=kp.data_ptr(), N=N, V=Vn, K=K, keys=keys.data_ptr(), idx=idx.data_ptr())
    for bad in (dict(N=0), dict(V=0), dict(K=-2), dict(uv=None), dict(vis=None), dict(kp=None), dict(keys=None), dict(idx=None), dict(uv=uv.data_ptr() + 4)):
        assert lib.a3d_nearest_visible_vertex_fwd(*dict(good, **bad).values(), L.stream()) == -1, bad
        msg = lib.a3d_last_error().decode()
        assert "a3d_nearest_visible_vertex_fwd" in msg and "invalid argument" in msg, (bad, msg)
    torch.cuda.synchronize()
    assert bool((keys == -7).all()) and bool((idx == -7).all())
    assert lib.a3d_nearest_visible_vertex_fwd(*good.values(), L.stream()) == 0
    torch.cuda.synchronize()
    assert idx.tolist() == [[5, 69, 0], [5, 69, 0]]
    with pytest.raises(L.A3DError, match="a3d_nearest_visible_vertex_fwd"):
        L.call("a3d_nearest_visible_vertex_fwd", *dict(good, K=0).values(), L.stream())


def test_this_file_ran_under_guard_level_2_without_a_canary_touched():
    ops, L = _ops(), _L()
    assert L.GUARD == 2 and isinstance(ops.torch, L.GuardedTorch)
    before = dict(L.guard_stats)
    case = C.make_case("lattice_V5000_K17")
    uv, vis, kp = (torch.from_numpy(case[k]).cuda() for k in ("uv", "vis", "kp"))
    ops.nearest_visible_vertex(uv, vis, kp)
    clip, tri = grid_mesh(257)
    ops.vertex_visibility(ops.rasterize(clip.cuda(), tri.cuda(), (33, 70)), tri.cuda(), 257)
    # vis + ok, keys + idx, and what rasterize allocates: all guarded, all checked after every entry point
    assert L.guard_stats["allocations"] - before["allocations"] >= 5 and L.guard_stats["checks"] - before["checks"] >= 3
    assert L.guard_stats["buffers_checked"] > before["buffers_checked"]
    L.guard_check("the end of tests/test_keypoints_gpu.py")
