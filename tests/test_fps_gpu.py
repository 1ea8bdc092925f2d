"""Farthest-point sampling on the GPU (csrc/fps.hip) through ops.farthest_point_sample, util.sample_farthest_points and
skinning.estimate_bones(resample=True), against the float64 greedy reference of tests/fps_ref.py (itself held to a golden of the
reference project by tests/test_fps_cpu.py).  Inputs: tests/fps_cases.py.  References are computed once per cloud and shared.

Two forms of check (assert_picks):
  equality   where the float64 run leaves a relative gap >= 32 eps32 between best and second-best candidate at every pick, the kernel's
             index sequence equals the float64 one exactly;
  validity   everywhere else EVERY pick, measured in float64 against the kernel's own earlier picks, is within VALID_BOUND = 4 eps32
             (relative) of the true maximum.  Derivation, with u = eps32 / 2 the unit roundoff and float32 inputs: dx = fl(a - b) carries
             (1 + d), |d| <= u; its square (1 + d)^2 (1 + d'), three roundings; the two additions of non-negative terms add one each: the
             sum of squares is within 5 u; the square root halves that and rounds once more: 3.5 u = 1.75 eps32 per distance, and so per
             running minimum (the minimum of values each within 1.75 eps32).  The kernel's pick v has the largest FLOAT32 minimum, so its
             true minimum is at least (1 - 1.75 eps32) / (1 + 1.75 eps32) of any other point's: within 3.5 eps32, rounded up to 4 for the
             second-order terms.  (No squares underflow here: coordinates are O(1) and distinct points lie >= 1e-4 apart.)
"""
import functools
import importlib

import numpy as np
import pytest
import torch

import bones_wide_cases as BC
import fps_cases as C
import fps_ref as R

pytestmark = pytest.mark.gpu
L = importlib.import_module("3danimals_amd._lib")
sk = importlib.import_module("3danimals_amd.model.geometry.skinning")
util = importlib.import_module("3danimals_amd.model.geometry.util")
ops = importlib.import_module("3danimals_amd.ops")
VALID_BOUND = 4 * C.EPS32
TOL = 1e-6  # TOL of tests/test_bones_wide_gpu.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def sample(pts, k, start):
    """The kernel on CPU inputs -> (indices [N,k], points [N,k,3]) back on the CPU; the points are checked to be bit copies."""
    idx, got = ops.farthest_point_sample(pts.cuda(), k, start.cuda(), return_points=True)
    idx, got = idx.cpu(), got.cpu()
    assert idx.dtype == torch.int64 and idx.shape == (pts.shape[0], k) and int(idx.min()) >= 0 and int(idx.max()) < pts.shape[1]
    want = pts.gather(1, idx[..., None].expand(-1, -1, 3))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    return idx, got


def assert_picks(pts, start, idx, ref=None, what=""):
    """One cloud: equality where the float64 gaps allow it, validity of every pick otherwise.  -> whether equality was demanded."""
    k = len(idx)
    picks, gaps = ref if ref is not None else R.greedy(pts.numpy(), k, start)
    if gaps[:k].min() >= C.GAP_BOUND:
        assert np.array_equal(idx.numpy(), picks[:k]), (what, "first difference at pick", int(np.argmax(idx.numpy() != picks[:k])))
        return True
    short = R.pick_shortfall(pts.numpy(), idx.numpy())
    print(what, "gap", gaps[:k].min(), "largest shortfall / eps32", short.max() / C.EPS32)
    assert int(idx[0]) == picks[0] and short.max() <= VALID_BOUND, (what, int(short.argmax()), short.max() / C.EPS32)
    return False


@functools.lru_cache(maxsize=None)
def sweep_ref(V, n, k):
    pts, start = C.batch(V, max(C.SWEEP_N))
    return R.greedy(pts[n].numpy(), k, int(start[n]))


@pytest.mark.parametrize("V", C.SWEEP_V)
def test_wave_and_work_group_edges(V, dev):
    """V around the sizes at which a wave and a work-group fill up, k in {1, V // 4, V}, N in {1, 3, 40}; sampled points bit for bit;
    two calls give the same bits."""
    demanded = 0
    for N, k in C.sweep_combos(V):
        pts, start = C.batch(V, N)
        idx, got = sample(pts, k, start)
        again = sample(pts, k, start)
        assert torch.equal(idx, again[0]) and torch.equal(got.view(torch.int32), again[1].view(torch.int32))
        kmax = V if N < 40 or V <= 65 else V // 4
        demanded += sum(assert_picks(pts[n], int(start[n]), idx[n], sweep_ref(V, n, kmax), f"V={V} N={N} k={k} n={n}") for n in range(N))
    print("V", V, "clouds held to equality:", demanded)
    assert demanded > 0


@pytest.mark.parametrize("V", C.BOUNDARY_V)
def test_one_below_at_and_one_above_every_regime_boundary(V, dev):
    k = min(V // 4, C.BOUNDARY_K_MAX)
    pts, start = C.batch(V, 3)
    idx, _ = sample(pts, k, start)
    for n in range(3):
        assert_picks(pts[n], int(start[n]), idx[n], what=f"V={V} n={n}")


def test_equality_clouds_the_lattice_and_identical_points(dev):
    for name, (V, seed, start) in C.EQUALITY.items():
        idx, _ = sample(C.cloud(V, seed)[None], V, torch.tensor([start]))
        picks, gaps = R.greedy(C.cloud(V, seed).numpy(), V, start)
        assert gaps.min() >= C.GAP_BOUND and np.array_equal(idx[0].numpy(), picks), name
    lat = C.lattice()
    idx, _ = sample(lat[None].repeat(3, 1, 1), lat.shape[0], torch.tensor([C.LATTICE_START, 0, 239]))
    for n, s in enumerate((C.LATTICE_START, 0, 239)):  # exact distances: the lowest index wins every tie, in float32 as in float64
        assert np.array_equal(idx[n].numpy(), R.greedy(lat.numpy(), lat.shape[0], s)[0]), n
    for V, k, s in ((70, 5, 33), (1500, 9, 1499)):  # every distance is 0: index 0 from the second pick on, as in the reference
        idx, _ = sample(C.identical(V)[None], k, torch.tensor([s]))
        assert idx[0].tolist() == [s] + [0] * (k - 1)


def test_last_bit_of_the_square_root_decides_as_in_float32(dev):
    """The distance is the CORRECTLY ROUNDED float32 square root: on fps_cases.near_ties the second pick hangs on the last bit of two
    square roots (equal -> the lower index, A; else the farther one), and the kernel picks as the float32 statement evaluated by numpy
    picks, in every cloud.  (The equality clouds and the lattice cannot tell: their candidates lie far more than a last bit apart.)"""
    pts = C.near_ties()
    p = pts.numpy()
    d = p[:, 0:1] - p
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    rounded_together = int(((d2[:, 1] != d2[:, 2]) & (np.sqrt(d2[:, 1]) == np.sqrt(d2[:, 2]))).sum())
    assert d2.dtype == np.float32 and rounded_together >= 200  # different squares, the same correctly rounded root: only the last bit ties them
    idx, _ = sample(pts, 3, torch.zeros(pts.shape[0], dtype=torch.int64))
    want = np.stack([R.greedy32(p[n], 3, 0) for n in range(p.shape[0])])
    wrong = np.nonzero((idx.numpy() != want).any(1))[0]
    print("clouds picked differently from float32:", len(wrong), "of", len(p), "; picks of B:", int((want[:, 1] == 2).sum()))
    assert len(wrong) == 0, wrong[:10]
    # and whole sequences, in both regimes: every operation of the statement is correctly rounded, so the float32 run is reproduced exactly
    for V, k, seed in ((1025, 1025, 5), (6000, 1500, 6), (C.VALIDITY[0], 600, C.VALIDITY[2])):
        idx, _ = sample(C.cloud(V, seed)[None], k, torch.tensor([V // 2]))
        assert np.array_equal(idx[0].numpy(), R.greedy32(C.cloud(V, seed).numpy(), k, V // 2)), V


def test_validity_cloud_in_the_workspace_regime(dev):
    V, k, seed = C.VALIDITY
    assert V > ops.FPS_REG_MAX_V
    pts = C.cloud(V, seed)
    idx, _ = sample(pts[None], k, torch.tensor([V // 3]))
    short = R.pick_shortfall(pts.numpy(), idx[0].numpy())
    print("largest shortfall / eps32", short.max() / C.EPS32, "picks that are not a float64 maximum", int((short > 0).sum()))
    assert int(idx[0, 0]) == V // 3 and short.max() <= VALID_BOUND and len(set(idx[0].tolist())) == k


def test_nan_is_the_greatest_and_stays(dev):
    """csrc/fps.hip: a NaN distance is greater than every number, +inf included, and a running minimum keeps its NaN -- the order of
    torch.max / torch.minimum and of numpy.  So the first pick after the start is the lowest index with a NaN coordinate, and every
    pick after that is index 0.  A point with an infinite coordinate is infinitely far from the finite ones and at NaN from itself: once
    picked it is picked again every time.  Out-of-range starts are clamped."""
    for V in (200, 3000, 17000):
        pts = C.cloud(V, 123).clone()
        pts[90, 1] = float("nan")
        pts[37, 2] = float("nan")
        pts[150, 0] = float("inf")
        idx, _ = sample(pts[None].repeat(3, 1, 1), 6, torch.tensor([5, 37, 150]))
        assert idx.tolist() == [[5, 37, 0, 0, 0, 0], [37, 0, 0, 0, 0, 0], [150, 37, 0, 0, 0, 0]], V
        for n, s in enumerate((5, 37, 150)):
            assert np.array_equal(idx[n].numpy(), R.greedy(pts.numpy(), 6, s)[0])
        pts = C.cloud(V, 123).clone()
        pts[150, 0] = float("inf")  # no NaN seen from the start 5: 150 is infinitely far, and at NaN from itself from then on
        idx, _ = sample(pts[None], 4, torch.tensor([5]))
        assert np.array_equal(idx[0].numpy(), R.greedy(pts.numpy(), 4, 5)[0]) and idx[0].tolist() == [5, 150, 150, 150]
        idx, _ = sample(C.cloud(V, 123)[None].repeat(2, 1, 1), 3, torch.tensor([-7, V + 10]))
        assert idx[:, 0].tolist() == [0, V - 1]


def torch_loop(pts, k, start):
    saved, sk.DEVICE_FPS = sk.DEVICE_FPS, False
    try:
        return util.sample_farthest_points(pts, k, return_index=True, start=start)
    finally:
        sk.DEVICE_FPS = saved


def test_strided_input_and_gradient_through_util(dev):
    """[B,3,N] input as estimate_bones makes it (a transposed view), contiguous [B,3,N], and a slice of a wider tensor: the indices of
    the torch loop (equality clouds) and the same gradient with respect to pts."""
    names = ["v300a", "v300b"]
    clouds = torch.stack([C.cloud(*C.EQUALITY[n][:2]) for n in names]).cuda()
    start = torch.tensor([C.EQUALITY[n][2] for n in names]).cuda()
    wide = torch.zeros(2, 5, 300, device="cuda")
    wide[:, 1:4] = clouds.transpose(1, 2)
    for pts in (clouds.transpose(1, 2), clouds.transpose(1, 2).contiguous(), wide[:, 1:4]):
        a = pts.clone().requires_grad_(True) if pts.is_contiguous() else pts.detach().requires_grad_(True)
        b = a.detach().clone().requires_grad_(True)
        with L.KernelTimer() as timer:
            out, idx = util.sample_farthest_points(a, 75, return_index=True, start=start)
        assert timer.summary()["a3d_estimate_bones"][0] == 1
        out_t, idx_t = torch_loop(b, 75, start)
        assert torch.equal(idx, idx_t) and torch.equal(out, out_t)
        for n, name in enumerate(names):
            assert np.array_equal(idx[n].cpu().numpy(), R.greedy(clouds[n].cpu().numpy(), 75, int(start[n]))[0])
        w = torch.arange(out.numel(), device="cuda", dtype=torch.float32).reshape(out.shape)
        (out * w).sum().backward()
        (out_t * w).sum().backward()
        assert torch.equal(a.grad, b.grad) and float(a.grad.abs().sum()) > 0
    # the generator is consumed identically on both paths
    torch.manual_seed(5)
    _, i1 = util.sample_farthest_points(clouds.transpose(1, 2), 4, return_index=True)
    r1 = torch.rand(3, device="cuda")
    torch.manual_seed(5)
    saved, sk.DEVICE_FPS = sk.DEVICE_FPS, False
    try:
        _, i2 = util.sample_farthest_points(clouds.transpose(1, 2), 4, return_index=True)
    finally:
        sk.DEVICE_FPS = saved
    assert torch.equal(i1[:, 0], i2[:, 0]) and torch.equal(r1, torch.rand(3, device="cuda"))


def bones_resampled(seq, thr, seed=3, **switches):
    kw = dict(n_leg_bones=3, body_bones_mode="z_minmax_y+", bone_y_threshold=thr, **BC.KW)
    saved = {k: getattr(sk, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(sk, k, v)
        torch.manual_seed(seed)
        with L.KernelTimer() as timer:
            out = sk.estimate_bones(seq, resample=True, **kw)
        return out, timer.summary()
    finally:
        for k, v in saved.items():
            setattr(sk, k, v)


@pytest.mark.parametrize("shape,thr", [((1, 2), None), ((1, 2), 0.4), ((5, 8), None), ((5, 8), 0.4)])
def test_estimate_bones_resamples_in_one_call(shape, thr, dev, monkeypatch):
    """One-group (2 instances) and wide (40 instances) sizes: ONE a3d_estimate_bones call and nothing else on the timer, the torch loop
    never entered; bones within 1e-6 of the torch statements run on the kernel's own picks, chain and aux equal."""
    seq = BC.base(*shape).cuda()
    B, F, n, _ = seq.shape
    k = n // 4
    assert ops.estimate_bones_is_wide(B * F, k) == (B * F > 32)
    monkeypatch.setattr(util, "sample_farthest_points", lambda *a, **kw: pytest.fail("the torch loop was taken"))
    (bones, chain, aux), calls = bones_resampled(seq, thr)
    assert {name: c[0] for name, c in calls.items()} == {"a3d_estimate_bones": 1}
    again, _ = bones_resampled(seq, thr)
    assert torch.equal(again[0], bones)
    monkeypatch.undo()
    torch.manual_seed(3)
    start = torch.randint(n, [B * F], device=seq.device)  # the draw estimate_bones made
    idx = ops.farthest_point_sample(seq.reshape(-1, n, 3), k, start)
    for j in (0, B * F - 1):
        assert_picks(seq.reshape(-1, n, 3)[j].cpu(), int(start[j]), idx[j].cpu(), what=f"instance {j}")
    picked = seq.reshape(-1, n, 3).gather(1, idx[..., None].expand(-1, -1, 3)).reshape(B, F, k, 3)
    kw = dict(n_leg_bones=3, body_bones_mode="z_minmax_y+", bone_y_threshold=thr, **BC.KW)
    saved, sk.DEVICE_ESTIMATE_BONES = sk.DEVICE_ESTIMATE_BONES, False
    try:
        bones_t, chain_t, aux_t = sk.estimate_bones(picked, **kw)
    finally:
        sk.DEVICE_ESTIMATE_BONES = saved
    print("max |kernel - torch|", float((bones - bones_t).abs().max()))
    assert bones.shape == bones_t.shape and float((bones - bones_t).abs().max()) <= TOL
    assert repr(chain) == repr(chain_t) and aux == aux_t
    torch.manual_seed(3)
    cached = sk.estimate_bones(seq, resample=True, compute_kinematic_chain=False, aux=aux, **kw)  # a cached chain: the same bones
    assert torch.equal(cached, bones)
    L.poll_deferred()


def test_switch_off_takes_the_torch_loop(dev, monkeypatch):
    seq = BC.base(1, 2).cuda()
    monkeypatch.setattr(ops, "farthest_point_sample", lambda *a, **kw: pytest.fail("the kernel was taken"))
    entered = []
    loop = util.sample_farthest_points
    monkeypatch.setattr(util, "sample_farthest_points", lambda *a, **kw: entered.append(1) or loop(*a, **kw))
    (bones, _, _), calls = bones_resampled(seq, None, DEVICE_FPS=False)
    assert entered == [1] and calls["a3d_estimate_bones"][0] == 1 and torch.isfinite(bones).all()  # (the bones of the torch picks, on the device as before)
    L.poll_deferred()


def test_raw_sample_only_call_with_the_tail_is_taken(dev):
    """The tail itself, packed by hand: a sample-only call with null bones buffers samples; the same bytes cut to the public size are a
    plain call, which refuses those null buffers."""
    import ctypes

    pts, start = C.batch(65, 3)
    pts, start = pts.cuda(), start.cuda()
    idx = torch.full((3, 16), -1, dtype=torch.int64, device="cuda")
    got = torch.zeros(3, 16, 3, device="cuda")
    a = L.EstimateBonesArgs(N=3, V=65, pos=pts.data_ptr())
    block = ops.pack_fps_block(a, 16, True, start.data_ptr(), got.data_ptr(), idx.data_ptr())
    L.call("a3d_estimate_bones", ctypes.addressof(block), L.stream())
    assert torch.equal(idx, ops.farthest_point_sample(pts, 16, start)) and torch.equal(got, pts.gather(1, idx[..., None].expand(-1, -1, 3)))
    a.size = ctypes.sizeof(L.EstimateBonesArgs)
    assert L.lib().a3d_estimate_bones(ctypes.addressof(a), None) != 0


def test_no_host_synchronisation(dev):
    """ops.farthest_point_sample, util.sample_farthest_points (the draw of the first picks included) and estimate_bones(resample=True)
    with a cached chain enqueue their work and return: torch's sync debug mode raises on any read-back."""
    pts, start = C.batch(1025, 3)
    pts, start = pts.cuda(), start.cuda()
    seq = BC.base(5, 8).cuda()
    kw = dict(n_leg_bones=3, body_bones_mode="z_minmax_y+", bone_y_threshold=0.4, **BC.KW)
    torch.manual_seed(3)
    bones, _, aux = sk.estimate_bones(seq, resample=True, **kw)
    want = ops.farthest_point_sample(pts, 256, start)
    L.poll_deferred()
    torch.cuda.synchronize()
    torch.manual_seed(3)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with L.KernelTimer() as timer:
            cached = sk.estimate_bones(seq, resample=True, compute_kinematic_chain=False, aux=aux, **kw)
            idx = ops.farthest_point_sample(pts, 256, start)
            out, idx_u = util.sample_farthest_points(pts.transpose(1, 2), 256, return_index=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert timer.summary()["a3d_estimate_bones"][0] == 3
    assert torch.equal(cached, bones) and torch.equal(idx, want) and idx_u.shape == (3, 256) and out.shape == (3, 3, 256)
    L.poll_deferred()
