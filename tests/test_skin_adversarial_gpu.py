"""The posing kernels (csrc/skin.hip, csrc/bones.hip, csrc/bones_common.h) on the GPU against the float64 restatement
tests/skin_ref.py, on the cases of skin_ref.CASES: ops.skin, ops.skin_weights, ops.bone_transforms, ops.skin_pose and the dispatch of
model.geometry.skinning.skinning -- forward outputs and every gradient, every template instance (guarded and unguarded), chain depths
1..8, V below one quad group and one matrix step, the four shared / per-image combinations, the loop branches of the four launchers,
run-to-run behaviour and argument validation.

Tolerance.  Errors are in units of 2^-24 x magnitude (skin_ref).  skin_ref.MEASURED holds what the torch float32 path reaches per case
and quantity (measured and asserted on the CPU by tests/test_skin_cpu.py); a kernel gets 4 x that many units plus 4 ulp of the float64
value, and nothing else.  No vertex is left out.  tests/test_skin_cpu.py::test_bounds_catch_a_removed_piece shows the bounds bite.
"""
import functools
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skin_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("3danimals_amd.ops")


@pytest.fixture(scope="module")
def mods():
    m = lambda n: importlib.import_module("3danimals_amd." + n)
    return dict(skinning=m("model.geometry.skinning"), lib=m("_lib"))


@functools.lru_cache(maxsize=None)
def case_and_reference(name):
    """(case, float64 reference): computed once per case, shared by the tests that need it, never modified."""
    c = S.build(name)
    return c, S.evaluate(c)


def within(got, ref, name, key, what=""):
    got = got.detach().cpu()
    val, mag = ref[key]
    assert got.shape == val.shape and got.dtype == torch.float32, (name, key, tuple(got.shape))
    u = S.units(got, val, mag) if bool(torch.isfinite(got).all()) else float("inf")
    print(f"{name}{what}: {key} {u:.3f} units (torch fp32 path {S.figure(name, key)}, bound {S.allowed_units(name, key):.3f} + 4 ulp)")
    bad = S.bad_elements(got, val, mag, name, key)
    if bad.numel():
        i = tuple(bad[0].tolist())
        pytest.fail(f"{name}{what}: {key} outside the bound at {bad.shape[0]} elements, e.g. {i}: got {float(got[i])!r}, ref {float(val[i])!r}, "
                    f"magnitude {float(mag[i])!r} ({u:.2f} units)")


def run(c, ops, dev, sk=None):
    """Case ``c`` through the operator it names: key -> tensor (on the device)."""
    op, temp = c["op"], c["temperature"]
    bones = c["bones"].to(dev)
    up = lambda k: None if c.get(k) is None else c[k].to(dev)
    if op == "weights":
        return dict(w=ops.skin_weights(c["v"].to(dev), bones, max(c["v"].shape[0], bones.shape[0]), temp))
    if op == "bones":
        ang = c["angles"].to(dev).requires_grad_(True)
        M = ops.bone_transforms(bones, ang, c["chain"].to(dev))
        (ga,) = torch.autograd.grad(M, ang, up("g_T"))
        return dict(T=M, g_angles=ga)
    if op == "skin":
        v = c["v"].to(dev).requires_grad_(c.get("grad") != "T")
        T = c["T"].to(dev).requires_grad_(True)
        out = ops.skin(v, bones, T, temp)
        if c.get("grad") == "T":
            (gT,) = torch.autograd.grad(out, T, up("g_out"))
            return dict(out=out, g_T=gT)
        gv, gT = torch.autograd.grad(out, [v, T], up("g_out"))
        return dict(out=out, g_v=gv, g_T=gT)
    v = c["v"].to(dev).requires_grad_(c.get("grad") != "angles")
    ang = c["angles"].to(dev).requires_grad_(True)
    if op == "skinning":
        out, _ = sk.skinning(v[:, None], bones[:, None], c["tree"], ang[:, None], temperature=temp)
        gv, ga = torch.autograd.grad(out, [v, ang], up("g_out")[:, None])
        return dict(out=out[:, 0], g_v=gv, g_angles=ga)
    out, T = ops.skin_pose(v, bones, ang, c["chain"].to(dev), temp)
    outs = [(o, g) for o, g in ((out, up("g_out")), (T, up("g_T"))) if g is not None]
    ins = [ang] if c.get("grad") == "angles" else [v, ang]
    g = torch.autograd.grad([o for o, _ in outs], ins, [g for _, g in outs])
    res = dict(out=out, T=T, g_angles=g[-1])
    if len(ins) == 2:
        res["g_v"] = g[0]
    return res


def names(op, loops=False):
    return [n for n, s in S.CASES.items() if s["op"] == op and n.startswith("loop_") == loops]


def compare(name, ops, dev, sk=None, what=""):
    c, ref = case_and_reference(name)
    got = run(c, ops, dev, sk)
    for k in S.keys_of(c):
        within(got[k], ref, name, k, what)
    return c, ref, got


# ---------------------------------------------------------------------------------------------------------------- the operators
@pytest.mark.parametrize("name", names("skin"))
def test_skin_blend_against_float64(name, ops, dev):
    """a3d_skin_fwd / a3d_skin_bwd, transforms given: K in {1, 3, 19, 20, 21, 32, 33, 64} over the three kernel sizes, V in {1, 3, 63, 64,
    65, 257}, B in {1, 3}, vertices and bones shared or per image (a shared mesh's gradient is the sum over the images), and a gradient
    wanted by the transforms only (no g_v buffer)."""
    compare(name, ops, dev)


@pytest.mark.parametrize("name", names("weights"))
def test_skin_weights_against_float64(name, ops, dev):
    """ops.skin_weights: layout [K,Bw,V] for Bw = 1 and Bw = B at temperatures 1e-3, 0.05, 1, 50; every vertex's weights sum to 1
    within the weights' own bound (the float64 weights sum to 1, so the sum may be off by the sum over the bones of what each weight
    may be off by); coincident bones get equal weights bit for bit."""
    c, ref, got = compare(name, ops, dev)
    w = got["w"]
    Bw = max(c["v"].shape[0], c["bones"].shape[0])
    assert tuple(w.shape) == (c["K"], Bw, c["V"]) and Bw == (c["B"] if (c["vb"] or c["bb"]) else 1)
    dev_sum = (w.double().sum(0).cpu() - 1.0).abs()
    val, mag = ref["w"]
    bound = S.EPS * (S.allowed_units(name, "w") * mag + 4.0 * val.abs()).sum(0)
    print(f"{name}: |sum of weights - 1| <= {float(dev_sum.max()) / S.EPS:.2f} x 2^-24 (bound {float(bound.min()) / S.EPS:.2f} and up)")
    assert bool((dev_sum <= bound).all())
    assert torch.equal(c["bones"][:, 0], c["bones"][:, 1]) and torch.equal(w[0], w[1])


@pytest.mark.parametrize("name", names("bones"))
def test_bone_transforms_against_float64(name, ops, dev):
    """a3d_bone_transforms_*: every skeleton family up to K = 64 with D = 8 (the large-LDS launch of the backward), N in {1, 33}, bones
    shared and per instance, every angle set, one-hot g_M rows (a link credited to the wrong bone shows)."""
    compare(name, ops, dev)


@pytest.mark.parametrize("name", names("pose"))
def test_skin_pose_against_float64(name, ops, dev):
    """a3d_skin_pose_*: K in {1, 2, 3, 8, 19} on the guarded instances, K = 20 on the unguarded one with D = 1, 2 and the quadruped
    tree's depth; loss on the vertices, on the transforms only (g_out is None) and on both; gradient to the angles only.  The same
    case under no_grad (no products buffer, no extra work-group) gives the same outputs."""
    c, ref, got = compare(name, ops, dev)
    with torch.no_grad():
        out, T = ops.skin_pose(c["v"].to(dev), c["bones"].to(dev), c["angles"].to(dev), c["chain"].to(dev), c["temperature"])
    within(out, ref, name, "out", " (no_grad)")
    within(T, ref, name, "T", " (no_grad)")
    assert torch.equal(out, got["out"]) and torch.equal(T, got["T"])


def test_skinning_dispatch_takes_the_two_launch_path_for_21_bones(ops, dev, mods):
    """model.geometry.skinning.skinning with K = 21 (above a3d_skin_pose_max_bones): a3d_bone_transforms_* + a3d_skin_*, still the
    float64 answer.  A chain of depth 9 is above both paths' limit of 8 links: skinning() has no fallback for it and raises the
    library's argument error from a3d_bone_transforms_fwd."""
    sk, L = mods["skinning"], mods["lib"]
    with L.KernelTimer() as timer:
        compare("skinning_wide21_v65", ops, dev, sk)
    calls = {n: k for n, (k, _) in timer.summary().items() if n.startswith(("a3d_skin", "a3d_bone"))}
    assert calls == {"a3d_bone_transforms_fwd": 1, "a3d_skin_fwd": 1, "a3d_skin_bwd": 1, "a3d_bone_transforms_bwd": 1}, calls
    tree = S._tree_of([k - 1 for k in range(9)])
    assert S.chain_table(tree).shape == (9, 9) and not ops.skin_pose_supported(9, 9)
    with pytest.raises(L.A3DError, match="a3d_bone_transforms_fwd.*invalid argument"):
        sk.skinning(torch.rand(1, 1, 5, 3, device=dev), torch.rand(1, 1, 9, 2, 3, device=dev), tree, torch.zeros(1, 1, 9, 3, device=dev))


# ---------------------------------------------------------------------------------------------------------------- loop branches
def _up(a, b):
    return (a + b - 1) // b


def test_skin_fwd_two_groups_per_work_group(ops, dev):
    """a3d_skin_fwd: groups = ceil(ceil(V / 64) / 128) = 2, and the last work-group's second group lies wholly past V (the break)."""
    name = "loop_skin_fwd_v8200_b2"
    V = S.CASES[name]["V"]
    ngroups = _up(V, 64)
    groups = _up(ngroups, 128)
    grid = _up(ngroups, groups)
    assert groups == 2 and ((grid - 1) * groups + 1) * 64 >= V and (grid - 1) * groups * 64 < V and V % 64 != 0
    compare(name, ops, dev)


def test_skin_pose_fwd_two_groups_and_second_backward(ops, dev):
    """a3d_skin_pose_fwd: groups = ceil(ceil(V / 64) B / 1024) = 2 with a last group past V; a second backward through the same graph
    (the buffer the forward cleared served the first: the memset path) gives the same gradients within the same bound."""
    name = "loop_pose_fwd_b16_v4100"
    s = S.CASES[name]
    ngroups = _up(s["V"], 64)
    groups = max(1, _up(ngroups * s["B"], 1024))
    grid = _up(ngroups, groups)
    assert groups == 2 and ((grid - 1) * groups + 1) * 64 >= s["V"] and s["V"] % 64 != 0
    c, ref = case_and_reference(name)
    v, ang = c["v"].to(dev).requires_grad_(True), c["angles"].to(dev).requires_grad_(True)
    out, T = ops.skin_pose(v, c["bones"].to(dev), ang, c["chain"].to(dev), c["temperature"])
    within(out, ref, name, "out")
    within(T, ref, name, "T")
    for what in (" (first backward)", " (second backward)"):
        gv, ga = torch.autograd.grad([out, T], [v, ang], [c["g_out"].to(dev), c["g_T"].to(dev)], retain_graph=True)
        within(gv, ref, name, "g_v", what)
        within(ga, ref, name, "g_angles", what)


def test_skin_pose_bwd_two_chunks_per_work_group(ops, dev):
    """a3d_skin_pose_bwd: ceil(ceil(V / 256) B / 768) = 2 chunks per work-group, the last chunk partial."""
    name = "loop_pose_bwd_b16_v12289"
    s = S.CASES[name]
    cpb = max(1, _up(_up(s["V"], 256) * s["B"], 768))
    assert cpb == 2 and s["V"] % 256 != 0 and s["V"] > 512
    compare(name, ops, dev)


def test_skin_bwd_two_chunks_per_work_group(ops, dev):
    """a3d_skin_bwd: ceil(ceil(V / 256) B / 4096) = 2 chunks per work-group, the last chunk partial (K = 3 keeps the float64 side small)."""
    name = "loop_skin_bwd_b3_v349701_k3"
    s = S.CASES[name]
    cpb = max(1, _up(_up(s["V"], 256) * s["B"], 4096))
    assert cpb == 2 and s["V"] % 256 != 0
    compare(name, ops, dev)


# ---------------------------------------------------------------------------------------------------------------- run to run
@pytest.mark.parametrize("name", ["skin_k21_v257_batched_batched", "pose_quadruped_v257_shared_verts", "skinning_wide21_v65"])
def test_three_runs_agree(name, ops, dev, mods):
    """Forward outputs and g_v are bit-identical across three runs.  g_T of the two-launch path and g_angles of the fused path are sums
    of atomics over work-groups: their run-to-run spread stays inside the bound their error is held to (nothing tighter is asserted)."""
    c, ref = case_and_reference(name)
    runs = [run(c, ops, dev, mods["skinning"]) for _ in range(3)]
    for k in S.keys_of(c):
        atomic = (k == "g_T" and c["op"] == "skin") or (k == "g_angles" and c["op"] in ("pose", "skinning"))
        for r in runs[1:]:
            if not atomic:
                assert torch.equal(r[k], runs[0][k]), (name, k)
            else:
                val, mag = ref[k]
                bound = S.EPS * (S.allowed_units(name, k) * mag + 4.0 * val.abs())
                spread = (r[k].double().cpu() - runs[0][k].double().cpu()).abs()
                print(f"{name}: {k} spread {float((spread / (S.EPS * mag.clamp_min(1e-300))).max()):.3f} units")
                assert bool((spread <= bound).all()), (name, k)


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_invalid_arguments_are_refused_before_any_launch(dev, mods):
    """K = 65, temperature 0, a v_batch that is neither 1 nor B, K = 21 for the pose entries and D = 9 each return the argument error,
    and no kernel runs: the output buffers keep the value they were filled with."""
    L = mods["lib"]
    ptr, st = L.ptr, L.stream
    f = lambda *s: torch.full(s, 7.0, device=dev)
    B, V = 3, 10
    outs = []

    def refused(entry, *args):
        with pytest.raises(L.A3DError, match=entry + ".*invalid argument"):
            L.call(entry, *args)

    def skin_fwd(K, temp, vb, B=B):
        v, bones, T, out, w = f(B, V, 3), f(B, K, 2, 3), f(B, K, 12), f(B, V, 3), f(K, B, V)
        outs.extend([out, w])
        refused("a3d_skin_fwd", ptr(v), vb, ptr(bones), B, ptr(T), B, V, K, temp, ptr(out), ptr(w), None, st())

    def skin_bwd(K, temp, vb):
        g, v, bones, T, gv, gT = f(B, V, 3), f(B, V, 3), f(B, K, 2, 3), f(B, K, 12), f(B, V, 3), f(B, K, 12)
        outs.extend([gv, gT])
        refused("a3d_skin_bwd", ptr(g), ptr(v), vb, ptr(bones), B, ptr(T), B, V, K, temp, ptr(gv), ptr(gT), 0, st())

    def pose(K, D):
        v, bones, ang, out, T, ga = f(B, V, 3), f(B, K, 2, 3), f(B, K, 3), f(B, V, 3), f(B, K, 12), f(B, K, 3)
        chain = torch.full((K, D), -1, dtype=torch.int32, device=dev)
        ps = f(B, K * D * 24 + K * 36)
        outs.extend([out, T, ga, ps])
        refused("a3d_skin_pose_fwd", ptr(v), B, ptr(bones), B, ptr(ang), ptr(chain), B, V, K, D, 1.0, ptr(out), ptr(T), ptr(ps), ptr(ga), st())
        refused("a3d_skin_pose_bwd", ptr(out), ptr(v), B, ptr(bones), B, ptr(T), ptr(ps), ptr(ang), ptr(chain), B, V, K, D, 1.0, ptr(out), None,
                ptr(ga), 0, st())

    def bones_entry(K, D):
        bones, ang, M, ga = f(B, K, 2, 3), f(B, K, 3), f(B, K, 12), f(B, K, 3)
        chain = torch.full((K, D), -1, dtype=torch.int32, device=dev)
        outs.extend([M, ga])
        refused("a3d_bone_transforms_fwd", ptr(bones), B, ptr(ang), ptr(chain), B, K, D, ptr(M), st())
        refused("a3d_bone_transforms_bwd", ptr(M), ptr(bones), B, ptr(ang), ptr(chain), B, K, D, ptr(ga), st())

    skin_fwd(65, 1.0, B)
    skin_fwd(4, 0.0, B)
    skin_fwd(4, 1.0, 2)
    skin_bwd(65, 1.0, B)
    skin_bwd(4, 0.0, B)
    skin_bwd(4, 1.0, 2)
    pose(21, 2)
    pose(4, 9)
    bones_entry(65, 2)
    bones_entry(4, 9)
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)
