"""csrc/articulation.hip through 3danimals_amd/articulation.py on the device, every element against the float64 restatement of
tests/articulation_ref.py under the project's usual rule (4 x the units the torch float32 statement reaches, plus 4 ulp of the float64
value).  The shapes are the smallest at which each mechanism can go wrong (tests/articulation_cases.py), not the workload's."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import articulation_cases as C  # noqa: E402
import articulation_ref as R  # noqa: E402
import test_articulation_cpu as T  # noqa: E402  (run_desc, run_limits, limits_of: how a case is run)

pytestmark = pytest.mark.gpu
A = importlib.import_module("3danimals_amd.articulation")
L = importlib.import_module("3danimals_amd._lib")
ops = importlib.import_module("3danimals_amd.ops")
DEV = "cuda"
KEYS = ("pos", "feat", "g_feat", "g_patch")


def _check(out, ref, table_name):
    for k in ref:
        bad = R.bad_elements(out[k], *ref[k], R.figure(table_name, k))
        print(f"{table_name}: {k} {R.units(out[k], *ref[k]):.3f} units (torch float32: {R.figure(table_name, k)})")
        assert len(bad) == 0, (table_name, k, len(bad), bad[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------- descriptors
@pytest.mark.parametrize("name", list(C.DESC_CASES))
def test_descriptors_against_float64(name):
    """Forward and both gradients, every element; the same bits on a second run; the gradient of patch_feat in patch_feat's strides when
    it is dense (NCHW, the permuted NHWC view) and contiguous when it is not (the channel slice)."""
    c = C.build_desc(name)
    out = T.run_desc(A.bone_inputs, c, DEV)
    assert all(out[k].is_cuda and out[k].dtype == torch.float32 for k in KEYS if k in out)
    ref = R.evaluate_desc(c, out["pos"][..., :2])
    assert sorted(ref) == sorted(k for k in out if not k.startswith("_"))
    _check(out, ref, f"desc/{name}")
    again = T.run_desc(A.bone_inputs, c, DEV)
    for k in ref:
        assert torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)), k
    if "g_patch" in out:
        leaf = out["_patch_leaf"]
        assert out["g_patch"].shape == leaf.shape
        if c["layout"] == "slice":
            assert not leaf.is_contiguous() and out["g_patch"].is_contiguous()
        else:
            assert out["g_patch"].stride() == leaf.stride() or min(leaf.shape[1:]) == 1
    if name in C.NON_FINITE:  # non-finite in the same places as the torch statement; zero sample, zero scatter there
        _, tpos = A._bone_inputs_torch(c["bones"], c["mvp"], c["w2c"], C.Z_OFFSET, C.SPATIAL_SCALE)
        pos = out["pos"].cpu()
        assert torch.equal(torch.isnan(pos), torch.isnan(tpos)) and torch.equal(torch.isinf(pos), torch.isinf(tpos))
        assert not torch.isfinite(pos[0, list(C.NON_FINITE_BONES), :2]).all(1).any()
        sampled = out["feat"][0, list(C.NON_FINITE_BONES)][:, (c["D"] if "global" in c["mode"] else 0):]
        assert (sampled == 0).all()
        assert torch.isfinite(out["feat"]).all() and torch.isfinite(out["g_patch"]).all()
        lone = C.build_desc(name)  # the scatter of those three bones alone is nothing at all
        lone["g"] = torch.zeros_like(lone["g"])
        lone["g"][0, list(C.NON_FINITE_BONES)] = c["g"][0, list(C.NON_FINITE_BONES)]
        lone["g"][..., :(c["D"] if "global" in c["mode"] else 0)] = 0
        assert (T.run_desc(A.bone_inputs, lone, DEV)["g_patch"] == 0).all()


def test_one_entry_point_call_each_way():
    c = C.build_desc("n3_k20_cat_dbelow_32x32_nchw")
    feat = c["feat"].to(DEV).requires_grad_(True)
    patch = c["patch"].to(DEV).requires_grad_(True)
    args = [c[k].to(DEV) for k in ("bones", "mvp", "w2c")]
    with L.KernelTimer() as timer:
        bf, pos = A.bone_inputs(*args, C.Z_OFFSET, C.SPATIAL_SCALE, feat, patch)
        fwd = {k: v[0] for k, v in timer.summary().items()}
        bf.backward(c["g"].to(DEV))
        both = {k: v[0] for k, v in timer.summary().items()}
    assert fwd == {"a3d_bone_inputs_fwd": 1} and both == {"a3d_bone_inputs_fwd": 1, "a3d_bone_inputs_bwd": 1}
    lc = C.build_limits("k20_n3_magicpony")
    x = lc["x"].to(DEV).requires_grad_(True)
    with L.KernelTimer() as timer:
        angles, reg = A.constrain_angles(x, T.limits_of(lc["kind"], lc["cfg"]), return_reg=True)
        fwd = {k: v[0] for k, v in timer.summary().items()}
        (angles.sum() + reg).backward()
        both = {k: v[0] for k, v in timer.summary().items()}
    assert fwd == {"a3d_constrain_angles_fwd": 1} and both == {"a3d_constrain_angles_fwd": 1, "a3d_constrain_angles_bwd": 1}


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_bf16_patch_feat_under_autocast(layout):
    """float32 outputs, a bf16 gradient in the patch's own strides; the values are those of the bf16-rounded patch in float32."""
    c = C.build_desc("n3_k5_cbelow_dabove_3x5_nhwc_shared")
    c["patch"] = c["patch"].bfloat16().float()
    c["layout"] = layout
    ref_out = T.run_desc(A.bone_inputs, c, DEV)
    feat = c["feat"].to(DEV).requires_grad_(True)
    patch = C.layout_of(c["patch"].to(DEV), layout).bfloat16().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        bf, pos = A.bone_inputs(c["bones"].to(DEV), c["mvp"].to(DEV), c["w2c"].to(DEV), C.Z_OFFSET, C.SPATIAL_SCALE, feat, patch, c["mode"])
    assert bf.dtype == torch.float32 and pos.dtype == torch.float32
    assert torch.equal(bf, ref_out["feat"]) and torch.equal(pos, ref_out["pos"])
    g_feat, g_patch = torch.autograd.grad(bf, [feat, patch], c["g"].to(DEV))
    assert g_patch.dtype == torch.bfloat16 and g_feat.dtype == torch.float32
    assert torch.equal(g_feat, ref_out["g_feat"]) and torch.equal(g_patch, ref_out["g_patch"].bfloat16())


def test_sizes_the_kernels_refuse_take_the_torch_statement_and_device_false_too():
    rng = np.random.default_rng(5)
    K = L.ARTICULATION_MAX_BONES + 1
    bones = torch.from_numpy(rng.uniform(-0.5, 0.5, (1, K, 2, 3))).float().to(DEV)
    mvp, w2c = (t.to(DEV) for t in C.camera(2, rng))
    feat, patch = torch.randn(2, 3, device=DEV), torch.randn(2, 4, 3, 5, device=DEV)
    with L.KernelTimer() as timer:
        bf, pos = A.bone_inputs(bones, mvp, w2c, C.Z_OFFSET, C.SPATIAL_SCALE, feat, patch)
        limits = A.ArticulationLimits(0.5, np.ones((K, 3)))
        angles = A.constrain_angles(torch.randn(2, K, 3, device=DEV), limits)
        assert timer.summary() == {}
    assert bf.shape == (2, K, 7) and pos.shape == (2, K, 9) and angles.shape == (2, K, 3)
    with pytest.raises(ValueError):
        ops.bone_inputs(bones, mvp, w2c, C.Z_OFFSET, C.SPATIAL_SCALE, feat, patch)
    c = C.build_desc("n3_k5_sample_cat_3x5_nchw_shared")
    on = T.run_desc(A.bone_inputs, c, DEV)
    A.DEVICE = False
    try:
        with L.KernelTimer() as timer:
            off = T.run_desc(A.bone_inputs, c, DEV)
            assert timer.summary() == {}
    finally:
        A.DEVICE = True
    assert off["feat"].is_cuda and sorted(on) == sorted(off)
    for k in KEYS:  # the two settings agree
        if k in on:
            assert torch.allclose(on[k], off[k], rtol=1e-5, atol=1e-5), k
    lc = C.build_limits("k20_n3_magicpony")
    limits = T.limits_of(lc["kind"], lc["cfg"])
    lon = T.run_limits(A.constrain_angles, lc, limits, DEV)
    A.DEVICE = False
    try:
        with L.KernelTimer() as timer:
            loff = T.run_limits(A.constrain_angles, lc, limits, DEV)
            assert timer.summary() == {}
    finally:
        A.DEVICE = True
    for k in lon:
        assert torch.allclose(lon[k], loff[k], rtol=1e-5, atol=1e-6), k


def test_argument_validation_raises_before_any_launch():
    c = C.build_desc("n3_k5_sample_cat_3x5_nchw_shared")
    b, mvp, w2c, feat, patch = (c[k].to(DEV) for k in ("bones", "mvp", "w2c", "feat", "patch"))
    limits = A.limits_base(8, 4, 3, 0.1, 60)
    with L.KernelTimer() as timer:
        for bad in (lambda: A.bone_inputs(b, mvp[:2], w2c, 10.0, 7.0), lambda: A.bone_inputs(b[0], mvp, w2c, 10.0, 7.0),
                    lambda: A.bone_inputs(b, mvp, w2c, 10.0, 0.0), lambda: A.bone_inputs(b, mvp, w2c, 10.0, 7.0, feat, patch, "dino"),
                    lambda: A.bone_inputs(b, mvp, w2c, 10.0, 7.0, feat[:, None], patch), lambda: A.bone_inputs(b, mvp, w2c, 10.0, 7.0, feat, patch[:2]),
                    lambda: A.constrain_angles(torch.zeros(3, 19, 3, device=DEV), limits), lambda: A.constrain_angles(torch.zeros(3, 20, 3, device=DEV).long(), limits),
                    lambda: ops.constrain_angles(torch.zeros(3, 20, 3, device=DEV), limits.scale_on(DEV).double(), 0.1),
                    lambda: ops.constrain_angles(torch.zeros(3, 20, 3, device=DEV), limits.scale_on(DEV)[:19], 0.1)):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(L.A3DError):
            ops.bone_inputs(b.cpu(), mvp, w2c, 10.0, 7.0)
        with pytest.raises(L.A3DError):
            ops.constrain_angles(torch.zeros(3, 20, 3), limits.scale, 0.1)
        assert timer.summary() == {}


# ---------------------------------------------------------------------------------------------------------------- limits
@pytest.mark.parametrize("name", list(C.LIMIT_CASES))
def test_limits_against_float64(name):
    """angles, reg and the gradient arriving through both; the same bits on a second run."""
    c = C.build_limits(name)
    limits = T.limits_of(c["kind"], c["cfg"])
    out = T.run_limits(A.constrain_angles, c, limits, DEV)
    assert out["reg"].dim() == 0 and out["reg"].dtype == torch.float32
    _check(out, R.evaluate_limits(c), f"limits/{name}")
    again = T.run_limits(A.constrain_angles, c, limits, DEV)
    for k in out:
        assert torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)), k
    zero = limits.scale_on(DEV) == 0
    assert (out["angles"][:, zero] == 0).all() and (out["g_x"][:, zero] == 0).all()
    sat = (c["x"].abs() * limits.multiplier >= 20).to(DEV)
    assert (sat.any() or c["x"].numel() < 3 * len(C.SPECIAL_X)) and (out["g_x"][sat] == 0).all()  # a saturated tanh: the gradient is exactly 0


@pytest.mark.parametrize("which", [dict(g_angles=True, g_reg=False), dict(g_angles=False, g_reg=True)])
def test_limits_gradient_through_one_output_alone(which):
    name = "k20_n3_fauna_constraints"
    c = C.build_limits(name)
    out = T.run_limits(A.constrain_angles, c, T.limits_of(c["kind"], c["cfg"]), DEV, **which)
    ref = R.evaluate_limits(c, **which)
    assert len(R.bad_elements(out["g_x"], *ref["g_x"], R.figure(f"limits/{name}", "g_x"))) == 0
    x = c["x"].reshape(3, 1, 20, 3).to(DEV).requires_grad_(True)  # [B,F,K,3] in, the same shape out; without reg
    angles = A.constrain_angles(x, T.limits_of(c["kind"], c["cfg"]))
    assert angles.shape == x.shape and torch.equal(angles.reshape(3, 20, 3), out["angles"])
    if which["g_angles"]:
        g, = torch.autograd.grad(angles, x, c["g_angles"].reshape(3, 1, 20, 3).to(DEV))
        assert torch.equal(g.reshape(3, 20, 3), out["g_x"])


def test_limits_at_infinity_and_at_zero_factors():
    """x = +-inf: +-S out and gradient 0; at a bone whose factor is 0 exactly 0 out and exactly 0 gradient (the reference gives NaN
    there: the one documented difference), reg finite."""
    limits = A.limits_base(8, 4, 3, 0.1, 60, static_root_bones=True, constrain_legs=True, extra_constraints=True)
    S = limits.scale_on(DEV)
    assert (S == 0).any() and (S != 0).any()
    x = torch.full((3, 20, 3), float("inf"), device=DEV)
    x[1] = -x[1]
    x[2] = torch.tensor([0.0, 1e-30, -1e-30]).to(DEV)
    x.requires_grad_(True)
    angles, reg = A.constrain_angles(x, limits, return_reg=True)
    g, = torch.autograd.grad((angles * 3.0).sum() + reg * 2.0, x)
    assert torch.equal(angles[0], S) and torch.equal(angles[1], -S) and torch.isfinite(reg)
    assert (g[:2] == 0).all() and torch.isfinite(g).all() and (g[2][S == 0] == 0).all() and (g[2][S != 0] != 0).all()
    tiny = (S.double() * 0.1 * x[2].detach().double()).float()
    assert torch.allclose(angles[2], tiny, rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------------------------- golden rows
@pytest.mark.parametrize("name", list(C.GOLDEN_LIMITS))
def test_limits_golden_through_the_device_path(name):
    gold = np.load(os.path.join(T.GOLDEN, "articulation_limits.npz"))[name]
    kind, cfg = C.GOLDEN_LIMITS[name]
    x = C.golden_limits_x(name)
    c = dict(kind=kind, cfg=cfg, x=x, g_angles=torch.zeros_like(x), g_reg=torch.zeros(()))
    ref, mag = R.evaluate_limits(c)["angles"]
    angles = A.constrain_angles(x.to(DEV), T.limits_of(kind, cfg))
    assert angles.shape == x.shape
    fig = R.figure(f"golden_limits/{name}", "angles")
    assert len(R.bad_elements(angles, ref, mag, fig)) == 0
    assert len(R.bad_elements(gold, ref, mag, fig)) == 0


@pytest.mark.parametrize("name", list(C.GOLDEN_BONES))
def test_bones_golden_through_the_device_path(name):
    g = np.load(os.path.join(T.GOLDEN, "articulation_bones.npz"))
    c = T._golden_desc_case(name)
    bones = c["bones"][:, None].to(DEV) if c["bones"].shape[0] > 1 else c["bones"].to(DEV)  # ([B,F,K,2,3]: flattened)
    bf, pos = A.bone_inputs(bones, c["mvp"].to(DEV), c["w2c"].to(DEV), C.Z_OFFSET, C.SPATIAL_SCALE, c["feat"].to(DEV), c["patch"].to(DEV), c["mode"])
    assert tuple(bf.shape) == g[name + "_feat"].shape and tuple(pos.shape) == g[name + "_pos"].shape
    ref = R.evaluate_desc(c, pos[..., :2])
    _check({"pos": pos, "feat": bf}, ref, f"golden_bones/{name}")
    assert float(np.abs(bf.cpu().numpy() - g[name + "_feat"]).max()) <= 1e-5 and float(np.abs(pos.cpu().numpy() - g[name + "_pos"]).max()) <= 1e-5
