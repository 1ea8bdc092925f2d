"""csrc/pose.hip through 3danimals_amd/pose.py on the device, every element of every case against the float64 restatement of
tests/pose_ref.py under the project's usual rule (4 x the units the torch float32 statement reaches, plus 4 ulp of the float64 value);
rot_idx and rand_pose_flag equal to what the reference's own functions returned.  The shapes are the smallest at which each mechanism can
go wrong (tests/pose_cases.py), not the workload's."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_cases as C  # noqa: E402
import pose_ref as R  # noqa: E402
import test_pose_cpu as T  # noqa: E402  (run_fused, run_cameras, run_random_view: how a case is run)

pytestmark = pytest.mark.gpu
P = importlib.import_module("3danimals_amd.pose")
L = importlib.import_module("3danimals_amd._lib")
ops = importlib.import_module("3danimals_amd.ops")
DEV = "cuda"


def _check(out, ref, table_name):
    for k, v in ref.items():
        if not isinstance(v, tuple):
            assert out[k].dtype == torch.int64 and np.array_equal(out[k].cpu().numpy(), v), (table_name, k)
            continue
        assert out[k].is_cuda and out[k].dtype == torch.float32, k
        fig = R.figure(table_name, k)
        print(f"{table_name}: {k} {R.units(out[k], *v):.3f} units (torch float32: {fig})")
        bad = R.bad_elements(out[k], *v, fig)
        assert len(bad) == 0, (table_name, k, len(bad), bad[:4].tolist())


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("name", list(C.FUSED_CASES))
def test_fused_against_float64(name):
    """The nine float outputs and g_raw, every element; the two integer outputs equal to the reference's; the same bits on a second run."""
    c = C.build_fused(name)
    out = T.run_fused(c, DEV)
    _check(out, R.evaluate_fused(c), f"fused/{name}")
    gold = np.load(os.path.join(T.GOLDEN, "pose_pick.npz"))
    for k in ("rot_idx", "rand_pose_flag"):
        assert np.array_equal(out[k].cpu().numpy(), gold[f"{name}/{k}"]), k
    again = T.run_fused(c, DEV)
    for k in out:
        if not k.startswith("_"):
            assert _same_bits(out[k], again[k]), k
    assert not out["rot_idx"].requires_grad and not out["rand_pose_flag"].requires_grad
    assert torch.equal(out["_raw_leaf"].detach().cpu(), c["raw"])


@pytest.mark.parametrize("name", list(T.EACH_CASES))
def test_fused_gradient_through_every_output_and_through_each_alone(name):
    """The case's gradient again with all nine outputs fed, and with each output fed alone (the others absent, not zero tensors): what
    nothing feeds is exactly 0 -- the forward columns of a hypothesis that was not picked, unless poses_raw itself is fed."""
    c = C.build_fused(name)
    for key, grads in [("g_all", C.FLOAT_OUTPUTS)] + [("g_" + k, (k,)) for k in C.FLOAT_OUTPUTS]:
        out = T.run_fused(c, DEV, grads=grads)
        ref = R.evaluate_fused(c, grads)["g_raw"]
        fig = R.figure(f"fused_each/{name}", key)
        print(f"fused_each/{name}: {key} {R.units(out['g_raw'], *ref):.3f} units (torch float32: {fig})")  # (units asserts the exact zeros)
        assert len(R.bad_elements(out["g_raw"], *ref, fig)) == 0, grads
        if "poses_raw" not in grads:
            H = c["H"]
            vec = out["g_raw"][:, :4 * H].reshape(-1, H, 4)[..., 1:]
            other = torch.arange(H, device=DEV)[None] != out["rot_idx"][:, None]
            assert (vec[other] == 0).all(), grads


def test_one_entry_point_call_each_way():
    c = C.build_fused("n5_h8_oct_it7000_rand")
    raw = c["raw"].to(DEV).requires_grad_(True)
    with L.KernelTimer() as timer:
        out = P.predict_cameras(raw, c["total_iter"], **T._kwargs(c, DEV))
        fwd = {k: v[0] for k, v in timer.summary().items()}
        res = dict(zip(T.OUTPUTS, out[:6]), **out[6])
        torch.autograd.grad([res[k] for k in C.FLOAT_OUTPUTS], raw, [c["g"][k].to(DEV) for k in C.FLOAT_OUTPUTS])
        both = {k: v[0] for k, v in timer.summary().items()}
    assert fwd == {"a3d_pose_cameras_fwd": 1} and both == {"a3d_pose_cameras_fwd": 1, "a3d_pose_cameras_bwd": 1}
    cc = C.build_cameras("n3_extra")
    pose = cc["pose"].to(DEV).requires_grad_(True)
    with L.KernelTimer() as timer:
        cams = P.cameras_from_pose(pose, C.Z_OFFSET, C.FOV, offset_extra=cc["offset_extra"])
        fwd = {k: v[0] for k, v in timer.summary().items()}
        torch.autograd.grad(list(cams), pose, [cc["g"][k].to(DEV) for k in T.CAMERA_KEYS])
        both = {k: v[0] for k, v in timer.summary().items()}
    assert fwd == {"a3d_cameras_from_pose_fwd": 1} and both == {"a3d_cameras_from_pose_fwd": 1, "a3d_cameras_from_pose_bwd": 1}
    v = C.build_random_view("bins360")
    w2c_pred, degree = v["w2c_pred"].to(DEV), v["rand_degree"].to(DEV)
    with L.KernelTimer() as timer:
        P.random_view_cameras(w2c_pred, degree, C.FOV, 360)
        assert {k: n[0] for k, n in timer.summary().items()} == {"a3d_random_view_cameras": 1}


def test_non_finite_values_appear_where_the_torch_statement_has_them():
    c = C.build_fused(C.NON_FINITE)
    with torch.no_grad():
        dev = P.predict_cameras(c["raw"].to(DEV), c["total_iter"], **T._kwargs(c, DEV))
        host = P.predict_cameras(c["raw"], c["total_iter"], **C.fused_kwargs(c))
    seen = 0
    for a, b in list(zip(dev[:6], host[:6])) + [(dev[6][k], host[6][k]) for k in ("rot_prob", "rot_logit", "rots_probs")]:
        a = a.cpu()
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isposinf(a), torch.isposinf(b)) and torch.equal(torch.isneginf(a), torch.isneginf(b))
        fin = torch.isfinite(b)
        assert torch.allclose(a[fin], b[fin], rtol=1e-5, atol=1e-6)
        assert not fin.all()  # (the case reaches every output)
        seen += int((~fin).sum())
    assert seen > 50 and torch.isfinite(dev[3][4:]).all()  # (softplus, exp and tanh of an infinity are finite: image 4 is a camera)
    assert torch.equal(dev[6]["rot_idx"].cpu(), host[6]["rot_idx"]) and torch.equal(dev[6]["rand_pose_flag"].cpu(), host[6]["rand_pose_flag"])


@pytest.mark.parametrize("name", list(C.CAMERA_CASES))
def test_cameras_alone_against_float64(name):
    c = C.build_cameras(name)
    out = T.run_cameras(c, DEV)
    _check(out, R.evaluate_cameras(c), f"cameras/{name}")
    again = T.run_cameras(c, DEV)
    assert all(_same_bits(out[k], again[k]) for k in out)
    for k in T.CAMERA_KEYS:  # each gradient alone: the others are absent, not zero tensors
        one = T.run_cameras(c, DEV, grads=(k,))
        ref = R.evaluate_cameras(c, (k,))["g_pose"]
        R.units(one["g_pose"], *ref)  # (asserts the exact zeros)
        assert len(R.bad_elements(one["g_pose"], *ref, R.figure(f"cameras_each/{name}", "g_" + k))) == 0, k


def test_cameras_alone_agree_with_the_tail_of_the_fused_call():
    c = C.build_fused("n257_h4_it7000_rand_extra")
    out = T.run_fused(c, DEV)
    cams = P.cameras_from_pose(out["pose"].detach(), C.Z_OFFSET, C.FOV, offset_extra=c["offset_extra"])
    for k, t in zip(T.CAMERA_KEYS, cams):
        assert _same_bits(t, out[k].detach()), k


@pytest.mark.parametrize("name", list(C.RANDOM_VIEW_CASES))
def test_random_view_against_float64_with_rand_degree_on_the_host_and_on_the_device(name):
    c = C.build_random_view(name)
    out = T.run_random_view(c, DEV)
    _check(out, R.evaluate_random_view(c), f"random_view/{name}")
    host = T.run_random_view(c, DEV, degree_device="cpu")
    gold = np.load(os.path.join(T.GOLDEN, "pose_random_view.npz"))
    for k in T.CAMERA_KEYS:
        assert _same_bits(out[k], host[k]) and not out[k].requires_grad, k
        assert np.abs(out[k].cpu().numpy() - gold[f"{name}/{k}"]).max() <= 1e-5, k  # (a coarse net under the bounds)
    assert _same_bits(out["w2c"].cpu(), torch.from_numpy(gold[name + "/w2c"]))


def test_sizes_the_kernels_refuse_take_the_torch_statement_and_device_false_too():
    c = C.build_fused("n3_h4_it7000_rand")
    H = L.POSE_MAX_HYPOS + 1
    with L.KernelTimer() as timer:
        out = P.predict_cameras(torch.randn(2, 4 * H + 3, device=DEV), 7000, orthant_signs=torch.ones(H, 3), max_trans_xyz_range=c["max_trans"],
                                cam_pos_z_offset=10.0, fov=25.0, num_hypos=H)
        assert timer.summary() == {}
    assert out[0].is_cuda and out[0].shape == (2, 4 * H + 3)
    with pytest.raises(ValueError):
        ops.predict_cameras(torch.randn(2, 4 * H + 3, device=DEV), torch.ones(H, 3, device=DEV), c["max_trans"].to(DEV), None, None, False, False, 1.0,
                            0.0, 2, -10.0, P._proj16(25.0, 0.1, 1000.0))
    on = T.run_fused(c, DEV)
    P.DEVICE = False
    try:
        with L.KernelTimer() as timer:
            off = T.run_fused(c, DEV)
            cams = P.cameras_from_pose(on["pose"].detach(), C.Z_OFFSET, C.FOV)
            assert timer.summary() == {}
    finally:
        P.DEVICE = True
    assert off["pose"].is_cuda and cams[0].is_cuda
    for k in on:
        if not k.startswith("_"):
            assert torch.allclose(on[k].float(), off[k].float(), rtol=1e-5, atol=1e-5), k


def test_argument_validation_raises_before_any_launch():
    c = C.build_fused("n3_h4_it7000_rand")
    raw = c["raw"].to(DEV)
    kw = T._kwargs(c, DEV)
    with L.KernelTimer() as timer:
        for bad in (lambda: P.predict_cameras(raw[:, :18], 7000, **kw), lambda: P.predict_cameras(raw, 7000, **dict(kw, num_hypos=8)),
                    lambda: P.predict_cameras(raw, 7000, **dict(kw, rand_perm=kw["rand_perm"][:2])), lambda: P.cameras_from_pose(raw, 10.0, 25.0),
                    lambda: P.random_view_cameras(torch.zeros(3, 4, 4, device=DEV), torch.zeros(3, device=DEV), 25.0)):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(L.A3DError):
            ops.cameras_from_pose(torch.zeros(3, 12), -10.0, P._proj16(25.0, 0.1, 1000.0))
        assert timer.summary() == {}
