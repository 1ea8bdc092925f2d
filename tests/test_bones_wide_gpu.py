"""estimate_bones on the GPU for more than 32 instances: the multi-work-group path of a3d_estimate_bones (csrc/bones_wide.hip) through
skinning.estimate_bones, against the torch restatement it replaces there (itself pinned by the reference's goldens) and against a
golden of the reference.  Inputs: tests/bones_wide_cases.py (checked on the CPU by tests/test_bones_wide_cpu.py: none sits on a
rounding edge).  The torch results are computed once per input and shared."""
import functools
import importlib

import numpy as np
import pytest
import torch

import bones_wide_cases as C
from conftest import golden

pytestmark = pytest.mark.gpu
L = importlib.import_module("3danimals_amd._lib")
sk = importlib.import_module("3danimals_amd.model.geometry.skinning")
TOL = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def run(seq, mode, thr, n_leg, **switches):
    """Chain rebuilt, then chain cached, with the module switches set as given -> (bones, chain, aux, cached bones, calls by entry point)."""
    kw = dict(n_leg_bones=n_leg, body_bones_mode=mode, bone_y_threshold=thr, **C.KW)
    saved = {k: getattr(sk, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(sk, k, v)
        with L.KernelTimer() as timer:
            bones, chain, aux = sk.estimate_bones(seq.clone(), compute_kinematic_chain=True, **kw)
            again = sk.estimate_bones(seq.clone(), compute_kinematic_chain=False, aux=aux, **kw)
        return bones, chain, aux, again, timer.summary()
    finally:
        for k, v in saved.items():
            setattr(sk, k, v)


@functools.lru_cache(maxsize=None)
def torch_statements(maker, args, mode, thr, n_leg):
    """The torch restatement on the GPU (DEVICE_ESTIMATE_BONES off), once per input."""
    return run(getattr(C, maker)(*args).cuda(), mode, thr, n_leg, DEVICE_ESTIMATE_BONES=False)


def assert_equal_to_torch(maker, args, mode, thr, n_leg):
    seq = getattr(C, maker)(*args).cuda()
    b_k, chain_k, aux_k, again_k, calls_k = run(seq, mode, thr, n_leg, DEVICE_ESTIMATE_BONES=True, DEVICE_ESTIMATE_BONES_WIDE=True)
    b_t, chain_t, aux_t, again_t, calls_t = torch_statements(maker, args, mode, thr, n_leg)
    assert calls_k.get("a3d_estimate_bones", (0,))[0] == 2 and "a3d_estimate_bones" not in calls_t  # the kernels ran: no fall-back
    assert b_k.shape == b_t.shape == (*seq.shape[:2], 8 + 4 * n_leg, 2, 3)
    print("max |kernel - torch|", float((b_k - b_t).abs().max()), float((again_k - again_t).abs().max()))
    assert float((b_k - b_t).abs().max()) <= TOL and float((again_k - again_t).abs().max()) <= TOL
    assert torch.equal(again_k, b_k)  # chain cached == chain rebuilt, bit for bit: also two calls on one input
    assert repr(chain_k) == repr(chain_t) and aux_k["bones_to_joints"] == aux_t["bones_to_joints"]
    if n_leg:
        assert [l["body_bone_idx"] for l in aux_k["legs"]] == [l["body_bone_idx"] for l in aux_t["legs"]]
    L.poll_deferred()  # (every quadrant holds a vertex: nothing pending raises)
    return b_k


@pytest.mark.parametrize("n_leg", [3, 0])
@pytest.mark.parametrize("mode,thr", C.MODES)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_wide_kernels_equal_the_torch_restatement(shape, mode, thr, n_leg, dev):
    """Bones within 1e-6, the same chain and attachment joints, cached == rebuilt and call == call bit for bit, and a3d_estimate_bones
    counted twice where the parent commit fell back to ~245 torch launches per call."""
    b = assert_equal_to_torch("base", shape, mode, thr, n_leg)
    again = run(C.base(*shape).cuda(), mode, thr, n_leg)[0]
    assert torch.equal(again, b)


def test_switch_sends_wide_calls_back_to_the_torch_statements(dev):
    seq = C.base(3, 11).cuda()
    *_, calls = run(seq, "z_minmax_y+", None, 3, DEVICE_ESTIMATE_BONES=True, DEVICE_ESTIMATE_BONES_WIDE=False)
    assert "a3d_estimate_bones" not in calls
    *_, calls = run(seq[:2], "z_minmax_y+", None, 3, DEVICE_ESTIMATE_BONES=True, DEVICE_ESTIMATE_BONES_WIDE=False)
    assert calls["a3d_estimate_bones"][0] == 2  # 22 instances: the one work-group, whatever the switch says
    L.poll_deferred()


@pytest.mark.parametrize("V", C.EDGE_V)
def test_slab_and_wave_edges(V, dev):
    """33 instances of V vertices around the sizes at which a wave, a work-group's trip and a slab fill up; spine only below 65 vertices,
    with legs (both quadrant rules) from there on."""
    for mode, thr in (C.MODES[1:] if V >= 65 else C.MODES[:2]):
        assert_equal_to_torch("cloud", (C.N_EDGE, V), mode, thr, 3 if V >= 65 else 0)


@pytest.mark.parametrize("mode,thr", C.MODES)
def test_ties_between_work_groups_go_to_the_first_index(mode, thr, dev):
    """Two vertices with the largest z, two with the smallest, two lowest ones in a quadrant, the members of a pair in different slabs
    and different in their other coordinates: a wrong winner moves a bone by 0.1 or more."""
    seq = C.ties()
    for name, (a, b) in C.TIE_PAIRS.items():
        assert a // C.SLAB != b // C.SLAB and float((seq[0, 0, a] - seq[0, 0, b]).abs().max()) >= 0.1, name
    assert float(seq[..., 2].max()) == float(seq[0, 0, C.TIE_PAIRS["z_max"][1], 2]) and float(seq[..., 1].min()) == float(seq[0, 0, C.TIE_PAIRS["foot0"][1], 1])
    assert_equal_to_torch("ties", (), mode, thr, 3)


def test_empty_quadrant_travels_as_a_deferred_check(dev):
    """One instance of 33 without a vertex in its -x quadrants: ``ok`` is cleared and the reference's message is raised at the next poll."""
    seq = C.empty(3, 11, 17).cuda()
    L.poll_deferred()
    with L.KernelTimer() as timer:
        bones = sk.estimate_bones(seq, n_leg_bones=3, body_bones_mode="z_minmax_y+", compute_kinematic_chain=True,
                                  legs_to_body_joint_indices=[2, 7, 7, 2], **C.KW)[0]
    assert timer.summary()["a3d_estimate_bones"][0] == 1 and torch.isfinite(bones).all()
    with pytest.raises(L.A3DError, match="no vertex in a leg quadrant"):
        L.poll_deferred()


@pytest.mark.parametrize("thr", [None, 0.4])
def test_cached_chain_runs_without_host_synchronisation(thr, dev):
    kw = dict(n_leg_bones=3, body_bones_mode="z_minmax_y+", bone_y_threshold=thr, **C.KW)
    seq = C.base(5, 8).cuda()
    bones, _, aux = sk.estimate_bones(seq.clone(), compute_kinematic_chain=True, **kw)
    L.poll_deferred()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with L.KernelTimer() as timer:
            cached = sk.estimate_bones(seq, compute_kinematic_chain=False, aux=aux, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert timer.summary()["a3d_estimate_bones"][0] == 1 and torch.equal(cached, bones)
    L.poll_deferred()


@pytest.mark.parametrize("tag,thr", [("default", None), ("fauna", 0.4)])
def test_wide_kernels_against_the_reference_golden(tag, thr, dev):
    g = golden("bones_wide.npz")
    B, F = (int(v) for v in g["shape"])
    with L.KernelTimer() as timer:
        bones, chain, aux = sk.estimate_bones(C.base(B, F).cuda(), n_leg_bones=3, body_bones_mode="z_minmax_y+", bone_y_threshold=thr, **C.KW)
    assert timer.summary()["a3d_estimate_bones"][0] == 1
    print("max |kernel - reference|", float(np.abs(bones.cpu().numpy() - g[f"{tag}_bones"]).max()))
    np.testing.assert_allclose(bones.cpu().numpy(), g[f"{tag}_bones"], atol=TOL)
    assert repr(chain) == str(g[f"{tag}_chain"]) and [l["body_bone_idx"] for l in aux["legs"]] == list(g[f"{tag}_leg_body_idx"])
    L.poll_deferred()
