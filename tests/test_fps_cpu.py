"""Farthest-point sampling (csrc/fps.hip, the resample tail of a3d_estimate_bones) without a GPU: the float64 reference of the GPU tests
against a golden of the reference project, the equality clouds' gaps, the tail packed by ops.py against its C definition, what the
entry point refuses before it launches, and the CPU path of estimate_bones(resample=True)."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import abi_check as A
import fps_cases as C
import fps_ref as R
from conftest import golden

L = importlib.import_module("3danimals_amd._lib")
sk = importlib.import_module("3danimals_amd.model.geometry.skinning")
util = importlib.import_module("3danimals_amd.model.geometry.util")
ops = importlib.import_module("3danimals_amd.ops")
MACROS = A.defines("a3d.h")
A3D_EINVAL = MACROS["A3D_EINVAL"]
PUBLIC = ctypes.sizeof(L.EstimateBonesArgs)


def golden_inputs():
    out = {name: (C.cloud(V, seed)[None], [start]) for name, (V, seed, start) in C.EQUALITY.items()}
    out["lattice"] = (C.lattice()[None], [C.LATTICE_START])
    q = C.quadruped()
    out["quadruped"] = (q.reshape(-1, q.shape[2], 3), list(C.QUADRUPED_START))
    return out


@pytest.mark.parametrize("name", list(C.EQUALITY) + ["lattice", "quadruped"])
def test_float64_reference_reproduces_the_reference_golden(name):
    """The reference project's float32 loop (recorded by golden/make_fps_golden.py) picks what the float64 greedy run with the
    lowest-index rule picks -- on the lattice, where every distance is exact and ties are everywhere, that IS the tie rule."""
    want = golden("fps_reference.npz")[name]
    pts, start = golden_inputs()[name]
    assert want.shape[0] == pts.shape[0]
    for n in range(pts.shape[0]):
        picks, _ = R.greedy(pts[n].numpy(), want.shape[1], start[n])
        assert np.array_equal(picks, want[n]), (name, n, int(np.argmax(picks != want[n])))
    if name == "lattice":
        assert float(C.lattice().max()) < 64 and C.lattice().shape == (240, 3) and sorted(want[0].tolist()) == list(range(240))


@pytest.mark.parametrize("name", list(C.EQUALITY))
def test_equality_clouds_leave_rounding_no_say(name):
    V, seed, start = C.EQUALITY[name]
    _, gaps = R.greedy(C.cloud(V, seed).numpy(), V, start)
    print(name, "smallest relative gap", gaps.min(), "bound", C.GAP_BOUND)
    assert V <= 1025 and gaps.min() >= C.GAP_BOUND


def test_shortfall_of_a_greedy_run_is_zero_and_of_a_wrong_pick_is_not():
    pts = C.cloud(300, 3000).numpy()
    picks, _ = R.greedy(pts, 75, 160)
    assert R.pick_shortfall(pts, picks).max() == 0.0
    picks[40] = picks[3]  # a point already picked: distance 0
    assert R.pick_shortfall(pts, picks)[40] == 1.0


# ---- the tail: ops.py's packing against csrc/eb_common.h, through the registered mirror (tests/test_abi_cpu.py holds it to the header too)
def test_tail_packing_matches_the_c_definition():
    fields = A.struct_fields("a3d_eb_fps_tail")
    mirror = type("Tail", (ctypes.Structure,), {"_fields_": fields})  # (built from the header: the packed block is read back with it)
    assert fields == L.EbFpsTail._fields_
    assert ctypes.sizeof(mirror) == ctypes.sizeof(L.EbFpsTail) == ops.FPS_TAIL_SIZE == MACROS["A3D_FPS_TAIL_SIZE"]
    assert MACROS["A3D_FPS_MAX_V"] == ops.FPS_MAX_V >= 131072 and MACROS["A3D_FPS_REG_MAX_V"] == ops.FPS_REG_MAX_V
    # the header's byte table
    text = open(os.path.join(A.INCLUDE, "a3d.h")).read()
    table = {name: int(off) for off, name in re.findall(r"\*\s+byte\s+(\d+)\s+(?:const )?\w+\*? (\w+)", text)}
    assert table == {n: getattr(mirror, n).offset for n, _ in fields}, table
    # a packed block, field by field
    a = L.EstimateBonesArgs(N=3, V=50, pos=0x1000, n_body=8)
    values = dict(k=12, sample_only=1, start=0x2000, sampled=0x3000, idx=0x4000)
    block = ops.pack_fps_block(a, **values)
    assert ctypes.sizeof(block) == PUBLIC + ops.FPS_TAIL_SIZE and ctypes.addressof(block) % 8 == 0
    head = L.EstimateBonesArgs.from_buffer_copy(bytes(block)[:PUBLIC])
    assert head.size == PUBLIC + ops.FPS_TAIL_SIZE and (head.N, head.V, head.pos, head.n_body) == (3, 50, 0x1000, 8)
    tail = mirror.from_buffer_copy(bytes(block)[PUBLIC:])
    assert {n: getattr(tail, n) for n in values} == values
    block = ops.pack_fps_block(a, 5, False, 0x2000, 0x3000, None)
    tail = mirror.from_buffer_copy(bytes(block)[PUBLIC:])
    assert (tail.k, tail.sample_only, tail.idx) == (5, 0, None)
    assert "typedef struct" not in text[text.index("The resample tail"):text.index("#define A3D_FPS_TAIL_SIZE")]


def _public(N=2, V=400, workspace=0x1000, **kw):
    """Arguments that never reach a kernel: the pointers are made-up addresses (every call below is refused by the validation)."""
    a = L.EstimateBonesArgs(N=N, pos=0x1000, bones=0x1000, nearest=0x1000, ok=0x1000, V=V, workspace=workspace, n_body=8, n_leg=3,
                            body_mode_y_plus=1)
    for i in range(4):
        a.attach[i] = -1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refused(block, needle):
    assert L.lib().a3d_estimate_bones(ctypes.addressof(block), None) == A3D_EINVAL, needle
    msg = L.lib().a3d_last_error()
    assert b"a3d_estimate_bones: invalid argument" in msg and needle in msg, (needle, msg)


@pytest.mark.parametrize("what,public,tail,needle", [
    ("k = 0", {}, dict(k=0), b"tail->k >= 1"),
    ("k > V", {}, dict(k=401), b"tail->k <= args->V"),
    ("null start", {}, dict(start=None), b"tail->start"),
    ("null sampled", {}, dict(sampled=None), b"tail->sampled"),
    ("V over the limit", dict(V=131073), {}, b"A3D_FPS_MAX_V"),
    ("more points than the bones path takes", dict(N=1 << 8, V=(1 << 16) + 1), {}, b"A3D_EB_WIDE_MAX_POINTS"),
    ("workspace regime without a workspace", dict(V=16385, workspace=None), dict(sample_only=1), b"A3D_FPS_REG_MAX_V"),
    ("null pos", dict(pos=None), {}, b"args->pos"),
    ("sampled bones without their buffers", dict(bones=None), {}, b"args->bones"),
    ("sampled bones, odd n_body", dict(n_body=7), {}, b"n_body"),
])
def test_entry_point_refuses_a_bad_tail_before_any_launch(what, public, tail, needle):
    values = dict(k=100, sample_only=0, start=0x2000, sampled=0x3000, idx=None)
    values.update(tail)
    _refused(ops.pack_fps_block(_public(**public), **values), needle)


def test_entry_point_refuses_a_size_between_the_two_sizes():
    for extra in (4, 8, ops.FPS_TAIL_SIZE - 8, ops.FPS_TAIL_SIZE - 1):
        block = ops.pack_fps_block(_public(), 100, 0, 0x2000, 0x3000, None)
        ctypes.cast(block, ctypes.POINTER(ctypes.c_uint32))[0] = PUBLIC + extra
        _refused(block, b"sizeof(a3d_eb_fps_tail)")


def test_public_size_and_tail_size_pass_the_size_checks():
    """A call of the public size is taken as before, and one with the tail is taken too: each gets as far as a LATER check (n_body
    must be even), which names what it refuses.  (Nothing may be launched here: the addresses are made up.)"""
    a = _public(n_body=7)
    a.size = PUBLIC
    _refused(a, b"n_body % 2 == 0")
    _refused(ops.pack_fps_block(_public(n_body=7), 100, 0, 0x2000, 0x3000, 0x4000), b"n_body % 2 == 0")
    sample_only = ops.pack_fps_block(_public(n_body=7, bones=None, nearest=None, ok=None), 0, 1, 0x2000, 0x3000, 0x4000)
    _refused(sample_only, b"tail->k >= 1")  # (a sample-only call does not look at the bones' arguments)


def test_cpu_tensors_keep_the_torch_loop(monkeypatch):
    """estimate_bones(resample=True) on CPU tensors: the reference's picks (the golden), and the bones of exactly those points."""
    want = golden("fps_reference.npz")["quadruped"]
    seq = C.quadruped()
    monkeypatch.setattr(torch, "randint", lambda n, shape, device=None: torch.tensor(C.QUADRUPED_START, dtype=torch.int64))
    pts = seq.reshape(-1, seq.shape[2], 3).transpose(1, 2)
    out, idx = util.sample_farthest_points(pts, seq.shape[2] // 4, return_index=True)
    assert np.array_equal(idx.numpy(), want) and torch.equal(out, pts.gather(2, idx[:, None, :].expand(-1, 3, -1)))
    kw = dict(n_body_bones=8, n_legs=4, n_leg_bones=3, body_bones_mode="z_minmax_y+")
    bones, chain, aux = sk.estimate_bones(seq.clone(), resample=True, **kw)
    picked = seq.gather(2, torch.from_numpy(want).reshape(1, 2, -1, 1).expand(-1, -1, -1, 3))
    assert torch.equal(picked, out.transpose(1, 2).reshape(1, 2, -1, 3))
    bones_p, chain_p, aux_p = sk.estimate_bones(out.transpose(1, 2).reshape(1, 2, -1, 3), **kw)  # (the layout estimate_bones itself makes)
    assert torch.equal(bones, bones_p) and repr(chain) == repr(chain_p) and repr(aux) == repr(aux_p)


def test_switch_and_limits_are_declared():
    assert isinstance(sk.DEVICE_FPS, bool)
    assert not ops.fps_device_ok(torch.zeros(2, 10, 3), 3)  # CPU tensors never go to the kernel
    with pytest.raises(L.A3DError):
        ops.farthest_point_sample(torch.zeros(2, 10, 3), 3, torch.zeros(2, dtype=torch.int64))
