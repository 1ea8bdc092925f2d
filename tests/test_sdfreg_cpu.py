"""The SDF sign-agreement regulariser without a GPU: the entry points of include/a3d_sdfreg.h, argument validation before any launch, the module's torch statements against the reference's goldens (float32,
bit for bit) and against the float64 restatement (tests/sdfreg_ref.py), the routing of sdf_bce_reg_loss, and the builder of the
vertex -> (edge, side) list the backward kernel walks."""
import importlib
import math
import os
import sys

import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check as A  # noqa: E402
import sdfreg_cases as C  # noqa: E402

ENTRIES = ("a3d_sdf_bce_fwd", "a3d_sdf_bce_bwd")
FAKE = 0x1000  # non-NULL, 16-byte aligned, never dereferenced


def _L():
    return importlib.import_module("3danimals_amd._lib")


def _M():
    return importlib.import_module("3danimals_amd.model.geometry.dmtet")


def _ops():
    return importlib.import_module("3danimals_amd.ops")


def test_seventh_header_matches_the_seventh_table_and_the_other_surfaces_are_untouched():
    """What is this surface's own (tests/test_abi_cpu.py holds every surface's table and constants to its header)."""
    protos = A.prototypes("a3d_sdfreg.h")
    assert set(protos) == set(ENTRIES)
    assert len(protos["a3d_sdf_bce_fwd"][1]) == 8 and len(protos["a3d_sdf_bce_bwd"][1]) == 10 and protos["a3d_sdf_bce_fwd"][1][1] == "int"
    assert "dmtet.py:161-169" in open(os.path.join(A.INCLUDE, "a3d_sdfreg.h")).read()  # the reference lines are cited
    overlay = importlib.import_module("3danimals_amd.overlay")
    assert "model.geometry.dmtet" in overlay.MODULES and "sdf_bce_reg_loss" in overlay.exported_names("model.geometry.dmtet")
    assert _M().HIP_SDF_REG is True


def test_entry_points_refuse_invalid_arguments_before_anything_is_launched():
    """None of the pointers below is ever dereferenced and nothing is launched (this runs without a GPU)."""
    lib = _L().lib()
    good = {
        "a3d_sdf_bce_fwd": dict(sdf=FAKE, Nv=5, edges=FAKE, Ne=7, part=FAKE, state=FAKE, loss=FAKE),
        "a3d_sdf_bce_bwd": dict(g=FAKE, sdf=FAKE, Nv=5, edges=FAKE, Ne=7, off=FAKE, inc=FAKE, state=FAKE, gsdf=FAKE),
    }

    def refused(name, **bad):
        args = dict(good[name], **bad)
        assert getattr(lib, name)(*args.values(), None) == -1, (name, bad)
        msg = lib.a3d_last_error().decode()
        assert "invalid argument" in msg and name in msg, (name, msg)

    for name, args in good.items():
        for key, val in args.items():
            if val == FAKE:
                refused(name, **{key: None})  # every pointer is required
        for key in ("Nv", "Ne"):
            refused(name, **{key: 0})
            refused(name, **{key: -3})
        refused(name, Ne=1 << 30)  # 2 Ne entries of the incidence list are indexed with an int
    refused("a3d_sdf_bce_fwd", edges=FAKE + 8)  # the rows are read with 16-byte loads
    refused("a3d_sdf_bce_fwd", part=FAKE + 4)


@pytest.mark.parametrize("name", C.FINITE)
def test_torch_statements_reproduce_the_reference_goldens_bit_for_bit(name):
    M, g = _M(), golden("sdfreg.npz")
    case = C.make_case(name)
    val, grad = C.twin32(name)
    assert val.dtype == torch.float32 and val.dim() == 0
    assert torch.equal(val, torch.from_numpy(g[f"{name}_loss32"])), (name, float(val))
    if f"{name}_grad32" in g:
        assert torch.equal(grad, torch.from_numpy(g[f"{name}_grad32"])), name
    else:
        assert name == "kuhn34"
    col_val, col_grad = C.value_and_grad(lambda s: M.sdf_bce_reg_loss(s, case["edges"]), case["sdf"][:, None])  # the public name on the CPU
    assert torch.equal(col_val, val) and col_grad.shape == (case["sdf"].shape[0], 1) and torch.equal(col_grad[:, 0], grad)


@pytest.mark.parametrize("name", C.FINITE)
def test_torch_statements_match_the_restatement_in_float64(name):
    """Values and gradients to 1e-12 relative (to the tensor's largest magnitude); the crossing rows are the restatement's."""
    M = _M()
    case = C.make_case(name)
    want_val, want_grad, mask = C.x64(name)
    val, grad = C.value_and_grad(lambda s: M.sdf_bce_reg_loss(s, case["edges"]), case["sdf"].double())
    assert val.dtype == torch.float64 and abs(float(val) - want_val) <= 1e-12 * abs(want_val), (name, float(val), want_val)
    assert float((grad - want_grad).abs().max()) <= 1e-12 * float(want_grad.abs().max()), name
    pair = case["sdf"][case["edges"]]
    assert torch.equal(torch.sign(pair[:, 0]) != torch.sign(pair[:, 1]), mask)
    if name in C.COUNTS:
        assert (case["sdf"].shape[0], case["edges"].shape[0], int(mask.sum())) == C.COUNTS[name]


def test_the_cases_are_what_they_say():
    # the crossing rule on the hand-made rows: (0, -1), (0, 1) cross, (0, 0) and (0, -0) and a self edge do not, duplicates count
    case, (_, grad, mask) = C.make_case("zeros"), C.x64("zeros")
    rows = {tuple(r): bool(m) for r, m in zip(case["edges"].tolist(), mask.tolist())}
    assert rows[(0, 2)] and rows[(2, 0)] and rows[(0, 3)] and rows[(3, 0)] and rows[(1, 4)] and rows[(5, 1)] and rows[(2, 3)] and rows[(3, 2)]
    assert not (rows[(0, 0)] or rows[(0, 1)] or rows[(1, 0)] or rows[(2, 2)] or rows[(3, 3)] or rows[(1, 1)] or rows[(2, 4)] or rows[(3, 5)])
    assert case["edges"].tolist().count([2, 3]) == 3 and int(mask.sum()) == 14
    # M == 0: nan and an all-zero gradient, from the statements too
    val, grad = C.twin32("none_cross")
    assert math.isnan(float(val)) and float(grad.abs().max()) == 0.0 and math.isnan(C.x64("none_cross")[0])
    # no overflow at large magnitudes: the issue's (80, -80), (200, -200) give 280
    M = _M()
    assert float(M.sdf_bce_reg_loss(torch.tensor([80.0, -80.0, 200.0, -200.0]), torch.tensor([[0, 1], [2, 3]]))) == 280.0
    val, grad = C.twin32("large")
    assert math.isfinite(float(val)) and bool(torch.isfinite(grad).all())
    # torch.sign(nan) is 0: a NaN crosses a non-zero end only
    case = C.make_case("nonfinite")
    pair = case["sdf"][case["edges"]]
    mask = (torch.sign(pair[:, 0]) != torch.sign(pair[:, 1])).tolist()
    rows = dict(zip(map(tuple, case["edges"].tolist()), mask))
    assert rows[(0, 3)] and rows[(4, 0)] and not rows[(0, 6)] and not rows[(0, 5)] and not rows[(6, 6)]
    assert C.value_class(C.twin32("nonfinite")[1]).tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0] and math.isnan(float(C.twin32("nonfinite")[0]))
    assert float(C.twin32("posinf")[0]) == float("inf") and bool(torch.isfinite(C.twin32("posinf")[1]).all())
    assert -(-C.make_case("kuhn34")["edges"].shape[0] // _L().SDF_BCE_BLOCK_EDGES) > 256  # more partials than the finishing work-group has threads


def test_cpu_float64_and_switched_off_inputs_take_the_torch_statements(monkeypatch):
    M, ops = _M(), _ops()
    calls = []
    monkeypatch.setattr(ops, "sdf_bce_reg_loss", lambda *a: calls.append(a) or torch.zeros(()))
    case = C.make_case("kuhn2")
    sdf, edges = case["sdf"], case["edges"]
    want = M._sdf_bce_reg_loss_torch(sdf, edges)
    assert torch.equal(M.sdf_bce_reg_loss(sdf, edges), want)  # a CPU tensor
    assert M.sdf_bce_reg_loss(sdf.double(), edges).dtype == torch.float64  # float64

    class OnGpu:  # what _sdf_reg_hip_ok looks at, without a GPU
        def __init__(self, t, device="cuda:0"):
            self.t, self.is_cuda, self.dtype, self.shape, self.device = t, True, t.dtype, t.shape, device

        def dim(self):
            return self.t.dim()

    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, OnGpu)))
    assert M._sdf_reg_hip_ok(OnGpu(sdf), OnGpu(edges)) and M._sdf_reg_hip_ok(OnGpu(sdf[:, None]), OnGpu(edges.int()))
    assert not M._sdf_reg_hip_ok(OnGpu(sdf.double()), OnGpu(edges))
    assert not M._sdf_reg_hip_ok(OnGpu(sdf[:, None].expand(-1, 2)), OnGpu(edges)) and not M._sdf_reg_hip_ok(OnGpu(sdf[None]), OnGpu(edges))
    assert not M._sdf_reg_hip_ok(OnGpu(sdf), OnGpu(edges.float())) and not M._sdf_reg_hip_ok(OnGpu(sdf), OnGpu(edges.reshape(-1)))
    assert not M._sdf_reg_hip_ok(OnGpu(sdf), OnGpu(edges, "cuda:1")) and not M._sdf_reg_hip_ok(OnGpu(sdf), OnGpu(edges[:0]))
    monkeypatch.setattr(M, "HIP_SDF_REG", False)
    assert not M._sdf_reg_hip_ok(OnGpu(sdf), OnGpu(edges))
    assert not calls


@pytest.mark.parametrize("name", ("zeros", "kuhn4"))
def test_incidence_list_holds_every_edge_side_once_under_its_vertex(name):
    ops = _ops()
    case = C.make_case(name)
    edges32, nv = case["edges"].int(), case["sdf"].shape[0]
    off, inc = ops.edge_incidence(edges32, nv)
    assert off.dtype == inc.dtype == torch.int32 and off.shape == (nv + 1,) and inc.shape == (2 * edges32.shape[0],)
    assert int(off[0]) == 0 and int(off[-1]) == inc.shape[0] and bool((off[1:] >= off[:-1]).all())
    assert sorted(inc.tolist()) == list(range(inc.shape[0]))  # every (edge, side) exactly once
    flat = edges32.reshape(-1)
    for v in range(nv):
        mine = inc[int(off[v]):int(off[v + 1])].tolist()
        assert mine == sorted(mine) and all(int(flat[i]) == v for i in mine), v  # under its vertex, in list order
    cached = ops.SdfEdges(edges32)
    assert (cached.lo, cached.hi) == (int(edges32.min()), int(edges32.max())) and cached.edges32.data_ptr() % 16 == 0
    cached.check(nv)
    with pytest.raises(IndexError, match="sdf_bce_reg_loss"):
        cached.check(nv - 1)
    with pytest.raises(IndexError):
        ops.SdfEdges(edges32 - 1).check(nv)
    again = cached.incidence(nv)
    assert again[0] is cached.incidence(nv)[0] and torch.equal(again[1], inc)  # built once
