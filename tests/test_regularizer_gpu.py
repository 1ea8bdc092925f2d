"""The mesh regularisers on the GPU (csrc/regularizer.hip) through model/render/regularizer.py and ops.

Loss values against the float64 restatement (tests/regularizer_ref.py, held to the reference's recorded tables and float32 results by
tests/test_regularizer_cpu.py): |hip - x64| <= 2^-23 |x64| -- the kernels carry terms and sums in double and round once to float32
(at most 2^-24 relative), with a factor 2 over that.  Against the reference's float32 golden the bound follows from the triangle
inequality.  Gradients by the parity rule bsdf_cases.parity with the module's float32 torch statements on the CPU as the twin.
"""
import functools
import importlib
import os
import sys

import pytest
import torch

from conftest import golden, kuhn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bsdf_cases as BC  # noqa: E402
import regularizer_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu

FUNCTIONS = {"laplace": "laplace_regularizer_const", "normal_consistency": "normal_consistency", "avg_edge_length": "avg_edge_length"}
GOLDEN_KEYS = {"normal_consistency": "nc32", "avg_edge_length": "ael32"}
ENTRIES = {"laplace": ["a3d_laplace_fwd", "a3d_laplace_bwd"], "normal_consistency": ["a3d_normal_consistency_fwd", "a3d_normal_consistency_bwd"],
           "avg_edge_length": ["a3d_edge_length_fwd", "a3d_edge_length_bwd"]}
NEW = {"a3d_edge_topology"} | {n for names in ENTRIES.values() for n in names}


def _M():
    return importlib.import_module("3danimals_amd.model.render.regularizer")


def _ops():
    return importlib.import_module("3danimals_amd.ops")


def _L():
    return importlib.import_module("3danimals_amd._lib")


def _extraction():
    """the marching-tets mesh of the 'emit_lists' case extracted on the GPU now: (faces int64 [F,3] as the extraction returns them, the
    vertex -> face lists it left in the cache)"""
    dmtet = importlib.import_module("3danimals_amd.model.geometry.dmtet")
    g = golden(C.EMIT_FIXTURE)
    pos, tets = kuhn(int(g["res"]))
    with torch.no_grad():
        _, faces, _, _ = dmtet.DMTet()(pos.cuda(), torch.from_numpy(g["sdf"]).cuda()[:, None], tets.cuda())
    assert torch.equal(faces.cpu(), C.make_case("emit_lists")["faces"])
    lists = _ops()._adj_cache.peek(_ops().tri_int32(faces))
    return faces, lists


@functools.lru_cache(maxsize=None)
def _tri(name):
    """[1,F,3] on the GPU, one tensor per case: the topology of a case is built once"""
    if name == "emit_lists":
        return _extraction()[0][None]
    return C.make_case(name)["faces"].cuda()[None]


def _run(name, loss, hip=True, device="cuda", tri=None):
    M = _M()
    if tri is None:
        tri = _tri(name) if device == "cuda" else C.make_case(name)["faces"][None]
    fn = getattr(M, FUNCTIONS[loss])
    prev, M.HIP_REGULARIZERS = M.HIP_REGULARIZERS, hip
    try:
        return C.value_and_grad(lambda v: fn(v, tri), C.make_case(name)["v_pos"].to(device))
    finally:
        M.HIP_REGULARIZERS = prev


@functools.lru_cache(maxsize=None)
def _twin32(name, loss):
    return _run(name, loss, device="cpu")


@pytest.mark.parametrize("loss", C.LOSS_NAMES)
@pytest.mark.parametrize("name", C.NAMES)
def test_parity_with_the_float64_restatement(name, loss):
    case = C.make_case(name)
    val, grad = _run(name, loss)
    x_val, x_grad = C.x64(name, loss)
    t_val, t_grad = _twin32(name, loss)
    assert val.dtype == torch.float32 and val.dim() == 0 and grad.dtype == torch.float32 and grad.shape == case["v_pos"].shape
    err = abs(float(val.double() - x_val))
    print(f"{name} {loss}: hip {float(val):.9g} x64 {float(x_val):.17g} |hip - x64| / |x64| = {err / abs(float(x_val)):.3e} (twin32 {abs(float(t_val.double() - x_val)) / abs(float(x_val)):.3e})")
    assert err <= 2.0 ** -23 * abs(float(x_val)), (name, loss, float(val), float(x_val))
    if loss in GOLDEN_KEYS:  # the reference's own float32 result
        ref = float(golden("regularizer.npz")[f"{name}_{GOLDEN_KEYS[loss]}"])
        assert abs(float(val) - ref) <= abs(ref - float(x_val)) + 2.0 ** -23 * abs(float(x_val)), (name, loss, float(val), ref)
    BC.parity(f"{name} {loss} g_v_pos", grad, t_grad, x_grad)
    iso = C.isolated_vertices(case)
    if bool(iso.any()):
        assert float(grad[:, iso].abs().max()) == 0.0
    again_val, again_grad = _run(name, loss)
    assert torch.equal(again_val, val) and torch.equal(again_grad, grad)


def test_the_kernels_are_what_ran_and_the_edge_table_is_built_once():
    L, ops = _L(), _ops()
    tri = C.make_case("degenerate")["faces"].cuda()[None]  # a fresh tensor: nothing cached for it
    ops.vertex_face_adjacency(ops.tri_int32(tri), C.make_case("degenerate")["v_pos"].shape[1])
    for hip in (True, False):
        with L.KernelTimer() as timer:
            for _ in range(2):
                for loss in C.LOSS_NAMES:
                    _run("degenerate", loss, hip=hip, tri=tri)
        summary = {n.split("[")[0]: launches for n, (launches, _) in timer.summary().items()}
        if hip:
            assert set(summary) == NEW, set(summary) ^ NEW
            assert summary["a3d_edge_topology"] == 1 and all(summary[n] == 2 for n in NEW - {"a3d_edge_topology"}), summary
        else:
            assert not set(summary) & NEW, summary
    assert _M().HIP_REGULARIZERS is True


def _sync_debug_mode_works():
    """whether this torch build reports a host synchronisation under set_sync_debug_mode('error') on this device"""
    probe = torch.ones(1, device="cuda")
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    return False


def test_a_cached_topology_call_does_not_synchronise_with_the_host():
    if not _sync_debug_mode_works():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not report a .item() on this torch build / device")
    M = _M()
    tri = _tri("mesh_b4")
    v = C.make_case("mesh_b4")["v_pos"].cuda().requires_grad_(True)
    for loss in C.LOSS_NAMES:  # build and cache every topology first
        getattr(M, FUNCTIONS[loss])(v, tri)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        results = []
        for loss in C.LOSS_NAMES:
            out = getattr(M, FUNCTIONS[loss])(v, tri)
            results.append((out, torch.autograd.grad(out, v)[0]))
        M.HIP_REGULARIZERS = False
        with pytest.raises(RuntimeError):  # torch.unique reads its output size back
            M.avg_edge_length(v, tri)
    finally:
        M.HIP_REGULARIZERS = True
        torch.cuda.set_sync_debug_mode(prev)
    for loss, (out, grad) in zip(C.LOSS_NAMES, results):
        want_val, want_grad = _run("mesh_b4", loss)
        assert torch.equal(out.detach().cpu(), want_val) and torch.equal(grad.cpu(), want_grad)


def test_fixed_stride_lists_and_csr_lists_give_the_same_bits():
    ops = _ops()
    faces, lists = _extraction()
    assert lists is not None and lists.stride > 0  # the emit launch's own lists
    fresh = faces.clone()[None]
    for loss in C.LOSS_NAMES:
        a, b = _run("emit_lists", loss, tri=faces[None]), _run("emit_lists", loss, tri=fresh)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), loss
    assert ops._adj_cache.peek(ops.tri_int32(fresh)).stride == 0
    assert ops._edge_cache.peek(ops.tri_int32(faces)).adjacency is lists
    # the edge table itself does not depend on the list form, and it is the restatement's
    t_a, t_b = ops._edge_cache.peek(ops.tri_int32(faces)), ops._edge_cache.peek(ops.tri_int32(fresh))
    assert torch.equal(t_a.table, t_b.table) and int(t_a.num_edges) == int(t_b.num_edges) == C.tables("emit_lists")[0].shape[0]


@pytest.mark.parametrize("name", ("nonmanifold", "repeated", "fan"))
def test_the_edge_table_is_the_restatement(name):
    """representatives = unique edges; each representative's face and partner are the restatement's two columns"""
    L, ops = _L(), _ops()
    tri = ops.tri_int32(_tri(name))
    topo = ops.edge_topology(tri, C.make_case(name)["v_pos"].shape[1])
    table, faces = topo.table.cpu(), C.make_case(name)["faces"]
    edges, cols = C.tables(name)
    want = {tuple(e): tuple(c) for e, c in zip(edges.tolist(), cols.tolist())}
    assert int(topo.num_edges) == len(want)
    got = {}
    for s in (table[:, 0] & L.EDGE_REPRESENTATIVE).nonzero().flatten().tolist():
        f, c = divmod(s, 3)
        i, j = int(faces[f, c]), int(faces[f, (c + 1) % 3])
        assert int(table[s, 0]) & L.EDGE_WINNER
        if int(table[s, 0]) & L.EDGE_STAND_IN:
            assert int(table[s, 1]) == 0
        got[(min(i, j), max(i, j))] = (f, int(table[s, 1])) if i <= j else (int(table[s, 1]), f)
    assert got == want


def test_empty_inputs_return_what_the_torch_statements_return():
    M = _M()
    tri = _tri("tetra")
    none = torch.zeros((1, 0, 3), dtype=torch.int64, device="cuda")
    for loss in C.LOSS_NAMES:
        fn = getattr(M, FUNCTIONS[loss])
        for v, t in ((torch.rand(2, 5, 3), none), (torch.rand(0, 4, 3), tri)):  # F == 0, B == 0
            want = fn(v, t.cpu())  # the torch statements
            x = v.cuda().requires_grad_(True)
            got = fn(x, t)
            assert got.dtype == torch.float32 and got.dim() == 0
            assert torch.equal(torch.isnan(got.cpu()), torch.isnan(want)) and (bool(torch.isnan(want)) or float(got.detach()) == float(want)), (loss, got, want)
            (g,) = torch.autograd.grad(got, x)  # the graph is connected
            assert g.shape == x.shape


def test_float64_input_takes_the_torch_statements_and_wrong_inputs_raise():
    L, M, ops = _L(), _M(), _ops()
    tri = _tri("tetra")
    v64 = C.make_case("tetra")["v_pos"].double().cuda()
    with L.KernelTimer() as timer:
        for loss in C.LOSS_NAMES:
            val, grad = C.value_and_grad(lambda v: getattr(M, FUNCTIONS[loss])(v, tri), v64)
            want_val, want_grad = C.x64("tetra", loss)
            assert val.dtype == torch.float64 and abs(float(val - want_val)) <= 1e-12 * abs(float(want_val))
            assert float((grad - want_grad).abs().max()) <= 1e-12 * float(want_grad.abs().max())
    assert not {n.split("[")[0] for n in timer.summary()} & NEW
    v = C.make_case("tetra")["v_pos"].cuda()
    for fn in (ops.laplace_regularizer, ops.normal_consistency, ops.avg_edge_length):
        for bad_v, bad_t in ((v.double(), tri), (v.half(), tri), (v[0], tri), (v[..., :2], tri), (v, tri.float()), (v, tri[..., :2]),
                             (v, tri.expand(2, -1, -1))):
            with pytest.raises(ValueError, match=fn.__name__):
                fn(bad_v, bad_t)
        with pytest.raises(L.A3DError):
            fn(v.cpu(), tri)
