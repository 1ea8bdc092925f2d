"""The mesh regularisers without a GPU: the entry points of include/a3d_reg.h, argument validation before any launch, the restatement's edge tables against the reference's recorded ones, the module's
torch statements against the reference's goldens (float32) and against the restatement (float64, values and gradients), and known
answers of the corrected Laplacian."""
import importlib
import math
import os
import sys

import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check as A  # noqa: E402
import regularizer_cases as C  # noqa: E402
import regularizer_ref as R  # noqa: E402

ENTRIES = ("a3d_edge_topology", "a3d_reg_partials", "a3d_laplace_fwd", "a3d_laplace_bwd", "a3d_normal_consistency_fwd",
           "a3d_normal_consistency_bwd", "a3d_edge_length_fwd", "a3d_edge_length_bwd")
FAKE = 0x1000  # non-NULL, never dereferenced


def _L():
    return importlib.import_module("3danimals_amd._lib")


def _M():
    return importlib.import_module("3danimals_amd.model.render.regularizer")


def test_fifth_header_matches_the_fifth_table_and_the_other_surfaces_are_untouched():
    """What is this surface's own (tests/test_abi_cpu.py holds every surface's table and constants to its header)."""
    protos = A.prototypes("a3d_reg.h")
    assert set(protos) == set(ENTRIES)
    assert protos["a3d_reg_partials"][0] == "size_t" and len(protos["a3d_normal_consistency_bwd"][1]) == 15
    overlay = importlib.import_module("3danimals_amd.overlay")
    assert len(overlay.MODULES) == 9 and not any("regularizer" in str(m) for m in overlay.MODULES)  # imported directly
    assert _M().HIP_REGULARIZERS is True


def test_entry_points_refuse_invalid_arguments_before_anything_is_launched():
    """None of the pointers below is ever dereferenced and nothing is launched (this runs without a GPU)."""
    lib = _L().lib()
    sizes = dict(B=2, V=5, F=4)
    good = {
        "a3d_edge_topology": dict(tri=FAKE, F=4, V=5, off=FAKE, adj=FAKE, ls=0, table=FAKE, ne=FAKE),
        "a3d_laplace_fwd": dict(v=FAKE, tri=FAKE, off=FAKE, adj=FAKE, ls=0, **sizes, scaled=FAKE, part=FAKE, loss=FAKE),
        "a3d_laplace_bwd": dict(g=FAKE, scaled=FAKE, tri=FAKE, off=FAKE, adj=FAKE, ls=0, **sizes, gv=FAKE),
        "a3d_normal_consistency_fwd": dict(v=FAKE, tri=FAKE, table=FAKE, ne=FAKE, **sizes, stand=FAKE, part=FAKE, loss=FAKE),
        "a3d_normal_consistency_bwd": dict(g=FAKE, v=FAKE, tri=FAKE, table=FAKE, ne=FAKE, off=FAKE, adj=FAKE, ls=0, stand=FAKE, **sizes,
                                           scratch=FAKE, gv=FAKE),
        "a3d_edge_length_fwd": dict(v=FAKE, tri=FAKE, table=FAKE, ne=FAKE, **sizes, part=FAKE, loss=FAKE),
        "a3d_edge_length_bwd": dict(g=FAKE, v=FAKE, tri=FAKE, table=FAKE, ne=FAKE, off=FAKE, adj=FAKE, ls=0, **sizes, gv=FAKE),
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
        for key in ("B", "V", "F"):
            if key in args:
                refused(name, **{key: 0})
                refused(name, **{key: -3})
        if "B" in args:
            refused(name, B=65536)
        if "ls" in args:
            refused(name, ls=-1)
        refused(name, F=(1 << 31) // 3 + 1)
    assert lib.a3d_reg_partials(0, 5) == 0 and lib.a3d_reg_partials(2, 0) == 0
    assert lib.a3d_reg_partials(2, 100) == 4 * 2 * 2 and lib.a3d_reg_partials(3, 256) == 4 * 3 * 3


@pytest.mark.parametrize("name", C.NAMES)
def test_restated_edge_tables_equal_the_reference_tables(name):
    g = golden("regularizer.npz")
    edges, cols = C.tables(name)
    assert torch.equal(edges, torch.from_numpy(g[f"{name}_edges"]).long()), name
    assert torch.equal(cols, torch.from_numpy(g[f"{name}_tris_per_edge"]).long()), name
    # ... and the module's own helpers on the CPU (torch's sequential index put) give the same
    mesh = importlib.import_module("3danimals_amd.model.render.mesh")
    tri = C.make_case(name)["faces"][None]
    assert torch.equal(mesh.compute_edges(tri), edges) and torch.equal(mesh.compute_edge_to_face_mapping(tri), cols)
    if name == "nonmanifold":  # the case is what it says: a duplicate in column 0 decided by the last write, empty second columns
        e = {tuple(k): tuple(c) for k, c in zip(edges.tolist(), cols.tolist())}
        assert e[(0, 1)] == (1, 2) and e[(1, 2)] == (3, 0) and e[(0, 2)] == (0, 0)
    if name == "fan":
        assert int(((cols[:, 1] == 0) & (cols[:, 0] != 0)).sum()) >= 69  # rim edges paired with face 0
    if name == "repeated":
        assert [3, 3] in edges.tolist()  # the self edge


@pytest.mark.parametrize("name", C.NAMES)
def test_torch_statements_reproduce_the_reference_goldens(name):
    """float32 on the CPU: the recorded float32 evaluation to 8 ulp (a mean over up to 2 x 1920 terms, another CPU's vector width)."""
    M = _M()
    g = golden("regularizer.npz")
    case = C.make_case(name)
    v_pos, tri = case["v_pos"], case["faces"][None]
    for fn, key in ((M.normal_consistency, "nc32"), (M.avg_edge_length, "ael32"), (M.get_edge_length, "gel32")):
        got, want = fn(v_pos, tri), torch.from_numpy(g[f"{name}_{key}"])
        assert got.shape == want.shape and got.dtype == torch.float32
        assert float((got - want).abs().max()) <= 8 * 2.0 ** -24 * float(want.abs().max()), (name, key)


@pytest.mark.parametrize("name", C.NAMES)
def test_torch_statements_match_the_restatement_in_float64(name):
    """Values and gradients to 1e-12 relative (to the tensor's largest magnitude), the corrected Laplacian included."""
    M = _M()
    case = C.make_case(name)
    v64, tri = case["v_pos"].double(), case["faces"][None]
    for loss, fn in zip(C.LOSS_NAMES, (M.laplace_regularizer_const, M.normal_consistency, M.avg_edge_length)):
        val, grad = C.value_and_grad(lambda v: fn(v, tri), v64)
        want_val, want_grad = C.x64(name, loss)
        assert val.dtype == torch.float64 and abs(float(val - want_val)) <= 1e-12 * abs(float(want_val)), (name, loss)
        assert float((grad - want_grad).abs().max()) <= 1e-12 * float(want_grad.abs().max()), (name, loss)
    assert torch.equal(M.get_edge_length(v64, tri), R.get_edge_length(v64, case["faces"], C.tables(name)))


def test_the_corrected_laplacian_satisfies_known_answers():
    # the centre of a regular planar hexagon: the umbrella term vanishes there
    ang = torch.arange(6, dtype=torch.float64) * (math.pi / 3)
    hexagon = torch.cat([torch.zeros(1, 3, dtype=torch.float64), torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros(6, dtype=torch.float64)], -1)])[None]
    tri = torch.tensor([[0, 1 + i, 1 + (i + 1) % 6] for i in range(6)])
    term = R.laplace_term(hexagon, tri)
    assert float(term[0, 0].abs().max()) <= 1e-15 and float(term[0, 1:].abs().min(0).values.max()) > 0.1
    assert torch.allclose(term, R.laplace_term_loops(hexagon, tri), rtol=0, atol=1e-15)
    # rim vertex 1 has two corner entries: ((v2 - v1) + (v0 - v1) + (v0 - v1) + (v6 - v1)) / 4
    want = ((hexagon[0, 2] - hexagon[0, 1]) + 2 * (hexagon[0, 0] - hexagon[0, 1]) + (hexagon[0, 6] - hexagon[0, 1])) / 4
    assert torch.allclose(term[0, 1], want, rtol=0, atol=1e-15)
    # the isolated vertex contributes 0, value and gradient, and does not change the other vertices' terms
    case = C.make_case("mesh_isolated")
    iso = C.isolated_vertices(case)
    assert int(iso.sum()) == 1
    v64 = case["v_pos"].double()
    term = R.laplace_term(v64, case["faces"])
    assert float(term[:, iso].abs().max()) == 0.0
    assert float(C.x64("mesh_isolated", "laplace")[1][:, iso].abs().max()) == 0.0
    # a face that lists a vertex twice counts twice: vertex 3 of 'repeated' has three corner entries
    rep = C.make_case("repeated")
    v64 = rep["v_pos"].double()
    loops = R.laplace_term_loops(v64, rep["faces"])
    assert torch.allclose(R.laplace_term(v64, rep["faces"]), loops, rtol=0, atol=1e-14)
    want3 = ((v64[:, 2] - v64[:, 3]) + (v64[:, 1] - v64[:, 3]) + 2 * (v64[:, 4] - v64[:, 3])) / 6
    assert torch.allclose(loops[:, 3], want3, rtol=0, atol=1e-14)
    # the module's corrected statements: autograd's gradient equals the restatement's, and the reference's index shape is what raises
    M = _M()
    tri3 = rep["faces"][None]
    val, grad = C.value_and_grad(lambda v: M.laplace_regularizer_const(v, tri3), v64)
    want_val, want_grad = C.x64("repeated", "laplace")
    assert abs(float(val - want_val)) <= 1e-12 * float(want_val) and float((grad - want_grad).abs().max()) <= 1e-12 * float(want_grad.abs().max())
    norm = torch.zeros(2, 7, 1, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="Expected index"):
        norm.scatter_add_(1, tri3[..., 0:1].repeat(2, 1, 3), torch.ones(2, 4, 3, dtype=torch.float64))
