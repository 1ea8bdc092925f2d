"""compute_tangents on the GPU (csrc/tangent.hip) through Mesh.v_tng / ops.vertex_tangents.

Values and both gradients against the float64 restatement (tests/tangent_ref.py, held to the reference's goldens by
tests/test_tangent_cpu.py) by the parity rule bsdf_cases.parity, with the float32 torch statements of mesh._tangents as the twin.
"""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bsdf_cases as BC  # noqa: E402
import tangent_cases as C  # noqa: E402
import tangent_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _M():
    return importlib.import_module("3danimals_amd.model.render.mesh")


def _ops():
    return importlib.import_module("3danimals_amd.ops")


def _mesh(case, device, v_pos=None, v_nrm=None, v_tex=None, t_nrm_idx=None):
    M = _M()
    B = case["v_pos"].shape[0]
    faces = case["faces"].to(device)[None]
    v_pos = case["v_pos"].to(device) if v_pos is None else v_pos
    v_nrm = case["v_nrm"].to(device) if v_nrm is None else v_nrm
    v_tex = case["v_tex"].to(device).expand(B, -1, -1) if v_tex is None else v_tex  # (a stride-0 view for a shared atlas, as Mesh._expand_uv)
    m = M.Mesh(v_pos, faces, v_nrm, faces if t_nrm_idx is None else t_nrm_idx, v_tex, case["uv_idx"].to(device)[None])
    return M.compute_tangents(m)


def _run(case, device, hip=True, **kw):
    """(v_tng, g_v_pos, g_v_nrm) on the CPU; the isolated vertex takes no part in the loss."""
    M = _M()
    keep = ~C.isolated_vertices(case)
    w = C.mesh_weights(case)
    v_pos, v_nrm = (case[k].to(device).requires_grad_(True) for k in ("v_pos", "v_nrm"))
    prev, M.HIP_TANGENTS = M.HIP_TANGENTS, hip
    try:
        tng = _mesh(case, device, v_pos, v_nrm, **kw).v_tng
    finally:
        M.HIP_TANGENTS = prev
    gs = torch.autograd.grad((tng[:, keep] * w.to(device)[:, keep]).sum(), [v_pos, v_nrm])
    return tng.detach().cpu(), gs[0].cpu(), gs[1].cpu()


def _x64(case):
    keep = ~C.isolated_vertices(case)
    v_pos, v_nrm = (case[k].double().requires_grad_(True) for k in ("v_pos", "v_nrm"))
    tng = R.vertex_tangents(v_pos, case["v_tex"].double(), v_nrm, case["faces"], case["uv_idx"])
    gs = torch.autograd.grad((tng[:, keep] * C.mesh_weights(case).double()[:, keep]).sum(), [v_pos, v_nrm])
    return tng.detach(), gs[0], gs[1]


@pytest.mark.parametrize("name", C.MESH_NAMES)
def test_parity_with_the_float64_restatement(name):
    """The committed DMTet meshes (every face its own uv cell: huge face tangents that cancel), a tetrahedron (V = 4, F = 4, an atlas per
    image), a fan whose hub has valence 70 with B = 3, and a mesh with two degenerate uv triangles and a mirrored one."""
    case = C.make_mesh_case(name)
    keep = ~C.isolated_vertices(case)
    hip, twin, x64 = _run(case, "cuda"), _run(case, "cpu"), _x64(case)
    vmask = keep[None].expand(case["v_pos"].shape[:2])
    for what, h, t, x in zip(("v_tng", "g_v_pos", "g_v_nrm"), hip, twin, x64):
        assert h.shape == x.shape and h.dtype == torch.float32
        assert torch.equal(torch.isnan(h), torch.isnan(t)), (name, what)  # the NaN pattern of the isolated vertex is the statements'
        assert not bool(torch.isnan(h[:, keep]).any())
        h, t, x = (u.clone() for u in (h, t, x))
        for u in (h, t, x):  # (compared above; parity's scale is a median over the whole tensor, which a NaN would poison)
            u[:, ~keep] = 0
        BC.parity(f"{name} {what}", h, t, x, vmask)
    if name == "mesh_isolated":
        assert bool(torch.isnan(hip[0][:, ~keep]).all()) and bool(torch.isnan(hip[2][:, ~keep]).all()) and float(hip[1][:, ~keep].abs().max()) == 0.0
    if name in ("mesh_b1", "mesh_b4"):  # the reference's own float32 result, the tolerance of tests/test_gpu_parity.py
        np.testing.assert_allclose(hip[0].numpy(), golden(name + ".npz")["v_tng"], atol=5e-5)
    if name == "mesh_isolated":
        ref32 = golden("tangent_meshes.npz")["mesh_isolated_tng32"]
        np.testing.assert_allclose(hip[0][:, keep].numpy(), ref32[:, keep.numpy()], atol=5e-5)
    again = _run(case, "cuda")  # both passes bit-reproducible
    assert all(torch.equal(a[:, keep], b[:, keep]) for a, b in zip(hip, again))


def test_the_kernel_is_what_ran():
    """Mesh.v_tng of a CUDA float32 mesh goes through a3d_tangents_fwd / _bwd; with the switch off, through neither."""
    L = importlib.import_module("3danimals_amd._lib")
    case = C.make_mesh_case("tetra")
    for hip in (True, False):
        with L.KernelTimer() as timer:
            _run(case, "cuda", hip=hip)
        names = [n.split("[")[0] for n in timer.summary() if "tangents" in n]
        assert names == (["a3d_tangents_fwd", "a3d_tangents_bwd"] if hip else []), names


def test_shared_atlas_as_a_stride_0_view_equals_the_repeated_atlas():
    case = C.make_mesh_case("fan")
    B = case["v_pos"].shape[0]
    shared = case["v_tex"].cuda().expand(B, -1, -1)
    assert shared.stride(0) == 0
    a = _run(case, "cuda", v_tex=shared)
    b = _run(case, "cuda", v_tex=case["v_tex"].cuda().repeat(B, 1, 1))
    c = _run(case, "cuda", v_tex=case["v_tex"].cuda())  # [1,Nuv,2] itself
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))
    assert shared.stride(0) == 0 and shared.data_ptr() == shared[1].data_ptr()  # still a view


def test_out_of_scope_meshes_fall_back_and_still_match():
    """An atlas that wants a gradient, or normals with an index list of their own, take the torch statements."""
    L = importlib.import_module("3danimals_amd._lib")
    M = _M()
    case = C.make_mesh_case("degenerate")
    B = case["v_pos"].shape[0]
    want = _run(case, "cuda")
    uv = case["v_tex"].cuda().expand(B, -1, -1).clone().requires_grad_(True)
    with L.KernelTimer() as timer:
        m = _mesh(case, "cuda", v_tex=uv)
        tng = m.v_tng
        (g_uv,) = torch.autograd.grad(tng.sum(), uv)
    assert not [n for n in timer.summary() if "tangents" in n] and float(g_uv.abs().max()) > 0
    assert float((tng.detach().cpu() - want[0]).abs().max()) <= 5e-5
    # the same indices in another tensor are still in scope; other indices are not
    faces = case["faces"].cuda()[None]
    with L.KernelTimer() as timer:
        same = _mesh(case, "cuda", t_nrm_idx=faces.clone()).v_tng
    assert [n for n in timer.summary() if "tangents" in n] and torch.equal(same.cpu(), want[0])
    other = faces.clone()
    other[0, 0] = other[0, 0].flip(0)  # the first face's normals in another order: tangents land on the same vertices, but it is another list
    with L.KernelTimer() as timer:
        fell = _mesh(case, "cuda", t_nrm_idx=other).v_tng
    assert not [n for n in timer.summary() if "tangents" in n]
    ref = R.vertex_tangents(case["v_pos"].double(), case["v_tex"].double(), case["v_nrm"].double(), case["faces"], case["uv_idx"], other[0].cpu())
    assert float((fell.cpu() - ref).abs().max()) <= 5e-5
    with pytest.raises(ValueError, match="v_tex receives no gradient"):
        _ops().vertex_tangents(case["v_pos"].cuda(), uv, case["v_nrm"].cuda(), faces, case["uv_idx"].cuda())
    assert M.HIP_TANGENTS is True


def test_tangent_render_mode_equals_the_render_with_the_switch_off():
    """render_mesh(..., render_modes=['tangent']) of the mesh_b4 scene at 32 x 32: the interpolated tangents of both paths within 5e-5."""
    M = _M()
    render = importlib.import_module("3danimals_amd.model.render.render")
    case = C.make_mesh_case("mesh_b4")
    dev = torch.device("cuda")
    B = case["v_pos"].shape[0]
    mvp = torch.diag(torch.tensor([0.25, 0.25, 0.1, 1.0]))[None].repeat(B, 1, 1).to(dev)
    w2c = torch.eye(4)[None].repeat(B, 1, 1).to(dev)
    campos = torch.tensor([0.0, 0.0, -10.0]).repeat(B, 1).to(dev)
    outs = []
    for hip in (True, False):
        prev, M.HIP_TANGENTS = M.HIP_TANGENTS, hip
        try:
            mesh = M.make_mesh(case["v_pos"].to(dev), case["faces"].to(dev)[None], case["v_tex"].to(dev).expand(B, -1, -1),
                               case["uv_idx"].to(dev)[None], None)
            prior = M.make_mesh(case["v_pos"][:1].to(dev), case["faces"].to(dev)[None], case["v_tex"].to(dev), case["uv_idx"].to(dev)[None], None)
            with torch.no_grad():
                out = render.render_mesh(None, mesh, mvp, w2c, campos, None, None, (32, 32), spp=1, num_layers=1, msaa=False,
                                         background=torch.zeros(B, 32, 32, 3, device=dev), bsdf="diffuse", render_modes=["tangent"],
                                         prior_mesh=prior)
        finally:
            M.HIP_TANGENTS = prev
        outs.append(out[0].cpu())
    assert outs[0].shape[0] == B and outs[0].shape[-2:] == (32, 32)
    covered = (outs[1][:, :3] != 0).any(1)
    assert float(covered.float().mean()) > 0.02  # the mesh is in view
    assert float((outs[0] - outs[1]).abs().max()) <= 5e-5
