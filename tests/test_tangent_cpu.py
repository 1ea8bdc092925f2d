"""The tangent frame without a GPU: the entry points of include/a3d_tangent.h and the op code of ops.py, argument validation before any launch, the repository's torch statements and the tests' float64 restatement
against the reference's recorded goldens, and the share of pixels the kink mask leaves out on the committed inputs."""
import ctypes
import importlib
import os
import sys

import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check as A  # noqa: E402
import tangent_cases as C  # noqa: E402
import tangent_ref as R  # noqa: E402

ENTRIES = ("a3d_shading_normal_rows", "a3d_shading_normal_fwd", "a3d_shading_normal_bwd", "a3d_tangents_fwd", "a3d_tangents_bwd")
FAKE = 0x1000  # non-NULL, never dereferenced


def _L():
    return importlib.import_module("3danimals_amd._lib")


def _ru():
    return importlib.import_module("3danimals_amd.model.render.renderutils")


def test_fourth_header_matches_the_fourth_table_and_the_other_surfaces_are_untouched():
    """What is this surface's own (tests/test_abi_cpu.py holds every surface's table and constants to its header)."""
    L = _L()
    protos = A.prototypes("a3d_tangent.h")
    assert set(protos) == set(ENTRIES)
    assert protos["a3d_shading_normal_rows"][0] == "int64" and len(protos["a3d_tangents_bwd"][1]) == 17
    assert L.SHADING_NORMAL_OP == 5 and "A3D_SHADING_NORMAL" not in open(os.path.join(A.INCLUDE, "a3d_bsdf.h")).read()
    ops = importlib.import_module("3danimals_amd.ops")
    assert ops.TANGENT_OPS["shading_normal"] == (5, (3,) * 6, 3) and "shading_normal" not in ops.BSDF_OPS


def _desc(L, **kw):
    d = L.BsdfDesc(size=ctypes.sizeof(L.BsdfDesc), op=5, variant=3, ndim=1, seg=8, out=FAKE, g_out=FAKE)
    d.shape[0] = 8
    for i in range(6):
        getattr(d, "in")[i] = FAKE
        d.stride[4 * i] = 3
        d.cstride[i] = 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_shading_normal_refuses_an_invalid_descriptor_before_anything_is_launched():
    """None of the pointers below is ever dereferenced and nothing is launched (this runs without a GPU)."""
    L = _L()
    lib = L.lib()

    def refused(name, d, *words):
        assert getattr(lib, name)(ctypes.byref(d), None) == -1, name
        msg = lib.a3d_last_error().decode()
        assert "invalid argument" in msg and name in msg and all(w in msg for w in words), (name, msg)

    for name in ("a3d_shading_normal_fwd", "a3d_shading_normal_bwd"):
        refused(name, _desc(L, size=ctypes.sizeof(L.BsdfDesc) - 4), "size")
        for op in (3, 4, 6, 17, -1):  # the BSDF codes belong to a3d_bsdf_*
            refused(name, _desc(L, op=op), "op")
        refused(name, _desc(L, variant=4), "variant")
        refused(name, _desc(L, variant=-1), "variant")
        refused(name, _desc(L, ndim=0), "ndim")
        refused(name, _desc(L, ndim=5), "ndim")
        d = _desc(L)
        d.shape[0] = -8
        refused(name, d, "shape")
        refused(name, _desc(L, seg=3), "seg")  # does not divide the pixel count
        refused(name, _desc(L, seg=0), "seg")
        d = _desc(L)
        d.stride[4] = -3
        refused(name, d, "stride")
        for i in range(6):
            d = _desc(L)
            getattr(d, "in")[i] = None
            refused(name, d, "in[%d]" % i)
        assert getattr(lib, name)(None, None) == -1
    refused("a3d_shading_normal_fwd", _desc(L, out=None), "out")
    refused("a3d_shading_normal_bwd", _desc(L, g_out=None), "g_out")
    d = _desc(L)
    d.g_mode[2] = 3
    refused("a3d_shading_normal_bwd", d, "gmode")
    d = _desc(L)
    d.g_mode[0] = 1  # a wanted gradient without a buffer
    refused("a3d_shading_normal_bwd", d, "g_in")
    d = _desc(L)  # a reduced gradient of an input that is NOT constant over the run
    d.g_mode[1], d.seg_div[1], d.g_in[1], d.g_final[1] = 2, 1, FAKE, FAKE
    refused("a3d_shading_normal_bwd", d, "in[1]", "REDUCE", "constant over")
    # the old surface refuses the new code (it was not loosened), the new rows function has a3d_bsdf_rows' rule
    assert lib.a3d_bsdf_fwd(ctypes.byref(_desc(L)), None) == -1 and "op" in lib.a3d_last_error().decode()
    assert lib.a3d_shading_normal_rows(ctypes.byref(_desc(L, size=8))) == -1 and lib.a3d_shading_normal_rows(ctypes.byref(_desc(L, seg=3))) == -1
    assert lib.a3d_shading_normal_rows(ctypes.byref(_desc(L, op=3))) == -1
    d = _desc(L, ndim=2, seg=3000)
    d.shape[0], d.shape[1] = 5, 3000
    assert lib.a3d_shading_normal_rows(ctypes.byref(d)) == 5 * 3 == lib.a3d_bsdf_rows(ctypes.byref(d))
    d = _desc(L)  # zero pixels: accepted, nothing to do
    d.shape[0] = 0
    assert lib.a3d_shading_normal_fwd(ctypes.byref(d), None) == 0


def test_tangents_refuse_invalid_arguments_before_anything_is_launched():
    L = _L()
    lib = L.lib()
    good_f = dict(v_pos=FAKE, v_tex=FAKE, ts=0, v_nrm=FAKE, tri=FAKE, ttri=FAKE, off=FAKE, adj=FAKE, ls=0, B=2, V=5, F=4, out=FAKE)
    good_b = dict(g=FAKE, v_pos=FAKE, v_tex=FAKE, ts=0, v_nrm=FAKE, tri=FAKE, ttri=FAKE, off=FAKE, adj=FAKE, ls=0, B=2, V=5, F=4, scratch=FAKE,
                  g_pos=FAKE, g_nrm=FAKE)

    def refused(name, good, **bad):
        args = dict(good, **bad)
        assert getattr(lib, name)(*args.values(), None) == -1, (name, bad)
        msg = lib.a3d_last_error().decode()
        assert "invalid argument" in msg and name in msg, (name, msg)

    for name, good in (("a3d_tangents_fwd", good_f), ("a3d_tangents_bwd", good_b)):
        for key, val in good.items():
            if val == FAKE:
                refused(name, good, **{key: None})  # every pointer is required
        for key in ("B", "V", "F"):
            refused(name, good, **{key: 0})
            refused(name, good, **{key: -3})
        refused(name, good, B=65536)
        refused(name, good, ls=-1)
        refused(name, good, ts=-2)


@pytest.mark.parametrize("kind,two_sided,opengl,seed", C.SN_GOLDEN_CASES)
def test_torch_statements_and_restatement_reproduce_the_shading_normal_goldens(kind, two_sided, opengl, seed):
    """Values and gradients to rounding: 1e-12 relative to the tensor's largest magnitude in float64; the float32 statements are the
    recorded float32 evaluation (4 ulp of the largest magnitude for another CPU's vector width)."""
    g = golden(f"tangent_sn_{kind}_{int(two_sided)}{int(opengl)}.npz")
    built = C.make_sn_inputs(kind, C.GOLDEN_PIXELS, seed, opengl)
    for i in range(6):
        assert torch.equal(torch.from_numpy(g[f"in_{i}"]), built[i]), (kind, i)
    g_out = torch.from_numpy(g["g_out"])
    fns = {"statements": lambda *a: _ru().prepare_shading_normal(*a, two_sided_shading=two_sided, opengl=opengl, use_python=True),
           "restatement": lambda *a: R.shading_normal(*a, two_sided, opengl)}
    for what, fn in fns.items():
        xs = [t.double().requires_grad_(True) for t in built]
        out = fn(*xs)
        want = torch.from_numpy(g["out64"])
        assert out.shape == want.shape and out.dtype == torch.float64
        assert float((out.detach() - want).abs().max()) <= 1e-12 * float(want.abs().max()), (what, kind)
        for i, gi in enumerate(torch.autograd.grad(out, xs, g_out.double())):
            w = torch.from_numpy(g[f"g64_{i}"])
            assert gi.shape == w.shape and float((gi - w).abs().max()) <= 1e-12 * max(float(w.abs().max()), 1e-300), (what, kind, i)
    x32 = [t.clone().requires_grad_(True) for t in built]
    o32 = fns["statements"](*x32)
    g32 = torch.autograd.grad(o32, x32, g_out)
    for got, key in [(o32.detach(), "out32")] + [(gi, f"g32_{i}") for i, gi in enumerate(g32)]:
        w = torch.from_numpy(g[key])
        assert float((got - w).abs().max()) <= 4 * 2.0 ** -24 * float(w.abs().max()), (kind, key)
    # without a GPU (and for float64) use_python=False runs the same statements
    assert torch.equal(_ru().prepare_shading_normal(*built, two_sided_shading=two_sided, opengl=opengl), o32.detach())


def test_the_kink_mask_leaves_out_no_more_than_the_cap():
    """The committed inputs and the seeds the GPU tests generate from: the share of pixels within 1e-5 of a kink, in float64."""
    for kind, two_sided, opengl, seed in C.SN_GOLDEN_CASES:
        share = float(C.sn_near_kink(C.make_sn_inputs(kind, C.GOLDEN_PIXELS, seed, opengl), two_sided, opengl).double().mean())
        assert share <= (0.0 if kind == "cond" else C.KINK_CAP), (kind, two_sided, opengl, share)
    for two_sided, opengl in C.VARIANTS:
        for n, seed in ((1025, 31), (3109, 32), (105, 33), (128, 34)):
            for kind in ("cond", "wild"):
                share = float(C.sn_near_kink(C.make_sn_inputs(kind, n, seed, opengl), two_sided, opengl).double().mean())
                assert share <= (0.0 if kind == "cond" else C.KINK_CAP), (kind, n, seed, share)
    # 'bcast' keeps the bend's ramp live for most pixels: view_pos receives a gradient there
    pos, view_pos, per, nrm, tng, geo = [t.double() for t in C.make_sn_inputs("bcast", 512, 120)]
    view = torch.nn.functional.normalize(view_pos - pos, dim=-1)
    d = (view * C.perturbed_normal(per, nrm, tng, True)).sum(-1) / 0.1
    assert float(((d > 0.05) & (d < 0.95)).double().mean()) >= 0.9


def _mesh_module():
    return importlib.import_module("3danimals_amd.model.render.mesh")


@pytest.mark.parametrize("name", C.MESH_NAMES)
def test_torch_statements_and_restatement_reproduce_the_tangent_goldens(name):
    """float64: 1e-11 of the largest magnitude (the DMTet atlas makes the sums cancel: a few more ulps than element-wise work).  The
    isolated vertex is NaN in the same places."""
    M = _mesh_module()
    g = golden("tangent_meshes.npz")
    case = C.make_mesh_case(name)
    B = case["v_pos"].shape[0]
    keep = ~C.isolated_vertices(case)
    w = C.mesh_weights(case).double()

    def statements(v_pos, v_nrm):
        m = M.Mesh(v_pos, case["faces"][None], v_nrm, case["faces"][None], case["v_tex"].to(v_pos.dtype).expand(B, -1, -1), case["uv_idx"][None])
        return M._tangents(m)

    restated = lambda v_pos, v_nrm: R.vertex_tangents(v_pos, case["v_tex"].to(v_pos.dtype), v_nrm, case["faces"], case["uv_idx"])
    for what, fn in (("statements", statements), ("restatement", restated)):
        v_pos, v_nrm = (case[k].double().requires_grad_(True) for k in ("v_pos", "v_nrm"))
        tng = fn(v_pos, v_nrm)
        want = torch.from_numpy(g[f"{name}_tng64"])
        assert torch.equal(torch.isnan(tng), torch.isnan(want)) and bool(torch.isnan(want[:, ~keep]).all()) and not bool(torch.isnan(want[:, keep]).any())
        assert float((tng.detach() - want)[:, keep].abs().max()) <= 1e-11, (what, name)
        gs = torch.autograd.grad((tng[:, keep] * w[:, keep]).sum(), [v_pos, v_nrm])
        for gi, key in zip(gs, ("gpos64", "gnrm64")):
            wg = torch.from_numpy(g[f"{name}_{key}"])
            assert torch.equal(torch.isnan(gi), torch.isnan(wg))
            assert float((gi - wg)[:, keep].abs().max()) <= 1e-11 * float(wg[:, keep].abs().max()), (what, name, key)
    if name in ("mesh_b1", "mesh_b4"):  # the atlas restated in tangent_cases is the one the committed v_tng was recorded with
        t32 = statements(case["v_pos"], case["v_nrm"])
        assert float((t32 - torch.from_numpy(golden(name + ".npz")["v_tng"])).abs().max()) <= 5e-5
    if name == "degenerate":  # the branches are what the case says they are
        uv = case["v_tex"][0][case["uv_idx"]]
        e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
        denom = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        assert int((denom == 0).sum()) == 2 and int((denom < 0).sum()) == 1
    if name == "fan":
        assert int((case["faces"] == 0).sum()) == C.FAN_RIM == 70
