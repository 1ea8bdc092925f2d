"""'depth' / 'tangent' on the fused render path, the parts that need no GPU: tests/depth_ref.py against the package's generic shade(),
the layout of the struct that carries the depth source, and the refusals of the entry point (which come before any launch: the pointers
below are never dereferenced)."""
import ctypes
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_ref  # noqa: E402
from conftest import seeded  # noqa: E402

L = importlib.import_module("3danimals_amd._lib")
FAKE = 0x1000  # non-NULL, never dereferenced


@pytest.mark.parametrize("B,H,W,shared", [(2, 6, 5, False), (3, 4, 7, True)])
def test_depth_ref_is_the_generic_shade_on_cpu_tensors(B, H, W, shared):
    """shade(..., render_modes=['depth']) of this package is the port of the reference's lines (render.py:101-108); depth_ref states them
    once more for float64.  Same statements: in float32 they agree to the last bits (bound: 4 ulp of a value in [0,1] -- two
    evaluations of the same expression may differ in how the matmul sums its four products), and float64 differs from float32 by the
    rounding of z over the range: |z| <= 4 here, range >= 1, so 2^-23 x 4 x a few operations, asserted as 1e-5."""
    R = importlib.import_module("3danimals_amd.model.render.render")
    pos = seeded((B, H, W, 3), 1, -1, 1)
    cover = seeded((B, H, W), 2, 0, 1) > 0.4
    pos = pos * cover[..., None]  # (dr.interpolate gives 0 where nothing was rasterised)
    nrm = torch.nn.functional.normalize(seeded((B, H, W, 3), 3, -1, 1), dim=-1)
    w2c = seeded((1 if shared else B, 4, 4), 4, -1, 1)
    w2c[:, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    view = seeded((B, 1, 1, 3), 5, -1, 1)
    out = R.shade(pos, nrm, nrm, None, pos, w2c.expand(B, -1, -1), view, None, None, "diffuse", render_modes=["depth"], cover=None)["depth"]
    assert out.shape == (B, H, W, 2) and bool((out[..., 1] == 1).all())
    ref32 = depth_ref.depth(pos, w2c)
    ref64 = depth_ref.depth(pos.double(), w2c.double())
    z = depth_ref.camera_z(pos.double(), w2c.double())
    assert float((z.amax(dim=(1, 2)) - z.amin(dim=(1, 2))).min()) >= 1.0 and float(z.abs().max()) <= 4.0
    assert float((out[..., :1] - ref32).abs().max()) <= 4 * 2.0 ** -23
    assert float((out[..., :1].double() - ref64).abs().max()) <= 1e-5
    assert float(ref64.min()) == 0.0 and float(ref64.max()) == 1.0


def test_depth_ref_shares_an_extreme_among_the_uncovered_pixels():
    """The tie rule the HIP adjoint follows: with the uncovered pixels' z (= w2c[2,3]) as the minimum, the covered rows get no share of
    d(loss)/dm; with a covered pixel as the minimum that row gets all of it."""
    pix = torch.tensor([1, 2, 5])
    cover = torch.zeros(1, 2, 3, dtype=torch.bool).view(-1).index_fill(0, pix, True).view(1, 2, 3)
    w2c = torch.eye(4, dtype=torch.float64)[None].clone()
    w2c[0, 2, 3] = 0.5
    for z0, low in ((0.2, None), (-0.2, 0)):  # (z of a row = its third coordinate + 0.5; of an uncovered pixel 0.5)
        rows = torch.tensor([[0.0, 0.0, z0], [0.0, 0.0, 0.9], [0.0, 0.0, 1.4]], dtype=torch.float64, requires_grad=True)
        d = depth_ref.depth(depth_ref.dense_positions(rows, pix, (1, 2, 3)), w2c)
        (d * cover[..., None]).sum().backward()
        r = 1.0 / (1.4 - min(0.0, z0))
        dcov = d.detach().view(-1)[pix]
        want = torch.full((3,), r, dtype=torch.float64)
        if low is not None:
            want[low] += r * float((dcov - 1).sum())
        want[2] += -r * float(dcov.sum())
        assert torch.allclose(rows.grad[:, 2], want, atol=1e-12), (z0, rows.grad[:, 2], want)


def test_ca_buffer_keeps_its_layout_and_the_depth_source_comes_after_shaded_out():
    """The depth source rides behind an existing entry point, in fields appended to a3d_ca_shade (a3d_ca_buffer is held to its size by
    the supersampling tests): every earlier field keeps its offset, the new ones follow the last old one, the version stays."""
    names = [f[0] for f in L.CaBuffer._fields_]
    assert names[-1] == "g_null" and ctypes.sizeof(L.CaBuffer) == 112 and L.CaBuffer.g_null.offset == 104
    assert [L.CaBuffer.vals.offset, L.CaBuffer.out.offset, L.CaBuffer.vals_rows.offset, L.CaBuffer.spp.offset] == [8, 24, 72, 80]
    sh = [f[0] for f in L.CaShade._fields_]
    old = ["size", "kd_stride", "gb", "par", "kd", "clear", "n_clear", "two_sided", "params", "shaded_out"]
    new = ["depth_gb", "depth_w2c_row", "depth_w2c_stride", "depth_pix", "depth_rows", "depth_state", "depth_out", "g_depth_gb", "g_depth_slots"]
    assert sh == old + new
    assert [getattr(L.CaShade, n).offset for n in old] == [0, 4, 8, 16, 24, 32, 40, 44, 48, 56]
    assert L.CaShade.depth_gb.offset == 64 and [getattr(L.CaShade, n).offset for n in new] == list(range(64, 136, 8))
    assert ctypes.sizeof(L.CaShade) == 136 and L.CaShade(size=136).depth_gb is None
    assert L.ABI_VERSION == 405


def _fwd(buf, shade, second=None):
    return L.lib().a3d_composite_aa_fwd(ctypes.addressof(buf), None if second is None else ctypes.addressof(second), FAKE, FAKE, FAKE, 4096, 1, 8, 8,
                                        None, ctypes.addressof(shade), None)


def _depth_source(**kw):
    args = dict(size=ctypes.sizeof(L.CaShade), depth_gb=FAKE, depth_w2c_row=FAKE, depth_w2c_stride=16, depth_pix=FAKE, depth_rows=5,
                depth_state=FAKE, depth_out=FAKE)
    args.update(kw)
    return L.CaShade(**args)


def test_entry_point_refuses_the_depth_combinations_before_anything_is_launched():
    lib = L.lib()
    full = ctypes.sizeof(L.CaBuffer)
    cases = {
        "C != 1": (L.CaBuffer(size=full, C=3, out=FAKE), _depth_source(), None),
        "vals given": (L.CaBuffer(size=full, C=1, vals=FAKE, out=FAKE), _depth_source(), None),
        "on a shaded buffer": (L.CaBuffer(size=full, C=1, out=FAKE), _depth_source(gb=FAKE, kd=FAKE, kd_stride=3, par=FAKE), None),
        "spp > 1": (L.CaBuffer(size=full, C=1, out=FAKE, spp=2, aa=1, cover_rast=FAKE, null_vals=FAKE), _depth_source(), None),
        "spp > 1 second": (L.CaBuffer(size=full, C=1, out=FAKE), _depth_source(),
                           L.CaBuffer(size=full, C=3, vals=FAKE, out=FAKE, spp=2, aa=1, cover_rast=FAKE, null_vals=FAKE)),
        "no state": (L.CaBuffer(size=full, C=1, out=FAKE), _depth_source(depth_state=None), None),
        "no w2c row": (L.CaBuffer(size=full, C=1, out=FAKE), _depth_source(depth_w2c_row=None), None),
        "struct between the sizes": (L.CaBuffer(size=full, C=1, out=FAKE), _depth_source(size=ctypes.sizeof(L.CaShade) - 4), None),
    }
    for what, (buf, shade, second) in cases.items():
        assert _fwd(buf, shade, second) != 0, what
        assert "invalid argument" in lib.a3d_last_error().decode(), what
    # the backward: the same checks, and the row count of the call must be the source's
    buf = L.CaBuffer(size=full, C=1, g_out=FAKE, g_vals=FAKE)
    bwd = lambda b, sh, P: lib.a3d_composite_aa_bwd(ctypes.addressof(b), None, FAKE, P, FAKE, FAKE, FAKE, 4096, FAKE, 1, FAKE, 1, 3, 1, 8, 8, FAKE,
                                                    ctypes.addressof(sh), None)
    assert bwd(buf, _depth_source(g_depth_gb=0x1000, g_depth_slots=0x2000), 4) != 0 and "depth_rows" in lib.a3d_last_error().decode()
    assert bwd(buf, _depth_source(g_depth_slots=0x2000), 5) != 0 and "g_depth_gb" in lib.a3d_last_error().decode()  # (no gradient array)
    assert bwd(buf, _depth_source(g_depth_gb=0x1004, g_depth_slots=0x2000), 5) != 0  # (rows are written as 16-byte stores)
    assert bwd(buf, _depth_source(g_depth_gb=0x1000), 5) != 0 and "g_depth_slots" in lib.a3d_last_error().decode()  # (no scratch)
    assert bwd(L.CaBuffer(size=full, C=2, g_out=FAKE, g_vals=FAKE), _depth_source(g_depth_gb=0x1000, g_depth_slots=0x2000), 5) != 0


def test_a_shade_struct_of_the_header_before_the_depth_source_is_still_read_as_one():
    """size = the offset of depth_gb: the entry point reads the struct as the shading recipe it was (here refused for ITS reasons -- no
    G-buffer rows -- not for its size); one dword shorter is refused for its size."""
    lib = L.lib()
    buf = L.CaBuffer(size=ctypes.sizeof(L.CaBuffer), C=3, out=FAKE)
    old = L.CaShade(size=L.CaShade.depth_gb.offset, depth_gb=FAKE)  # (the field lies past `size`: not read)
    assert _fwd(buf, old) != 0
    msg = lib.a3d_last_error().decode()
    assert "sh->gb" in msg and "size ==" not in msg, msg
    assert _fwd(buf, L.CaShade(size=L.CaShade.depth_gb.offset - 4)) != 0 and "size" in lib.a3d_last_error().decode()


def test_switch_and_mode_table():
    R = importlib.import_module("3danimals_amd.model.render.render")
    assert {"depth", "tangent"} <= R.FUSED_GBUFFER_MODES and isinstance(R.FUSED_DEPTH_TANGENT, bool)
    assert "depth" in R.ANTIALIASED_MODES and "tangent" not in R.ANTIALIASED_MODES
    ops = importlib.import_module("3danimals_amd.ops")
    assert callable(ops.depth_composite_antialias)
