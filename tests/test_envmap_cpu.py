"""Environment probes without a GPU: the torch-statement route of util.latlong_to_cubemap against the float64 restatement
(tests/envmap_ref.py), cube_to_dir against the cube lookup's face rule, the colour transforms, the argument rules of generated
coordinates (uv == NULL in a3d_texture_fwd / a3d_texture_bwd) through ctypes, the unchanged ABI surface and what the overlay exports."""
import ctypes
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import envmap_ref as E  # noqa: E402
import texture_ref as R  # noqa: E402

EPS23 = 2.0 ** -23
C_MAX = 8 * 0.56


@pytest.fixture(scope="module")
def util():
    return importlib.import_module("3danimals_amd.model.render.util")


def _ratio(got, want, tex, L):
    return float((got.double() - want).abs().max()) / (EPS23 * L * float(tex.max() - tex.min()))


@pytest.mark.parametrize("size, res", [((4, 8), [1, 1]), ((4, 8), [2, 2]), ((8, 16), [4, 4]), ((8, 16), [2, 3]), ((16, 32), [8, 8]), ((16, 32), [7, 7])])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_torch_route_on_cpu_tensors_against_the_float64_restatement(util, size, res, dtype):
    """CPU tensors take the reference's statements with the shim's torch tap.  float64 maps agree with the restatement to float64
    rounding; float32 maps within C_MAX * 2^-23 * L * (max - min), L the larger map dimension: a coordinate error of a few ulp through
    a bilinear tap, C_MAX = 8 x the float32 restatement's own worst ratio (0.56), the ceiling the HIP kernel is held to as well.  The
    texels that look along +-y (odd face sizes), where the longitude is undefined, are left out."""
    g = torch.Generator().manual_seed(size[0] * 100 + res[0])
    tex = torch.rand(*size, 3, generator=g, dtype=torch.float32)
    want = E.latlong_to_cubemap(tex, res)
    assert int(E.pole_mask(res).sum()) == 0 or res[0] % 2 == 1
    live = ~E.pole_mask(res)
    got = util.latlong_to_cubemap(tex.to(dtype), res)
    assert got.dtype == dtype and got.device == tex.device and tuple(got.shape) == (6, res[0], res[1], 3)
    r = _ratio(got[live], want[live], tex, max(size))
    assert r <= (C_MAX if dtype == torch.float32 else 1e-6), r
    # differentiable in the map
    t = tex.double().requires_grad_(True)
    w = torch.rand(6, res[0], res[1], 3, generator=g, dtype=torch.float64) * live[..., None]
    (util.latlong_to_cubemap(t, res) * w).sum().backward()
    t2 = tex.double().requires_grad_(True)
    (E.latlong_to_cubemap(t2, res) * w).sum().backward()
    assert torch.allclose(t.grad, t2.grad, rtol=0, atol=1e-9 * float(w.sum()))


def test_cubemap_to_latlong_on_cpu_tensors_raises_the_shims_error(util):
    with pytest.raises(NotImplementedError, match="cube-map sampling needs GPU tensors"):
        util.cubemap_to_latlong(torch.zeros(6, 4, 4, 3), [4, 8])


def test_cube_to_dir_inverts_the_face_rule_on_the_face_centres(util):
    zero = torch.zeros(1, dtype=torch.float64)
    want = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    for s in range(6):
        d = util.cube_to_dir(s, zero, zero)
        assert d.shape == (1, 3) and d[0].tolist() == [float(v) for v in want[s]]
        face, fs, ft, m = R.cube_face(d)
        assert int(face) == s and float(fs) == 0 and float(ft) == 0 and float(m) == 1
    # and off the centre: the lookup's face coordinates of cube_to_dir(s, x, y) are (x, y)
    x, y = torch.tensor([0.25, -0.5], dtype=torch.float64), torch.tensor([-0.75, 0.125], dtype=torch.float64)
    for s in range(6):
        face, fs, ft, _ = R.cube_face(util.cube_to_dir(s, x, y))
        assert face.tolist() == [s, s] and torch.equal(fs, x) and torch.equal(ft, y)
        assert torch.equal(util.cube_to_dir(s, x, y), R.cube_to_dir(torch.full((2,), s), x, y))


def test_srgb_transforms_invert_each_other(util):
    x = torch.cat([torch.linspace(0, 1, 1001, dtype=torch.float64), torch.tensor([0.0031308, 0.04045, 0.003, 0.05], dtype=torch.float64)])
    rgb = x[:, None, None].expand(-1, 1, 3).contiguous()
    back = util.rgb_to_srgb(util.srgb_to_rgb(rgb))
    assert torch.allclose(back, rgb, rtol=0, atol=1e-6)  # (the two published thresholds meet to ~1e-7)
    assert torch.allclose(util.srgb_to_rgb(util.rgb_to_srgb(rgb)), rgb, rtol=0, atol=1e-6)
    assert float(util.rgb_to_srgb(torch.full((1, 1, 3), 0.001))[0, 0, 0]) == pytest.approx(0.01292)
    assert float(util.srgb_to_rgb(torch.full((1, 1, 3), 0.5))[0, 0, 0]) == pytest.approx(((0.5 + 0.055) / 1.055) ** 2.4)
    rgba = torch.rand(2, 3, 4, dtype=torch.float64)
    out = util.rgb_to_srgb(rgba)
    assert out.shape == rgba.shape and torch.equal(out[..., 3], rgba[..., 3]) and torch.equal(out[..., :3], util.rgb_to_srgb(rgba[..., :3]))


def test_generated_coordinates_are_validated_before_any_launch_and_the_abi_did_not_grow():
    """uv == NULL with a rule broken: A3D_EINVAL and the rule in a3d_last_error(); no pointer below is ever dereferenced (no GPU)."""
    L = importlib.import_module("3danimals_amd._lib")
    lib = L.lib()
    fake = 0x1000

    def desc(boundary=0, filt=1, tex_batch=1, levels=1):
        d = L.TexDesc(size=ctypes.sizeof(L.TexDesc), C=3, tex_batch=tex_batch, filter=filt, boundary=boundary, levels=levels)
        for l in range(levels):
            d.height[l] = d.width[l] = 8 >> l
            d.level[l] = fake
        return d

    fwd = lambda d, B=6, uv_da=None, bias=None: lib.a3d_texture_fwd(ctypes.byref(d), None, uv_da, bias, B, 4, 4, fake, None)
    bwd = lambda d, B=6, uv_da=None, bias=None, g_uv=None, g_da=None, g_bias=None: lib.a3d_texture_bwd(
        ctypes.byref(d), fake, None, uv_da, bias, B, 4, 4, g_uv, g_da, g_bias, None)
    cases = [
        ("B == 6", lambda f: f(desc(), B=5)),
        ("A3D_TEX_LINEAR", lambda f: f(desc(filt=0))),
        ("uv_da", lambda f: f(desc(), uv_da=fake)),
        ("uv_da", lambda f: f(desc(), bias=fake)),
        ("A3D_TEX_WRAP", lambda f: f(desc(boundary=1))),
        ("A3D_TEX_WRAP", lambda f: f(desc(boundary=2))),
        ("levels must be 1", lambda f: f(desc(levels=2))),
        ("A3D_TEX_LINEAR", lambda f: f(desc(filt=3, levels=2))),
        ("tex_batch == 1", lambda f: f(desc(tex_batch=6))),
        ("B == tex_batch", lambda f: f(desc(boundary=3, tex_batch=2), B=1)),
    ]
    for name, f in (("a3d_texture_fwd", fwd), ("a3d_texture_bwd", bwd)):
        for rule, case in cases:
            assert case(f) == -1, (name, rule)
            msg = lib.a3d_last_error().decode()
            assert rule in msg and "generated coordinates" in msg and name in msg, (name, rule, msg)
    assert bwd(desc(), g_uv=fake) == -1 and "g_uv must be NULL" in lib.a3d_last_error().decode()
    assert bwd(desc(), g_bias=fake) == -1 and "gradients must be NULL" in lib.a3d_last_error().decode()
    # ... and the mode cost the ABI nothing: the same version, entry points and descriptor
    assert L.ABI_VERSION == 405 and lib.a3d_version() == 405
    assert len(L.SIGNATURES) == 126
    assert ctypes.sizeof(L.TexDesc) == 4 * 6 + 4 * 32 + 8 * 32


def test_overlay_exports_the_resamplers_and_keeps_the_image_io_private():
    overlay = importlib.import_module("3danimals_amd.overlay")
    u = overlay.exported_names("model.render.util")
    for name in ("latlong_to_cubemap", "cubemap_to_latlong", "cube_to_dir", "rgb_to_srgb", "srgb_to_rgb"):
        assert name in u and u[name].__module__ == "3danimals_amd.model.render.util", name
    for name in ("load_image", "load_image_raw", "save_image", "save_image_raw"):
        assert name not in u, name
    m = overlay.mirror("model.render.util")
    assert all(callable(getattr(m, n)) for n in ("load_image", "load_image_raw", "save_image", "save_image_raw"))
    l = overlay.exported_names("model.render.light")
    assert {"load_env", "save_env_map", "EnvironmentLight"} <= set(l)


def test_image_files_route_by_extension(util, tmp_path):
    import numpy as np

    img = np.random.default_rng(0).random((4, 9, 3)).astype(np.float32)
    fn = str(tmp_path / "probe.HDR")
    util.save_image_raw(fn, img)
    back = util.load_image(fn)
    assert back.dtype == np.float32 and back.shape == img.shape
    assert (np.abs(back - img) <= img.max(axis=-1, keepdims=True) / 128).all()
    assert np.array_equal(util.load_image_raw(fn), back)
    with pytest.raises(ValueError, match="only Radiance .hdr"):
        util.save_image_raw(str(tmp_path / "probe.exr"), img)
    png = str(tmp_path / "a.png")
    try:
        import PIL  # noqa: F401
    except ImportError:  # without Pillow only .hdr is served, and the error says so
        with pytest.raises(RuntimeError, match="Pillow"):
            util.save_image(png, img)
        return
    util.save_image(png, img)
    ldr = util.load_image(png)
    assert ldr.dtype == np.float32 and np.abs(ldr - img).max() <= 0.5 / 255 + 1e-6
    assert util.load_image_raw(png).dtype == np.uint8
