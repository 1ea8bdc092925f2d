"""Environment-lit shading without a GPU: the entry points of include/a3d_envshade.h, argument validation before any launch, the named
cases of tests/envshade_cases.py (each holds what it names; the share of pixels near a gradient kink, measured on float64 alone), and the proof that the GPU tests'
tolerance bites: a float64 restatement of the shade whose backward loses one piece at a time must leave it."""
import ctypes
import importlib
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_check as A  # noqa: E402
import envshade_cases as C  # noqa: E402
import envlight_ref as R  # noqa: E402

HEADER = os.path.join(ROOT, "include", "a3d_envshade.h")
FAKE = 0x1000  # non-NULL, never dereferenced


def _L():
    return importlib.import_module("3danimals_amd._lib")


def test_sixth_header_matches_the_sixth_table_and_the_other_surfaces_are_untouched():
    """What is this surface's own (tests/test_abi_cpu.py holds every surface's table, struct mirrors and constants to its header)."""
    protos = A.prototypes("a3d_envshade.h")
    assert protos == {"a3d_env_shade_fwd": ("int", ["ptr", "ptr"]), "a3d_env_shade_bwd": ("int", ["ptr", "ptr"])}
    light = importlib.import_module("3danimals_amd.model.render.light")
    assert light.HIP_ENV_SHADE is True and light.EnvironmentLight.MIN_ROUGHNESS == R.MIN_ROUGHNESS and light.EnvironmentLight.MAX_ROUGHNESS == R.MAX_ROUGHNESS


def _good(L, levels=(64, 32, 16), bwd=False):
    d = L.EnvShadeDesc(size=ctypes.sizeof(L.EnvShadeDesc), levels=len(levels), diffuse_size=16, fg_height=256, fg_width=256, specular=1, mtx_batch=1,
                       B=2, H=5, W=7, min_roughness=0.08, max_roughness=0.5)
    d.diffuse = d.fg = d.mtx = d.out = FAKE
    for l, s in enumerate(levels):
        d.spec[l], d.spec_size[l] = FAKE, s
    for i in range(5):
        getattr(d, "in")[i], d.pixel_stride[i], d.image_stride[i] = FAKE, 3, 105
    if bwd:
        d.g_out = FAKE
    return d


def test_entry_points_refuse_invalid_descriptors_before_anything_is_launched():
    """None of the pointers below is ever dereferenced and nothing is launched (this runs without a GPU)."""
    L = _L()
    lib = L.lib()

    def refused(fn, d, *words):
        assert getattr(lib, fn)(ctypes.byref(d) if d is not None else None, None) == -1, (fn, words)
        msg = lib.a3d_last_error().decode()
        assert "invalid argument" in msg and fn in msg and all(w in msg for w in words), (fn, msg)

    for fn, bwd in (("a3d_env_shade_fwd", False), ("a3d_env_shade_bwd", True)):
        refused(fn, None, "desc")
        d = _good(L, bwd=bwd)
        d.size = ctypes.sizeof(L.EnvShadeDesc) - 8  # a caller built against a shorter struct: refused before any other field is read
        d.B = -1
        refused(fn, d, "desc->size", "older header")

        def broken(words=(), **fields):
            d = _good(L, bwd=bwd)
            for k, v in fields.items():
                setattr(d, k, v)
            refused(fn, d, *words)
            return d

        broken(diffuse=None)  # a null map
        broken(fg=None)
        broken(mtx=None)
        broken(diffuse_size=0)
        for dim in ("B", "H", "W"):
            broken(**{dim: 0})
        broken(mtx_batch=3)  # neither 0, 1 nor B
        broken(min_roughness=0.5)  # lo < hi < 1
        broken(max_roughness=1.0)
        refused(fn, _good(L, levels=(32, 16), bwd=bwd), "at least 3 specular levels")
        refused(fn, _good(L, levels=(64, 32, 8), bwd=bwd), "halving rule")
        refused(fn, _good(L, levels=(63, 31, 15), bwd=bwd), "halving rule")
        d = _good(L, bwd=bwd)
        d.spec[1] = None
        refused(fn, d, "specular level 1")
        for i in range(5):
            d = _good(L, bwd=bwd)
            getattr(d, "in")[i] = None
            refused(fn, d, "in[%d]" % i)
            d = _good(L, bwd=bwd)
            d.pixel_stride[i] = -3
            refused(fn, d, "in[%d]" % i)
        broken(**{"g_out" if bwd else "out": None})
        # without the specular term nothing of the stack, the table or the constants is read
        d = _good(L, levels=(5, 3), bwd=bwd)
        d.specular, d.fg, d.B = 0, None, 0
        refused(fn, d, "d->B > 0")


@pytest.mark.parametrize("name", list(C.LIGHTS))
def test_lights_hold_what_they_name(name):
    sizes, dsize = C.LIGHTS[name]
    spec, dif = C.light(name)
    assert [tuple(s.shape) for s in spec] == [(6, s, s, 3) for s in sizes] and tuple(dif.shape) == (6, dsize, dsize, 3)
    assert len(sizes) >= 3 and all(b * 2 == a for a, b in zip(sizes, sizes[1:]))
    assert all(torch.equal(t, t.float().double()) and float(t.min()) >= 0 for t in spec + [dif])
    lds = [s for s in sizes if s <= 16]
    if name == "a_8_4_2":
        assert lds == list(sizes) and dsize == 2  # everything in LDS; a 2 x 2 face: every tap of the diffuse lookup leaves the face
    if name == "b_64_32_16":
        assert lds == [16] and dsize == 16  # both scatter routes
    if name == "c_64_to_4":
        leaves = C.frame((1, 1, 1000), 1)
        mip = R.get_mip(leaves[3][..., 1], len(sizes))
        assert len(sizes) == 5 and float(mip.max()) == len(sizes) - 1 and float(mip.min()) == 0
        assert int(((mip > len(sizes) - 2) & (mip < len(sizes) - 1)).sum()) > 100  # the upper branch, short of the top


@pytest.mark.parametrize("frame_name", list(C.FRAMES))
def test_frames_hold_what_they_name_and_few_pixels_lie_near_a_kink(frame_name):
    B, H, W = shape = C.FRAMES[frame_name]
    tiled = H >= 8 and W >= 8
    assert tiled == (frame_name in ("2x16x16", "1x9x8"))
    if frame_name == "1x9x8":
        assert H % 8 != 0  # a partial tile row
    if frame_name == "3x5x7":
        assert W < 8 and B * H * W > 64  # consecutive pixels, more than one wave, images change inside a wave
    for view in C.VIEWS:
        pos, n, kd, ks, v = leaves = C.frame(shape, 2, view)
        assert tuple(v.shape) == ((B, 1, 1, 3) if view == "image" else (B, H, W, 3)) and all(tuple(t.shape) == (B, H, W, 3) for t in leaves[:4])
        assert all(torch.equal(t, t.float().double()) for t in leaves)
        assert float((n.norm(dim=-1) - 1).abs().max()) < 1e-6 and float(ks[..., 1].max()) <= 1.2
    if B * H * W >= 1000:
        r = leaves[3][..., 1]
        assert bool((r < C.LO).any() and ((r > C.LO) & (r < C.HI)).any() and ((r > C.HI) & (r < 1)).any() and (r > 1).any())
    for kind in C.TRANSFORMS:
        m = C.transform(kind, B)
        if m is not None:
            rot = m[:, :3, :3]
            assert m.shape[0] == (1 if kind == "one" else B) and float((rot @ rot.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
            assert float((rot - torch.eye(3, dtype=torch.float64)).abs().max()) > 0.1 and float(m[:, :3, 3].abs().min()) >= 5


def test_few_pixels_of_a_random_case_lie_near_a_kink():
    """The share of pixels left out of the gradient comparison, on the float64 reference alone: below 1 % in every random case
    (expected about 2 axes x 3 grids x 2e-4), and the cases cover every operand form."""
    cases = C.random_cases()
    assert len(cases) == len(C.FRAMES) * len(C.LIGHTS)
    assert {c[2] for c in cases} == set(C.VIEWS) and {c[3] for c in cases} == set(C.TRANSFORMS) and {c[4] for c in cases} == {True, False}
    total = 0
    for light_name, frame_name, view, xfm, specular in cases:
        shape = C.FRAMES[frame_name]
        leaves = C.frame(shape, C.SEED, view)
        near = C.near_kink(*C.LIGHTS[light_name], leaves, specular, C.transform(xfm, shape[0], C.SEED))
        share = float(near.double().mean())
        total += int(near.sum())
        print(f"{light_name} {frame_name} view={view} xfm={xfm} specular={specular}: {int(near.sum())} of {near.numel()} near a kink")
        assert share < 0.01, (light_name, frame_name, share)
    assert total > 0  # (the measure is not blind)


def test_the_kink_measure_finds_directed_kinks():
    """Directed cases (exempt from the 1 % cap: every pixel is ON a kink): a normal on a cube-face diagonal, one at a texel boundary,
    roughness at lo / hi / 1 and at an integer level, n.v at 1e-4."""
    sizes, dsize = C.LIGHTS["c_64_to_4"]
    base = C.frame((1, 1, 8), 3)
    base[3][..., 1] = 0.3
    assert not bool(C.near_kink(sizes, dsize, base).any())

    def hits(i, value, channel=None, **kw):
        leaves = [t.clone() for t in base]
        if channel is None:
            leaves[i][0, 0, :] = torch.as_tensor(value, dtype=torch.float64)
        else:
            leaves[i][0, 0, :, channel] = value
        return bool(C.near_kink(sizes, dsize, leaves, **kw).all())

    assert hits(1, [0.6, 0.6, 0.1]) and hits(1, [0.3, -0.9, 0.9])  # face diagonals
    assert hits(1, [1.0, 0.25, 0.3], specular=False)  # (0.25 + 1) / 2 * 4 - 0.5 = 2: on a texel centre line of the 4 x 4 diffuse map
    for r in (C.LO, C.HI, 1.0, C.LO + (C.HI - C.LO) / 3):  # the last: level 1 of 5
        assert hits(3, r, channel=1), r
    assert not hits(3, 0.31, channel=1) and not hits(3, 0.05, channel=1) and not hits(3, 1.1, channel=1)  # constant level below lo, above 1
    wo = R.safe_normalize(base[4] - base[0])
    t = torch.linalg.cross(wo, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand_as(wo))
    leaves = [x.clone() for x in base]
    leaves[1] = t / t.norm(dim=-1, keepdim=True) + 1e-4 * wo
    assert bool(C.near_kink(sizes, dsize, leaves).all())


MUTATION_TARGETS = {"no_bias_grad": "ks", "no_fg_roughness_grad": "ks", "no_fg_ndv_grad": "gb_normal", "no_visibility_factor": "kd",
                    "rotation_not_transposed": "gb_normal", "no_coarse_slot_scatter": "specular[1]"}


def _restated_grads(dtype, mutate, spec64, dif64, leaves64, go64, mtx64):
    spec = [t.detach().clone().to(dtype).requires_grad_(True) for t in spec64]
    dif = dif64.detach().clone().to(dtype).requires_grad_(True)
    leaves = [t.detach().clone().to(dtype).requires_grad_(True) for t in leaves64]
    out = C.shade_restated(spec, dif, C.fg_table().to(dtype), leaves, True, None if mtx64 is None else mtx64.to(dtype), mutate)
    wrt = leaves + [dif] + spec
    gs = torch.autograd.grad((out * go64.to(dtype)).sum(), wrt, allow_unused=True)
    names = ["gb_pos", "gb_normal", "kd", "ks", "view_pos", "diffuse"] + [f"specular[{l}]" for l in range(len(spec))]
    return out.detach(), {n: (torch.zeros_like(t) if g is None else g).detach() for n, g, t in zip(names, gs, wrt)}


@pytest.fixture(scope="module")
def bite():
    """The named case the bounds are shown to bite on: light b (both scatter routes), [2,16,16], one lookup transform; float64 and
    float32 restatements, computed once."""
    spec64, dif64 = C.light("b_64_32_16")
    shape = C.FRAMES["2x16x16"]
    leaves64 = C.frame(shape, 11)
    mtx64 = C.transform("one", shape[0], 11)
    near = C.near_kink(*C.LIGHTS["b_64_32_16"], leaves64, True, mtx64)
    go64 = torch.randn(*shape, 3, generator=C._gen(511), dtype=torch.float64).float().double()
    go64[near] = 0
    args = (spec64, dif64, leaves64, go64, mtx64)
    out64, g64 = _restated_grads(torch.float64, None, *args)
    out32, g32 = _restated_grads(torch.float32, None, *args)
    return args, out64, g64, out32, g32


def test_the_restatement_is_the_reference(bite):
    (spec64, dif64, leaves64, go64, mtx64), out64, g64, out32, g32 = bite
    want = C.reference(spec64, dif64, C.fg_table(), leaves64, True, mtx64)
    assert float((out64 - want).abs().max()) <= 1e-13 * float(want.abs().max())
    for name in g64:  # the float32 restatement stays inside its own bound, and that bound is tight: far below the gradients themselves
        assert float((g32[name].double() - g64[name]).abs().max()) <= C.tolerance(g32[name], g64[name]) / 4
        assert C.tolerance(g32[name], g64[name]) < 1e-3 * float(g64[name].abs().max()), name


@pytest.mark.parametrize("mutate", list(C.MUTATIONS))
def test_a_backward_that_loses_one_piece_leaves_the_tolerance(bite, mutate):
    args, out64, g64, out32, g32 = bite
    out_m, g_m = _restated_grads(torch.float64, mutate, *args)
    assert torch.equal(out_m, out64) or float((out_m - out64).abs().max()) < 1e-12  # the values stay: only the backward is broken
    name = MUTATION_TARGETS[mutate]
    err, tol = float((g_m[name] - g64[name]).abs().max()), C.tolerance(g32[name], g64[name])
    print(f"{mutate}: max |g_{name} - x64| {err:.3e}, allowed {tol:.3e}")
    assert err > 10 * tol, (mutate, name, err, tol)


def test_a_wrong_sign_of_g_view_and_a_dropped_pixel_leave_the_tolerance(bite):
    (spec64, dif64, leaves64, go64, mtx64), out64, g64, out32, g32 = bite
    # +g_pos for g_view: view_pos [B,1,1,3] receives the image's sum of -g_pos
    wrong = g64["gb_pos"].sum(dim=(1, 2), keepdim=True)
    assert float((-wrong - g64["view_pos"]).abs().max()) <= 1e-12 * float(g64["view_pos"].abs().max())
    assert float((wrong - g64["view_pos"]).abs().max()) > 10 * C.tolerance(g32["view_pos"], g64["view_pos"])
    # one pixel's contribution to the diffuse map dropped: what that pixel alone sends
    one = torch.zeros_like(go64)
    one[1, 7, 9] = go64[1, 7, 9]
    assert float(one.abs().max()) > 0
    _, g_one = _restated_grads(torch.float64, None, spec64, dif64, leaves64, one, mtx64)
    assert float(g_one["diffuse"].abs().max()) > 10 * C.tolerance(g32["diffuse"], g64["diffuse"])
