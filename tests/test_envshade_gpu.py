"""EnvironmentLight.shade as one HIP launch each way (csrc/envshade.hip, ops.env_shade, light.HIP_ENV_SHADE) against float64.

Yardstick: tests/envlight_ref.shade with the lookups of tests/texture_ref.py, gradients by autograd (x64).  Bound, per tensor -- the
values, the five per-pixel gradients, g_diffuse and every g_specular[l] --: max |hip - x64| <= 4 max(max |x32 - x64|, 2^-22 max |x64|),
x32 = the float32 statements (EnvironmentLight._shade_torch) on the same inputs on the device; for the per-pixel gradients also
mean e(hip) <= 2 mean e(x32) with e of tests/bsdf_cases.rel_err.  A mean needs a sample: a gradient of fewer than MEAN_ROWS rows -- the
single-pixel list, and the three numbers per image that a view_pos [B,1,1,3] receives -- holds a handful of float32 roundings, and the
statements land within an ulp of float64 by luck as often as the kernel does (measured on the single-pixel lists: ratios 0.06 ... 17.0,
every error below 4e-6 relative).  Those rows are not left out: the same rule is applied to all of them pooled
(test_mean_rule_on_the_small_gradients_pooled); the max rule holds each of them on its own.  Pixels that tests/envshade_cases.near_kink finds within 1e-4 texel
units / 1e-5 of a kink get a zero output gradient, which leaves them out of every gradient comparison and of nothing else.
The ranges measured on an MI355X (printed by the tests), the threshold and the pooled ratio are in DESIGN.md section 16."""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import envshade_cases as C  # noqa: E402
from bsdf_cases import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("gb_pos", "gb_normal", "kd", "ks", "view_pos")
MEAN_ROWS = 32  # rows from which a per-pixel gradient is held to the mean rule on its own


def _mods():
    return (importlib.import_module("3danimals_amd.ops"), importlib.import_module("3danimals_amd.model.render.light"),
            importlib.import_module("3danimals_amd._lib"))


@pytest.fixture(autouse=True)
def _same_fg_table_and_switch():
    """The device light reads the table the float64 side reads (rounded to float32 once), and the switch is back at its default."""
    _, light, _ = _mods()
    key = str(torch.device("cuda", torch.cuda.current_device()))
    before, had = light._fg_cache.get(key), key in light._fg_cache
    light._fg_cache[key] = C.fg_table().float().cuda()
    try:
        yield
    finally:
        light.HIP_ENV_SHADE = True
        if had:
            light._fg_cache[key] = before
        else:
            light._fg_cache.pop(key, None)


def _device_light(spec64, dif64, grad=True):
    _, light, _ = _mods()
    lgt = light.EnvironmentLight(torch.zeros(6, 2, 2, 3, device="cuda"))
    lgt.specular = [t.float().cuda().requires_grad_(grad) for t in spec64]
    lgt.diffuse = dif64.float().cuda().requires_grad_(grad)
    return lgt


def _grads(out, go, wrt):
    gs = torch.autograd.grad((out * go).sum(), wrt, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(gs, wrt)]


def _device_run(fused, spec64, dif64, leaves64, go64, specular, mtx64, layout=None):
    """-> (values, gradients to the five inputs, the diffuse map and every specular level) of lgt.shade on the device."""
    _, light, _ = _mods()
    lgt = _device_light(spec64, dif64)
    lgt.xfm(None if mtx64 is None else mtx64.float().cuda())
    leaves = [t.float().cuda().requires_grad_(True) for t in leaves64]
    args = leaves if layout is None else layout(leaves)
    light.HIP_ENV_SHADE = fused
    try:
        out = lgt.shade(*args, specular=specular)
    finally:
        light.HIP_ENV_SHADE = True
    return out.detach(), _grads(out, go64.float().cuda().reshape(out.shape), leaves + [lgt.diffuse] + lgt.specular)


def _float64_run(spec64, dif64, leaves64, go64, specular, mtx64):
    spec = [t.clone().requires_grad_(True) for t in spec64]
    dif = dif64.clone().requires_grad_(True)
    leaves = [t.clone().requires_grad_(True) for t in leaves64]
    out = C.reference(spec, dif, C.fg_table(), leaves, specular, mtx64)
    return out.detach(), _grads(out, go64, leaves + [dif] + spec)


def _case(light_name, frame_name, view, xfm, specular, seed):
    spec64, dif64 = C.light(light_name)
    shape = C.FRAMES[frame_name]
    leaves64 = C.frame(shape, seed, view)
    mtx64 = C.transform(xfm, shape[0], seed)
    near = C.near_kink(*C.LIGHTS[light_name], leaves64, specular, mtx64)
    go64 = torch.randn(*shape, 3, generator=C._gen(seed + 500), dtype=torch.float64).float().double()
    go64[near] = 0
    return spec64, dif64, leaves64, mtx64, near, go64


def _compare(what, hip, x32, x64, keep=None, mean_rule=False, pool=None):
    """prints the figures of one tensor -> whether it is inside its bounds.  ``pool``: a list that takes (e(hip), e(x32)) of a tensor too
    small for a mean of its own."""
    e_hip, e_32 = float((hip.double().cpu() - x64).abs().max()), float((x32.double().cpu() - x64).abs().max())
    tol = C.tolerance(x32.cpu(), x64)
    line = f"{what}: max |hip - x64| {e_hip:.3e}, max |x32 - x64| {e_32:.3e}, allowed {tol:.3e}, used {e_hip / tol if tol else 0.0:.3f}"
    ok = e_hip <= tol
    if mean_rule:
        eh, et = rel_err(hip, x64), rel_err(x32, x64)
        if keep is not None:
            k = keep.reshape(*keep.shape, 1).expand_as(eh)
            eh, et = eh[k], et[k]
        ah, at = (float(eh.mean()), float(et.mean())) if eh.numel() else (0.0, 0.0)
        line += f"; mean e(hip) {ah:.3e} / mean e(x32) {at:.3e} = {ah / max(at, 1e-300):.3f}"
        if eh.numel() >= 3 * MEAN_ROWS:
            ok = ok and ah <= 2 * at
        else:
            line += " (pooled)"
            if pool is not None:
                pool.append((eh.reshape(-1), et.reshape(-1)))
    print(line)
    return ok


def _random_case(light_name, frame_name, view, xfm, specular, pool=None):
    """-> the tensors of one random case that leave their bounds (none, one hopes)."""
    spec64, dif64, leaves64, mtx64, near, go64 = _case(light_name, frame_name, view, xfm, specular, seed=C.SEED)
    out64, g64 = _float64_run(spec64, dif64, leaves64, go64, specular, mtx64)
    out32, g32 = _device_run(False, spec64, dif64, leaves64, go64, specular, mtx64)
    outh, gh = _device_run(True, spec64, dif64, leaves64, go64, specular, mtx64)
    print(f"{light_name} {frame_name} view={view} xfm={xfm} specular={specular}: {int(near.sum())} of {near.numel()} pixels near a kink")
    bad = []
    if not _compare("values", outh, out32, out64):
        bad.append("values")
    names = list(NAMES) + ["diffuse"] + [f"specular[{l}]" for l in range(len(spec64))]
    for i, name in enumerate(names):
        keep = ~near if tuple(g64[i].shape[:-1]) == tuple(near.shape) else None
        if not _compare("g_" + name, gh[i], g32[i], g64[i], keep=keep if i < 5 else None, mean_rule=i < 5, pool=pool):
            bad.append("g_" + name)
    assert all(bool(torch.isfinite(g).all()) for g in gh)
    return bad


@pytest.mark.parametrize("light_name,frame_name,view,xfm,specular", C.random_cases())
def test_values_and_every_gradient_against_float64(light_name, frame_name, view, xfm, specular):
    assert not _random_case(light_name, frame_name, view, xfm, specular)


def test_mean_rule_on_the_small_gradients_pooled():
    """The per-pixel gradients of fewer than MEAN_ROWS rows of every random case -- the single-pixel lists, view_pos [B,1,1,3] --, all
    in one sample: mean e(hip) <= 2 mean e(x32)."""
    pool = []
    for light_name, frame_name, view, xfm, specular in C.random_cases():
        B, H, W = C.FRAMES[frame_name]
        if B * H * W < MEAN_ROWS or view == "image":
            _random_case(light_name, frame_name, view, xfm, specular, pool=pool)
    eh, et = torch.cat([a for a, _ in pool]), torch.cat([b for _, b in pool])
    ah, at = float(eh.mean()), float(et.mean())
    print(f"pooled over {len(pool)} tensors, {eh.numel()} numbers: mean e(hip) {ah:.3e} / mean e(x32) {at:.3e} = {ah / max(at, 1e-300):.3f}")
    assert len(pool) >= 15 and ah <= 2 * at


def test_gradient_reaches_env_base_through_build_mips():
    """create_trainable_env_rnd(64).build_mips() -> shade -> d / d env_base.  The float64 side takes the device's maps as its inputs and
    its map gradients go down the device's own build_mips backward, like the other two (the float64 build_mips takes 40 s and is
    held to its bound by tests/test_envlight_gpu.py): what is compared is the shade's part of the chain, at env_base."""
    _, light, _ = _mods()
    torch.manual_seed(4)
    lgt = light.create_trainable_env_rnd(64)
    lgt.build_mips()
    assert [s.shape[1] for s in lgt.specular] == [64, 32, 16]
    maps = lgt.specular + [lgt.diffuse]
    shape = (2, 16, 16)
    leaves64 = C.frame(shape, 21)
    spec64, dif64 = [s.detach().cpu().double() for s in lgt.specular], lgt.diffuse.detach().cpu().double()
    near = C.near_kink((64, 32, 16), 16, leaves64)
    go64 = torch.randn(*shape, 3, generator=C._gen(22), dtype=torch.float64).float().double()
    go64[near] = 0
    _, g64 = _float64_run(spec64, dif64, leaves64, go64, True, None)
    down = lambda gs: torch.autograd.grad(maps, lgt.base, grad_outputs=[g.float().cuda() for g in gs], retain_graph=True)[0]
    base64 = down(g64[6:] + [g64[5]])
    got = {}
    for fused in (False, True):
        light.HIP_ENV_SHADE = fused
        leaves = [t.float().cuda() for t in leaves64]
        out = lgt.shade(*leaves)
        got[fused], = torch.autograd.grad((out * go64.float().cuda()).sum(), lgt.base, retain_graph=True)
    assert _compare("g_env_base", got[True], got[False], base64.double().cpu())


def test_list_form_strided_views_and_two_runs_give_the_same_bits():
    """The same pixels as [B,H,W], as a [1,1,P] list and through stride-9 slices of a [...,9] tensor: torch.equal on the values and on
    the per-pixel gradients; two backward runs give identical per-pixel gradients."""
    spec64, dif64, leaves64, mtx64, near, go64 = _case("b_64_32_16", "2x16x16", "image", "one", True, seed=5)
    out, g = _device_run(True, spec64, dif64, leaves64, go64, True, mtx64)
    out2, g2 = _device_run(True, spec64, dif64, leaves64, go64, True, mtx64)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(g[:5], g2[:5]))

    def as_list(leaves):
        B, H, W, _ = leaves[0].shape
        return [t.expand(B, H, W, 3).reshape(1, 1, B * H * W, 3) for t in leaves]

    out_l, g_l = _device_run(True, spec64, dif64, leaves64, go64, True, mtx64, layout=as_list)
    assert torch.equal(out_l.reshape(out.shape), out)
    for name, a, b in zip(NAMES[:4], g[:4], g_l[:4]):
        assert torch.equal(a, b), name
    # (view_pos [B,1,1,3]: the sum over the image of -g_pos, in the order torch takes for each shape; the rows themselves are equal above)
    assert torch.allclose(g[4], g_l[4], rtol=1e-5, atol=1e-6 * float(g[4].abs().max()))

    def sliced(leaves):
        pos, n, kd, ks, view = leaves
        all_tex = torch.cat((kd, ks, torch.zeros_like(kd)), -1)
        assert all_tex[..., 3:6].stride(2) == 9
        return [pos, n, all_tex[..., 0:3], all_tex[..., 3:6], view]

    out_s, g_s = _device_run(True, spec64, dif64, leaves64, go64, True, mtx64, layout=sliced)
    assert torch.equal(out_s, out) and all(torch.equal(a, b) for a, b in zip(g[:5], g_s[:5]))
    # a partial tile row and W < 8 against their list forms
    for frame_name in ("1x9x8", "3x5x7"):
        spec64, dif64, leaves64, mtx64, near, go64 = _case("a_8_4_2", frame_name, "full", "none", True, seed=6)
        out, g = _device_run(True, spec64, dif64, leaves64, go64, True, None)
        out_l, g_l = _device_run(True, spec64, dif64, leaves64, go64, True, None, layout=as_list)
        assert torch.equal(out_l.reshape(out.shape), out) and all(torch.equal(a, b) for a, b in zip(g[:5], g_l[:5])), frame_name


def test_degenerate_vectors_give_the_statements_values():
    """A zero gb_normal and view_pos == gb_pos: the statements' values, zeros where they give zeros, no NaN unless they give one."""
    spec64, dif64 = C.light("b_64_32_16")
    leaves64 = C.frame((1, 1, 64), 9, "full")
    leaves64[1][0, 0, :16] = 0  # zero normals
    leaves64[4][0, 0, 8:24] = leaves64[0][0, 0, 8:24]  # the camera on the surface point (rows 8..15: both)
    go64 = torch.ones(1, 1, 64, 3, dtype=torch.float64)
    for specular in (True, False):
        out32, g32 = _device_run(False, spec64, dif64, leaves64, go64, specular, None)
        outh, gh = _device_run(True, spec64, dif64, leaves64, go64, specular, None)
        for name, a, b in zip(("values",) + NAMES, [outh] + gh[:5], [out32] + g32[:5]):
            assert torch.equal(torch.isnan(a), torch.isnan(b)), (name, specular)
            assert bool((a[b == 0] == 0).all()), (name, specular)
            fin = torch.isfinite(b)
            assert torch.allclose(a[fin], b[fin], rtol=1e-4, atol=1e-5 * float(b[fin].abs().max() + 1)), (name, specular)


def test_roughness_exactly_on_a_kink_takes_autograds_side():
    """Roughness exactly at float32 lo, hi, 1.0, 0 and 1.5: g_ks.y is zero where the statements' is zero and not zero where theirs
    stands clear of rounding noise (1e-5 of the largest): both decide on the same float32 numbers."""
    spec64, dif64 = C.light("c_64_to_4")
    values = (C.LO32, C.HI32, 1.0, 0.0, 1.5)
    leaves64 = C.frame((1, 1, 5 * 40), 13)
    for i, r in enumerate(values):
        leaves64[3][0, 0, i * 40:(i + 1) * 40, 1] = r
    go64 = torch.randn(1, 1, 200, 3, generator=C._gen(14), dtype=torch.float64).float().double()
    _, g32 = _device_run(False, spec64, dif64, leaves64, go64, True, None)
    _, gh = _device_run(True, spec64, dif64, leaves64, go64, True, None)
    a, b = gh[3][0, 0, :, 1], g32[3][0, 0, :, 1]
    clear = b.abs() > 1e-5 * float(b.abs().max())
    for i, r in enumerate(values):
        s = slice(i * 40, (i + 1) * 40)
        print(f"roughness {r}: statements zero {int((b[s] == 0).sum())} / clear {int(clear[s].sum())} of 40, kernel zero {int((a[s] == 0).sum())}")
    assert bool((a[b == 0] == 0).all()) and bool((a[clear] != 0).all())
    # lo and hi carry a gradient (the closed interval); at 1.0 the level sits on the top (both slots the same level) and the FG row is the
    # table's last, at 0 and 1.5 both clamps are shut: exactly zero
    assert int(clear[:80].sum()) >= 72 and bool((a[80:] == 0).all())
    assert torch.allclose(a, b, rtol=1e-3, atol=1e-4 * float(b.abs().max()))


def test_one_launch_each_way_and_none_for_an_empty_list():
    ops, light, L = _mods()
    spec64, dif64, leaves64, mtx64, near, go64 = _case("b_64_32_16", "list65", "full", "one", True, seed=3)
    lgt = _device_light(spec64, dif64)
    lgt.xfm(mtx64.float().cuda())
    leaves = [t.float().cuda().requires_grad_(True) for t in leaves64]
    with L.KernelTimer() as t:
        out = lgt.shade(*leaves)
        out.sum().backward()
    assert {k: len(v) for k, v in t.records.items()} == {"a3d_env_shade_fwd": 1, "a3d_env_shade_bwd": 1}
    assert all(x.grad is not None for x in leaves + [lgt.diffuse] + lgt.specular)
    empty = [x.detach()[:, :, :0].requires_grad_(True) for x in leaves]
    with L.KernelTimer() as t:
        out = lgt.shade(*empty)
        assert tuple(out.shape) == (1, 1, 0, 3) and out.grad_fn is not None
        g = torch.autograd.grad(out.sum(), empty + [lgt.diffuse], allow_unused=True)
    assert not t.records and tuple(g[0].shape) == (1, 1, 0, 3) and float(g[5].abs().max()) == 0.0


def test_everything_else_takes_the_statements():
    ops, light, L = _mods()
    spec64, dif64, leaves64, mtx64, near, go64 = _case("b_64_32_16", "3x5x7", "image", "none", True, seed=3)
    leaves = [t.float().cuda() for t in leaves64]

    def launched(lgt, args, **kw):
        with L.KernelTimer() as t:
            lgt.shade(*args, **kw)
        return set(t.records)

    lgt = _device_light(spec64, dif64, grad=False)
    assert launched(lgt, leaves) == {"a3d_env_shade_fwd"}
    light.HIP_ENV_SHADE = False
    assert "a3d_env_shade_fwd" not in launched(lgt, leaves) and "a3d_texture_fwd[C3]" in launched(lgt, leaves)
    light.HIP_ENV_SHADE = True
    assert "a3d_env_shade_fwd" not in launched(lgt, [t.double() for t in leaves])
    two = _device_light(spec64[1:], dif64, grad=False)
    assert "a3d_env_shade_fwd" not in launched(two, leaves)
    lgt.xfm(torch.eye(4, device="cuda")[None].requires_grad_(True))  # a transform that wants a gradient
    assert "a3d_env_shade_fwd" not in launched(lgt, leaves)
    lgt.xfm(torch.eye(4, device="cuda")[None].expand(2, 4, 4))  # neither 1 nor B = 3
    with pytest.raises(ValueError, match="lookup transform must be"):
        lgt.shade(*leaves)
    lgt.xfm(None)
    # argument errors: the shapes in Python, the rest through the ABI
    with pytest.raises(ValueError, match=r"\[6, S, S, 3\]"):
        ops.env_shade(lgt.diffuse[..., :2], lgt.specular, light._fg_lut("cuda"), *leaves)
    with pytest.raises(L.A3DError, match="at least 3 specular levels"):
        ops.env_shade(lgt.diffuse, lgt.specular[:2], light._fg_lut("cuda"), *leaves)
    with pytest.raises(L.A3DError, match="halving rule"):
        ops.env_shade(lgt.diffuse, [lgt.specular[0], lgt.specular[2], lgt.specular[2]], light._fg_lut("cuda"), *leaves)
