"""The background's gradient from the fused compositor (a3d_ca_buffer.g_null at spp 1: ca_bg_dense_kernel + ca_bg_records_kernel in
csrc/antialias.hip, ops.composite_antialias / ops.shade_composite_antialias with a background that requires grad, render_mesh under
render.FUSED_BACKGROUND_GRAD) on hand-made 16 x 16 frames with B = 2, in the style of tests/aa_cases.py (its Scene builds them).

Reference.  float64 autograd through the dense statement: torch.lerp(background, [value, 1], coverage) followed by the float64
antialias of tests/aa_ref.py (``BgRows``: an aa_ref.Buffer whose background is a leaf, evaluated by aa_ref.evaluate GIVEN the float32
decisions like every other buffer there).  The end-to-end case compares render_mesh with the switch on against the same call with the
switch off (the torch compositor + ops.antialias).

Bound.  The one tests/test_aa_adversarial_gpu.py applies to g_vals: errors in units of 2^-24 x magnitude (aa_ref's magnitudes: the same
chain over absolute values); a kernel gets 4 x the figure the float32 evaluation of the restatement reaches on that run and quantity
plus 4 ulp of the float64 value, no element left out (aa_ref.bad_elements).  aa_ref.MEASURED tabulates those figures for the runs of
tests/aa_cases.py; for the runs of this file the float32 evaluation is made here, once per run, beside the float64 one.
End to end both sides are float32 and no float64 value exists: each side is granted that bound against the truth, so the two may differ
by twice it, with the figure the largest one aa_ref.MEASURED holds for the quantity's kind on the 16 x 16 compositor runs
('checker_16x16:rows*': out for the images, g_vals for the field outputs and the background, g_clip for the vertex positions) and the
tensor's largest absolute value as every element's magnitude (a sum's magnitude is at least its largest term).

Exact where the design says so: without a covered pixel g_bg IS the incoming gradient (summed over the images for a shared
background); under a full-screen quad it is exactly zero and g_vals / g_clip are the bits of the same call with a constant background;
padding rows come back zero.
"""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aa_cases as K  # noqa: E402
import aa_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu
B, H, W = 2, 16, 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("3danimals_amd.ops")


# ---------------------------------------------------------------------------------------------------------------- scenes
def _inside(tri_px, x, y):
    """Pixel centre (x + 0.5, y + 0.5) strictly inside the triangle ``tri_px`` [3,2] (either winding)."""
    p = np.array([x + 0.5, y + 0.5])
    s = [np.cross(tri_px[(k + 1) % 3] - tri_px[k], p - tri_px[k]) for k in range(3)]
    return all(v > 0 for v in s) or all(v < 0 for v in s)


# one triangle per image, corners on the 1/32 lattice (float32 and float64 decide alike), every edge crossing pixel pairs against the
# background at all slopes; image 1's is another triangle of the same (shared) clip tensor
TRIANGLES = (np.array([[2.25, 1.5], [13.75, 5.25], [5.5, 14.25]]), np.array([[12.5, 2.25], [14.25, 12.75], [1.75, 9.5]]))


@functools.lru_cache(maxsize=None)
def scene(name):
    s = K.Scene(B, H, W)
    if name == "empty":  # a triangle nobody owns: no covered pixel, no candidate pair
        s.add(TRIANGLES[0])
    elif name == "quad":  # two triangles sharing the diagonal, far larger than the frame: every pixel covered, the diagonal no silhouette
        v = [s.vertex(p) for p in ((-8.0, -8.0), (24.0, -8.0), (24.0, 24.0), (-8.0, 24.0))]
        t0 = s.add([None] * 3, share=(v[0], v[1], v[2]))
        t1 = s.add([None] * 3, share=(v[0], v[2], v[3]))
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    s.own(b, y, x, t0 if x > y else t1)
    else:
        assert name == "triangle", name
        for b, t in enumerate(TRIANGLES):
            tid = s.add(t)
            for y in range(H):
                for x in range(W):
                    if _inside(t, x, y):
                        s.own(b, y, x, tid)
    return s.finish(f"{name}_{H}x{W}", True)


@functools.lru_cache(maxsize=None)
def decided(name):
    c = scene(name)
    return A.decide(c["rast"], c["clip"], c["tri"], dtype=A.F32)


class BgRows(A.Buffer):
    """aa_ref's 'rows' buffer with the background as a second LEAF, composited by the dense statement: lerp(background, [value, 1],
    coverage) over dense images (render.py:261-262), then the antialias callable."""

    def __init__(self, g, vals, bg, keep=None):
        super().__init__("rows", g, vals=vals, bg=bg, keep=keep)
        self.leaves = ("vals", "bg")

    def image(self, leaves, case, aa, dtype, mag=False):
        rast = case["rast"]
        vals, bg, pix = leaves["vals"], leaves["bg"], A.covered_list(rast)
        P, C = pix.shape[0], vals.shape[1]
        rows = torch.cat([vals[:P], torch.ones(P, 1, dtype=dtype)], 1)
        shaded = torch.zeros(B * H * W, C + 1, dtype=dtype).index_copy(0, pix, rows).view(B, H, W, C + 1)
        coverage = (rast[..., 3:4] > 0).to(dtype)
        pre = torch.lerp(A._padded(bg, (B, H, W, C + 1), dtype), shaded, coverage)
        return aa(pre)[..., :(C + 1 if self.kw["keep"] is None else self.kw["keep"])]


def spec(C=3, keep=None, bg_batch=B, bg_channels=None, ask=True, pad=0, live=None, dead=False):
    """One buffer of a run.  ``bg_channels`` None: C + 1; ``ask``: the background requires grad; ``live``: leading channels of the
    handed-out image whose upstream gradient is not zero (the consumer sliced them: None = all); ``dead``: nobody differentiates the
    image (its gradient does not arrive at all)."""
    return dict(C=C, keep=keep, bg_batch=bg_batch, bg_channels=C + 1 if bg_channels is None else bg_channels, ask=ask, pad=pad, live=live, dead=dead)


RUNS = {
    "empty:own": ("empty", [spec()]),
    "empty:shared": ("empty", [spec(bg_batch=1)]),
    "quad:own": ("quad", [spec()]),
    "triangle:own": ("triangle", [spec()]),
    "triangle:shared": ("triangle", [spec(bg_batch=1)]),
    "triangle:rgb_under_rgba": ("triangle", [spec(bg_channels=3)]),  # the reference's 3-channel background of a 4-channel image
    "triangle:keep_cuts_alpha": ("triangle", [spec(ask=False), spec(C=16, keep=16, bg_channels=17)]),
    "triangle:sliced_gradient": ("triangle", [spec(bg_batch=1), spec(C=16, keep=16, bg_channels=5, live=7)]),
    "triangle:one_output_unused": ("triangle", [spec(), spec(C=5, bg_batch=1, dead=True)]),
    "triangle:first_asks": ("triangle", [spec(), spec(C=5, ask=False)]),
    "triangle:second_asks": ("triangle", [spec(ask=False), spec(C=5, bg_batch=1)]),
    "triangle:both_ask": ("triangle", [spec(bg_batch=1, bg_channels=3), spec(C=5)]),
    "triangle:padded_rows": ("triangle", [spec(pad=3), spec(C=16, keep=16, bg_channels=17, pad=5)]),
}


@functools.lru_cache(maxsize=None)
def buffers(run):
    case, specs = RUNS[run]
    c = scene(case)
    P = int(A.covered_list(c["rast"]).shape[0])
    out = []
    for i, sp in enumerate(specs):
        g = K._gen(f"background_grad:{run}#{i}")
        k = sp["C"] + 1 if sp["keep"] is None else sp["keep"]
        up = torch.randn((B, H, W, k), generator=g)
        if sp["live"] is not None:
            up[..., sp["live"]:] = 0
        if sp["dead"]:
            up.zero_()
        vals = torch.randn((P + sp["pad"], sp["C"]), generator=g)
        bg = torch.randn((sp["bg_batch"], H, W, sp["bg_channels"]), generator=g)
        out.append(BgRows(up, vals, bg, sp["keep"]) if sp["ask"] else A.Buffer("rows", up, vals=vals, bg=bg, keep=sp["keep"]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(run):
    """(float64: name -> (value, magnitude), float32 restatement: name -> value) of a run; computed once, never modified."""
    c, d = scene(RUNS[run][0]), decided(RUNS[run][0])
    torch.set_num_threads(1)
    return A.evaluate(c, d["rec"], d["alpha"], buffers(run)), A.evaluate(c, d["rec"], d["alpha"], buffers(run), dtype=A.F32)


def within(got, run, key, what=""):
    """The bound of tests/test_aa_adversarial_gpu.py::within, the float32 restatement's figure measured here."""
    (val, mag), r32 = reference(run)[0][key], reference(run)[1][key]
    got = got.detach().cpu()
    assert got.shape == val.shape and got.dtype == torch.float32, (run, key, tuple(got.shape), tuple(val.shape))
    fig = A.units(r32, val, mag)
    u = A.units(got, val, mag) if bool(torch.isfinite(got).all()) else float("inf")
    print(f"UNITS {run}{what}: {key} {u:.3f} units (float32 restatement {fig:.3f}, bound {A.FACTOR * fig:.3f} + 4 ulp)")
    bad = A.bad_elements(got, val, mag, run, key, fig=fig)
    if bad.numel():
        i = tuple(bad[0].tolist())
        pytest.fail(f"{run}{what}: {key} outside the bound at {bad.shape[0]} elements, e.g. {i}: got {float(got[i])!r}, ref {float(val[i])!r}, "
                    f"magnitude {float(mag[i])!r} ({u:.2f} units, float32 restatement {fig:.3f})")


# ---------------------------------------------------------------------------------------------------------------- the device side
@functools.lru_cache(maxsize=None)
def device_case(name):
    ops = importlib.import_module("3danimals_amd.ops")
    c = scene(name)
    dev = torch.device("cuda:0")
    rast, clip, tri = c["rast"].to(dev), c["clip"].to(dev), c["tri"].to(dev).int().contiguous()
    pix, inv = ops.covered_pixels(rast, return_inverse=True)
    want = A.covered_list(c["rast"])
    assert torch.equal(torch.sort(pix.cpu()).values, want), name
    analysis = ops.AAAnalysis(rast, clip, ops.AATopology(tri, c["clip"].shape[-2]))
    return dict(rast=rast, clip=clip, tri=tri, pix=pix, inv=inv, rank=torch.searchsorted(want, pix.cpu()), analysis=analysis)


def to_device_rows(t, rank, dev):
    P = rank.shape[0]
    return torch.cat([t[:P][rank], t[P:]], 0).to(dev)


def from_device_rows(t, rank):
    t = t.detach().cpu()
    out = t.clone()
    out[rank] = t[:rank.shape[0]]
    return out


def execute(run, ops, dev, how="plain", constant_bg=False):
    """One forward and backward of a run through ops.composite_antialias: name -> tensor as aa_ref.evaluate names them.  ``how``: the
    upstream gradient arrives 'plain' (contiguous), as a channel 'slice' of a wider image (pixel stride K + 3), or through 'permute':
    the image goes on channels-first and, where the spec says so, only its leading channels are used -- the engine then hands back a
    zero-padded channels-first tensor.  ``constant_bg``: the same call with backgrounds that do not require grad."""
    S, bufs, specs = device_case(RUNS[run][0]), buffers(run), RUNS[run][1]
    clip = S["clip"].clone().requires_grad_(True)
    vals = [to_device_rows(b.kw["vals"], S["rank"], dev).requires_grad_(True) for b in bufs]
    bgs = [b.kw["bg"].to(dev).requires_grad_(sp["ask"] and not constant_bg) for b, sp in zip(bufs, specs)]
    second = dict(vals2=vals[1], background2=bgs[1], keep2=bufs[1].kw["keep"]) if len(bufs) == 2 else {}
    outs = ops.composite_antialias(vals[0], S["pix"], S["inv"], bgs[0], clip, S["analysis"], keep=bufs[0].kw["keep"], **second)
    outs = outs if len(bufs) == 2 else (outs,)
    used, ups = [], []
    for b, sp, out in zip(bufs, specs, outs):
        if sp["dead"]:
            continue
        g = b.g.to(dev)
        if how == "permute":
            n = g.shape[3] if sp["live"] is None else sp["live"]
            used.append(out.permute(0, 3, 1, 2)[:, :n])
            ups.append(g.permute(0, 3, 1, 2)[:, :n].contiguous())
        else:
            used.append(out)
            if how == "slice":
                wide = torch.randn(g.shape[:3] + (g.shape[3] + 3,), device=dev)
                wide[..., :g.shape[3]] = g
                g = wide[..., :g.shape[3]]
                assert g.stride(2) == b.g.shape[3] + 3
            ups.append(g)
    flat = [clip] + vals + [t for t in bgs if t.requires_grad]
    grads = list(torch.autograd.grad(used, flat, ups, allow_unused=True))
    res = dict(g_clip=grads[0])
    asked = iter(grads[1 + len(bufs):])
    for i, (sp, out) in enumerate(zip(specs, outs)):
        res[f"out{i}"] = out
        gv = grads[1 + i]
        res[f"raw_g_vals{i}"] = gv
        res[f"g_vals{i}"] = from_device_rows(torch.zeros_like(vals[i]) if gv is None else gv, S["rank"])
        if sp["ask"] and not constant_bg:
            res[f"g_bg{i}"] = next(asked)
    return res


def check_run(run, ops, dev, hows=("plain",)):
    for how in hows:
        res = execute(run, ops, dev, how)
        for k in reference(run)[0]:
            within(res[k], run, k, f" ({how})")
    return res


# ---------------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("run", ["empty:own", "empty:shared"])
def test_without_a_covered_pixel_the_background_takes_the_whole_gradient(run, ops, dev):
    res = execute(run, ops, dev)
    g = buffers(run)[0].g.to(dev)
    assert device_case("empty")["pix"].shape[0] == 0
    assert torch.equal(res["out0"], buffers(run)[0].kw["bg"].to(dev).expand(B, H, W, 4))
    assert torch.equal(res["g_bg0"], g if run == "empty:own" else (g[0] + g[1])[None])  # (a shared background: image 0 first, then image 1)
    assert bool((res["g_clip"] == 0).all())
    check_run(run, ops, dev)


def test_under_a_full_screen_quad_the_background_gets_exact_zeros(ops, dev):
    run = "quad:own"
    assert decided("quad")["rec"].shape[0] == 0 and device_case("quad")["pix"].shape[0] == B * H * W
    res, const = execute(run, ops, dev), execute(run, ops, dev, constant_bg=True)
    assert res["g_bg0"].shape == (B, H, W, 4) and bool((res["g_bg0"] == 0).all())
    assert torch.equal(res["raw_g_vals0"], const["raw_g_vals0"]) and torch.equal(res["g_clip"], const["g_clip"]) and torch.equal(res["out0"], const["out0"])
    check_run(run, ops, dev)


# ---------------------------------------------------------------------------------------------------------------- against float64
def test_the_triangle_scene_has_records_on_every_side():
    """The scene is what the cases below need: both images have crossing records with the background as source and as destination, right
    and lower pairs, and uncovered pixels that no record touches."""
    c, d = scene("triangle"), decided("triangle")
    u = A.unpack(d["rec"], H, W)
    cov = (c["rast"][..., 3] > 0).reshape(-1)
    dst = A.destinations(d["rec"], d["alpha"], W)
    assert d["rec"].shape[0] >= 40 and set(u["b"].tolist()) == {0, 1} and set(u["d"].tolist()) == {0, 1}
    assert bool((~cov[dst]).any()) and bool(cov[dst].any()) and bool((cov[u["pix0"]] != cov[u["p1"]]).all())
    touched = torch.zeros(B * H * W, dtype=torch.bool)
    touched[u["pix0"]] = True
    touched[u["p1"]] = True
    assert bool((~cov & ~touched).any()) and 0 < int(cov.sum()) < B * H * W


@pytest.mark.parametrize("run", ["triangle:own", "triangle:shared", "triangle:rgb_under_rgba", "triangle:keep_cuts_alpha"])
def test_one_triangle_against_the_background(run, ops, dev):
    """g_bg, g_vals, g_clip and the image against float64: a background per image, one shared by both (summed over the images), the
    3-channel background of a 4-channel image, and ``keep`` cutting the alpha channel of a 16-channel second buffer."""
    res = check_run(run, ops, dev, ("plain", "slice"))
    g_bg = res[f"g_bg{len(RUNS[run][1]) - 1}"]
    # a background pixel that is covered in every image that reads it: exactly zero (the dense pass writes it, no record adds to it)
    cov = (scene("triangle")["rast"][..., 3] > 0).to(dev)
    cov = cov if g_bg.shape[0] == B else (cov[0] & cov[1])[None]
    assert bool(cov.any()) and bool((g_bg[cov] == 0).all()) and bool((g_bg[~cov] != 0).any())


def test_a_channel_sliced_strided_gradient(ops, dev):
    """The image goes on through permute(0, 3, 1, 2) and a channel slice (7 of the 16 channels of the second buffer, whose background has
    5): the gradient arrives zero-padded and channels-first -- and, in the other execution, as a slice of a wider image read in place."""
    check_run("triangle:sliced_gradient", ops, dev, ("permute", "slice"))


def test_an_output_nobody_differentiated(ops, dev):
    """g_out = None for the second of two outputs: its background's gradient (it asked) and its rows' are zeros, the first buffer's are
    those of the float64 reference with a zero upstream gradient there."""
    run = "triangle:one_output_unused"
    res = check_run(run, ops, dev)
    assert res["g_bg1"].shape == (1, H, W, 6) and bool((res["g_bg1"] == 0).all()) and bool((res["g_vals1"] == 0).all())


@pytest.mark.parametrize("run", ["triangle:first_asks", "triangle:second_asks", "triangle:both_ask"])
def test_two_buffers_ask_independently(run, ops, dev):
    res = check_run(run, ops, dev, ("plain", "permute"))
    assert [k for k in ("g_bg0", "g_bg1") if k in res] == {"triangle:first_asks": ["g_bg0"], "triangle:second_asks": ["g_bg1"],
                                                            "triangle:both_ask": ["g_bg0", "g_bg1"]}[run]
    # the buffers' own gradients do not depend on who asks: the same call with constant backgrounds, to the order of its atomics
    const = execute(run, ops, dev, constant_bg=True)
    for k in ("g_vals0", "g_vals1", "g_clip", "out0", "out1"):
        within(const[k], run, k, " (constant backgrounds)")


def test_padded_rows_keep_a_zero_gradient(ops, dev):
    run = "triangle:padded_rows"
    res = check_run(run, ops, dev)
    P = device_case("triangle")["pix"].shape[0]
    for i, pad in ((0, 3), (1, 5)):
        g = res[f"raw_g_vals{i}"]
        assert g.shape[0] == P + pad and bool((g[P:] == 0).all()) and bool((g[:P] != 0).any())


def test_the_shaded_source_with_a_differentiable_background(ops, dev):
    """ops.shade_composite_antialias: the colour computed inside the launches, the background [B,H,W,3] (what render_mesh hands over)
    requiring grad, a 16-channel second buffer whose background asks too.  Reference: the float64 statement over the colours the
    stand-alone shading launch gives for the same recipe (the compositor's are the same bits: one shared device function)."""
    S, c, d = device_case("triangle"), scene("triangle"), decided("triangle")
    P = S["pix"].shape[0]
    g = K._gen("background_grad:shaded")
    rnd = lambda *shape: torch.randn(shape, generator=g)
    gb = torch.cat((rnd(P, 3), torch.nn.functional.normalize(rnd(P, 3), dim=-1), rnd(P, 6)), -1).to(dev).requires_grad_(True)
    w2c = (torch.eye(4)[None].repeat(B, 1, 1) + 0.2 * torch.nn.functional.pad(rnd(B, 3, 3), (0, 1, 0, 1))).to(dev)
    view, tex = rnd(B, 3).to(dev), torch.rand((P + 4, 5), generator=g).to(dev).requires_grad_(True)
    light = torch.cat((torch.nn.functional.normalize(rnd(B, 3), dim=-1), torch.rand((B, 2), generator=g) * 0.6 + 0.2), -1).to(dev)
    img = torch.div(S["pix"], H * W, rounding_mode="floor")
    bg, bg2 = rnd(B, H, W, 3).to(dev).requires_grad_(True), rnd(1, H, W, 17).to(dev).requires_grad_(True)
    vals2 = to_device_rows(rnd(P, 16), S["rank"], dev).requires_grad_(True)
    ups = [rnd(B, H, W, 4), rnd(B, H, W, 16)]
    clip = S["clip"].clone().requires_grad_(True)
    recipe = ops.ShadeRecipe(gb, w2c, view, light, tex, True, img)
    outs = ops.shade_composite_antialias(recipe, S["pix"], S["inv"], bg, clip, S["analysis"], vals2=vals2, background2=bg2, keep2=16)
    g_bg, g_bg2, g_vals2, g_clip, g_gb, g_tex = torch.autograd.grad(list(outs), [bg, bg2, vals2, clip, gb, tex], [u.to(dev) for u in ups])
    with torch.no_grad():
        colour = ops.ShadeRecipe(gb.detach(), w2c, view, light, tex.detach(), True, img).materialize()[2]
    bufs = (BgRows(ups[0], from_device_rows(colour, S["rank"]), bg.detach().cpu()),
            BgRows(ups[1], from_device_rows(vals2, S["rank"]), bg2.detach().cpu(), keep=16))
    torch.set_num_threads(1)
    r64, r32 = A.evaluate(c, d["rec"], d["alpha"], bufs), A.evaluate(c, d["rec"], d["alpha"], bufs, dtype=A.F32)
    got = dict(out0=outs[0], out1=outs[1], g_bg0=g_bg, g_bg1=g_bg2, g_vals1=from_device_rows(g_vals2, S["rank"]), g_clip=g_clip)
    for k, t in got.items():
        (val, mag), t = r64[k], t.detach().cpu()
        fig = A.units(r32[k], val, mag)
        print(f"UNITS shaded source: {k} {A.units(t, val, mag):.3f} units (float32 restatement {fig:.3f})")
        bad = A.bad_elements(t, val, mag, None, k, fig=fig)
        assert not bad.numel(), (k, bad.shape[0], tuple(bad[0].tolist()), A.units(t, val, mag), fig)
    assert bool(torch.isfinite(g_gb).all()) and bool(torch.isfinite(g_tex).all()) and bool((g_tex[P:] == 0).all()) and bool((g_gb != 0).any())


# ---------------------------------------------------------------------------------------------------------------- end to end, refusals
class _Tap:
    """A field network whose sample() output is kept: the test differentiates with respect to it."""

    def __init__(self, net):
        self.net, self.outs = net, []

    def __getattr__(self, name):
        return getattr(self.net, name)

    def sample(self, *a, **kw):
        self.outs.append(self.net.sample(*a, **kw))
        return self.outs[-1]


def _figure(kind):
    return max(v[k] for run, v in A.MEASURED.items() if run.startswith("checker_16x16:rows") for k in v if k.startswith(kind))


def test_render_mesh_with_the_switch_on_against_the_generic_path(ops, dev, monkeypatch):
    """['shaded', 'dino_pred'] with a background that requires grad, 2 images of 16 x 16: the route with the switch on is 'covered' with
    the fused compositor (whose backward then runs: its timer key appears); images and the gradients of the background, the vertex
    positions and the two fields' output rows agree with the switch-off call within twice the compositor bound (module docstring)."""
    pipeline = importlib.import_module("3danimals_amd.pipeline")
    render = importlib.import_module("3danimals_amd.model.render.render")
    _lib = importlib.import_module("3danimals_amd._lib")
    scene_ = pipeline.SyntheticScene(grid_res=8, batch=B, resolution=(H, W), device=dev, seed=2, net_width=32, net_layers=3, feat_dim=16, embedder_freq=4)
    with torch.no_grad():
        scene_.step(backward=False)
    prior = scene_.last["prior"]
    mvp, w2c, campos, feat = (t.detach() for t in (scene_.mvp, scene_.w2c, scene_.campos, scene_.feat))
    gen = K._gen("background_grad:render_mesh")
    bg0 = torch.rand((B, H, W, 3), generator=gen).to(dev)
    ups = [torch.randn((B, 4, H, W), generator=gen).to(dev), torch.randn((B, 16, H, W), generator=gen).to(dev)]
    modes = ["shaded", "dino_pred"]

    def run(switch):
        monkeypatch.setattr(render, "FUSED_BACKGROUND_GRAD", switch)
        verts = scene_.last["shape"].v_pos.detach().clone().requires_grad_(True)
        bg = bg0.clone().requires_grad_(True)
        mesh_mod = importlib.import_module("3danimals_amd.model.render.mesh")
        uvs = torch.rand(1, verts.shape[1], 2, generator=torch.Generator().manual_seed(5)).to(dev)
        shape = mesh_mod.make_mesh(verts, prior.t_pos_idx, uvs.expand(verts.shape[0], -1, -1), prior.t_pos_idx, None)
        tex, dino = _Tap(scene_.netTexture), _Tap(scene_.netDINO)
        route = render._plan_route(modes, shape, w2c, (H, W), 1, 1, False, bg, tex, scene_.netLight, dino, mtx=mvp, num_frames=1)
        timer = _lib.KernelTimer()
        with timer:
            outs = render.render_mesh(None, shape, mvp, w2c, campos, tex, scene_.netLight, (H, W), spp=1, msaa=False, background=bg, bsdf="diffuse",
                                      feat=feat, render_modes=modes, prior_mesh=prior, dino_net=dino, num_frames=1)
            leaves = dict(background=bg, v_pos=verts, texture_rows=tex.outs[0], dino_rows=dino.outs[0])
            grads = torch.autograd.grad(outs, list(leaves.values()), ups)
        res = dict(shaded=outs[0].detach(), dino_pred=outs[1].detach(), **{"g_" + k: g for k, g in zip(leaves, grads)})
        return route, set(timer.records), res

    r_off, keys_off, off = run(False)
    r_on, keys_on, on = run(True)
    assert r_off.path == "covered" and not r_off.composite and not any(k.startswith("a3d_composite_aa") for k in keys_off), (r_off, keys_off)
    assert r_on.path == "covered" and r_on.composite and any(k.startswith("a3d_composite_aa_bwd") for k in keys_on), (r_on, keys_on)
    cover = render.LAST_RAST[0][..., 3] > 0
    assert 0 < int(cover.sum()) < B * H * W
    kinds = dict(shaded="out", dino_pred="out", g_background="g_vals", g_texture_rows="g_vals", g_dino_rows="g_vals", g_v_pos="g_clip")
    failed = []
    for k, kind in kinds.items():
        a, b = on[k].double().cpu(), off[k].double().cpu()
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), k
        fig, scale = _figure(kind), float(b.abs().max())
        bound = 2.0 * A.EPS * (A.FACTOR * fig * scale + 4.0 * b.abs())
        worst = float(((a - b).abs() / (A.EPS * max(scale, 1e-300))).max())
        print(f"UNITS render_mesh: {k} differs by at most {worst:.3f} units of 2^-24 x {scale:.3e} (figure {fig}, allowed {2 * A.FACTOR * fig:.3f} + 8 ulp)")
        if not bool(((a - b).abs() <= bound).all()):
            failed.append((k, worst))
    assert not failed, failed
    assert bool((on["g_background"] != 0).any())


def test_supersampled_and_mask_calls_refuse_a_background_that_requires_grad(ops, dev):
    """msaa_composite_antialias and mask_antialias raise, with a message that names where such a call goes, and launch nothing."""
    _lib = importlib.import_module("3danimals_amd._lib")
    S = device_case("triangle")
    P = S["pix"].shape[0]
    vals, null = torch.rand(P, 3, device=dev), torch.rand(B, 3, device=dev)
    timer = _lib.KernelTimer()
    with timer:
        with pytest.raises(AssertionError, match="msaa_composite_antialias.*generic path"):
            ops.msaa_composite_antialias(vals, null, S["pix"], S["inv"], S["rast"], torch.rand(B, H // 2, W // 2, 4, device=dev).requires_grad_(True),
                                         S["clip"], S["analysis"], 2)
        with pytest.raises(AssertionError, match="msaa_composite_antialias.*generic path"):
            ops.msaa_composite_antialias(vals, null, S["pix"], S["inv"], S["rast"], None, S["clip"], S["analysis"], 2, vals2=vals, null_vals2=null,
                                         background2=torch.rand(1, H // 2, W // 2, 4, device=dev).requires_grad_(True))
        with pytest.raises(AssertionError, match="mask_antialias.*composite_antialias"):
            ops.mask_antialias(S["rast"], S["clip"], torch.rand(B, H, W, 4, device=dev).requires_grad_(True), S["analysis"])
    assert not timer.records, sorted(timer.records)
