"""render_mesh's routes on the GPU: what render._plan_route says a call does against the entry points that ran, and every route's launch
record against the parent commit's (tests/golden/render_routes.json: names, tags and counts, recorded by tools/render_routes.py).

Scene: _render_scene of test_depth_tangent_gpu (B = 2, the golden nets); frames of 32 x 32 unless the case says otherwise.  Every case runs
forward + backward twice under _lib.KernelTimer and the SECOND run is looked at: the first one fills the topology caches and gives the
deferred resolve a list length to allocate for.  run_case is also what the driver runs under the parent's package, so it asks the package
for nothing this commit added.
"""
import copy
import importlib
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN, seeded  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN_ROUTES = os.path.join(GOLDEN, "render_routes.json")

MODE_LISTS = [["shaded"], ["shaded", "dino_pred"], ["shaded", "flow"], ["shaded", "depth"], ["tangent"], ["tangent", "flow"],
              ["kd", "normal", "geo_normal", "shading"]]
CASES = {"+".join(m): dict(modes=m) for m in MODE_LISTS}
CASES.update({
    "msaa2_fused_msaa_on": dict(modes=["shaded", "dino_pred"], spp=2, msaa=True, switches=dict(FUSED_MSAA=True)),
    "msaa2_fused_msaa_off": dict(modes=["shaded", "dino_pred"], spp=2, msaa=True, switches=dict(FUSED_MSAA=False)),
    "layers2": dict(modes=["shaded", "dino_pred"], num_layers=2),
    "background_grad": dict(modes=["shaded", "dino_pred"], background="grad"),
    "w2c_grad": dict(modes=["shaded", "depth"], w2c_grad=True),
    "30x50": dict(modes=["shaded", "dino_pred"], res=(30, 50)),
    "mask": dict(modes=["shaded"], nets=False, background="plain"),
})
CASES.update({name + "_off": dict(modes=["shaded", "dino_pred"], switches={name: False})
              for name in ("FUSED_GBUFFER", "FUSED_COVER_GBUFFER", "DEFER_RESOLVE", "FUSED_COMPOSITE", "SHADE_IN_COMPOSITOR", "ALIAS_POSITIONS")})
SWITCH_DEFAULTS = dict(FUSED_MSAA=False, FUSED_DEPTH_TANGENT=True, FUSED_GBUFFER=True, FUSED_COVER_GBUFFER=True, DEFER_RESOLVE=True, FUSED_COMPOSITE=True,
                       SHADE_IN_COMPOSITOR=True, ALIAS_POSITIONS=True)  # (what a case does not name: the shipped setting, whatever the environment says)


def make_scene(dev):
    from test_depth_tangent_gpu import _render_scene

    return _render_scene(dev)


def run_case(R, scene, case, dev):
    """One forward + backward of ``case`` -> (named outputs, named gradients).  Like _render of test_depth_tangent_gpu, with what that one
    has no argument for: a frame that is not square, no nets, a background, gradients beyond the vertices'."""
    M, verts, faces, uvs, mvp, w2c, campos, nets, feat = scene
    B, res = mvp.shape[0], case.get("res", (32, 32))
    tex, dino, lgt = (copy.deepcopy(m).to(dev) for m in nets) if case.get("nets", True) else (None, None, None)
    v_pos = (verts[None].expand(B, -1, -1) + 0.002 * seeded((B, *verts.shape), 63, -1, 1).to(dev)).contiguous().requires_grad_(True)
    shape = M.make_mesh(v_pos, faces[None], uvs.expand(B, -1, -1), faces[None], None)
    prior = M.make_mesh(verts[None], faces[None], uvs, faces[None], None)
    w2c = w2c.clone().requires_grad_(True) if case.get("w2c_grad") else w2c
    background = None
    if case.get("background"):
        background = seeded((B, res[0], res[1], 3), 65, 0, 1).to(dev).requires_grad_(case["background"] == "grad")
    previous = {k: getattr(R, k) for k in SWITCH_DEFAULTS}
    try:
        for k, v in {**SWITCH_DEFAULTS, **case.get("switches", {})}.items():
            setattr(R, k, v)
        outs = R.render_mesh(None, shape, mvp, w2c, campos, tex, lgt, res, spp=case.get("spp", 1), num_layers=case.get("num_layers", 1),
                             msaa=case.get("msaa", False), background=background, bsdf="diffuse", feat=feat, render_modes=case["modes"], prior_mesh=prior,
                             dino_net=dino, num_frames=2 if "flow" in case["modes"] else None)
        sum((o * seeded(tuple(o.shape), 64 + i, -1, 1).to(dev)).sum() for i, o in enumerate(outs)).backward()
    finally:
        for k, v in previous.items():
            setattr(R, k, v)
    grads = {"v_pos": v_pos.grad, "w2c": w2c.grad, "background": None if background is None else background.grad}
    for name, net in (("tex", tex), ("dino", dino), ("lgt", lgt)):
        if net is not None:
            grads.update({f"{name}.{n}": p.grad for n, p in net.named_parameters()})
    return dict(zip(case["modes"], (o.detach() for o in outs))), {k: g for k, g in grads.items() if g is not None}


def launch_record(L, R, scene, case, dev):
    """-> ([[entry point + tag, launches], ...] in the order of first appearance, outputs, gradients) of the second of two runs."""
    run_case(R, scene, case, dev)
    with L.KernelTimer() as timer:
        outs, grads = run_case(R, scene, case, dev)
    torch.cuda.synchronize()
    return [[key, len(pairs)] for key, pairs in timer.records.items()], outs, grads


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    dev = torch.device("cuda:0")
    mods = [importlib.import_module("3danimals_amd" + m) for m in ("._lib", ".model.render.render", ".ops")]
    return dev, mods, make_scene(dev), json.load(open(GOLDEN_ROUTES))


@pytest.mark.parametrize("name", list(CASES))
def test_route_record_matches_the_launches_and_the_parents_record(name, env, monkeypatch):
    dev, (L, R, ops), scene, golden_routes = env
    case = CASES[name]
    planned = []
    real = R._plan_route
    monkeypatch.setattr(R, "_plan_route", lambda *a, **k: (planned.append(real(*a, **k)), planned[-1])[1])
    run_case(R, scene, case, dev)
    del planned[:]
    standalone = ops.resolve_events["standalone"]
    with L.KernelTimer() as timer:
        run_case(R, scene, case, dev)
    torch.cuda.synchronize()
    record = [[key, len(pairs)] for key, pairs in timer.records.items()]
    route = planned[0]  # render_mesh's own (a layer that was handed the route plans nothing)
    assert len(planned) == 1, planned
    print(name, route, record)
    ran = lambda entry: sum(n for key, n in record if key == entry or key.startswith(entry + "["))
    antialiased = [m for m in case["modes"] if m in R.ANTIALIASED_MODES]

    # (a) the planner against what ran
    rast_keys = [key for key, _ in record if key.startswith("a3d_rast_fwd")]
    assert rast_keys and all(("[defer]" in key) == route.defer for key in rast_keys), (route, rast_keys)
    assert (ran("a3d_rast_resolve_gbuffer_fwd") > 0) == route.defer, route
    if route.defer:
        assert ops.resolve_events["standalone"] == standalone and ran("a3d_rast_resolve") == 0, route
    assert (ran("a3d_cover_gbuffer_fwd") > 0) == (route.one_launch and not route.defer), route
    two_launches = route.covered_points and not route.one_launch
    assert (ran("a3d_cover_emit") > 0) == two_launches and (ran("a3d_gbuffer_fwd") > 0) == two_launches, route
    if route.composite and route.path == "covered" and antialiased:
        assert ran("a3d_composite_aa_fwd") > 0 and ran("a3d_aa_fwd") == 0, route
    if not route.composite and route.path != "mask" and antialiased:
        assert ran("a3d_composite_aa_fwd") == 0 and ran("a3d_aa_fwd") > 0, route
    assert (ran("a3d_mask_aa_fwd") > 0) == (route.path == "mask"), route
    assert (ran("a3d_interp_fwd") > 0) == (route.path in ("dense", "layers")), route
    assert (ran("a3d_flow_delta_fwd") > 0) == route.flow_delta, route
    # ... and the route each case was written for
    expect = {"msaa2_fused_msaa_on": "msaa", "layers2": "layers", "mask": "mask", "msaa2_fused_msaa_off": "dense", "w2c_grad": "dense",
              "tangent+flow": "dense", "FUSED_GBUFFER_off": "dense"}.get(name, "covered")
    assert route.path == expect, route
    assert route.defer == (expect == "covered" and name not in ("30x50", "FUSED_COVER_GBUFFER_off", "DEFER_RESOLVE_off")), route
    assert route.composite == (expect == "msaa" or (expect == "covered" and name not in ("background_grad", "FUSED_COMPOSITE_off"))), route
    assert route.alias == (name not in ("ALIAS_POSITIONS_off", "msaa2_fused_msaa_on", "msaa2_fused_msaa_off", "layers2")), route

    # (b) the launch record against the parent's: any change of route shows here
    assert record == golden_routes["routes"][name], (name, record, golden_routes["routes"][name])


def test_the_golden_covers_the_matrix(env):
    golden_routes = env[3]
    assert sorted(golden_routes["routes"]) == sorted(CASES)
