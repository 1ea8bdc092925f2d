"""render._plan_route: the _Route of a call from its arguments and the module switches alone -- enumerated on the CPU, no kernel runs.

The device helper (render._on_gpu_f32) is patched to say yes, so that the planner sees CPU tensors as device float32 ones.  Factors: every
switch on / off (PIXEL_TILE 8 / 0), spp 1 / 2 / 4, msaa, one or two layers, three resolutions, seven mode lists, background none / plain /
requiring grad, w2c plain / requiring grad, material + light + DINO net present or all absent, autocast, the normal index buffer the position
one or another, tangents present / pending / absent.

Pruning (every factor stays): an argument factor is varied only under the mode lists that can see it -- w2c's grad under 'depth', the
tangents under 'tangent', the nets under ['shaded'] (the mask render's list).  The switches go (a) as all on, all off, each one alone off
and each one alone on over ALL argument combinations, and (b) as the full product of the eleven the planner reads over a smaller argument
set in which every value of every factor occurs; the five the planner never reads (they belong to later stages' arithmetic, not to the
route) take part in (a), where the per-switch check shows that they move nothing.
"""
import importlib
import itertools
import types

import pytest
import torch

R = importlib.import_module("3danimals_amd.model.render.render")

PLANNER_SWITCHES = ["FUSED_COMPOSITE", "SHADE_COVERED_ONLY", "FUSED_GBUFFER", "FUSED_COVER_GBUFFER", "DEFER_RESOLVE", "FUSED_FLOW_DELTA",
                    "FUSED_MASK_RENDER", "FUSED_MSAA", "FUSED_DEPTH_TANGENT", "ALIAS_POSITIONS", "PIXEL_TILE"]
OTHER_SWITCHES = ["DEFER_ANALYSIS", "FUSED_SHADING", "FIELD_INPUTS_FROM_GBUFFER", "SHADE_IN_COMPOSITOR", "POINT_BUCKET"]
SWITCHES = PLANNER_SWITCHES + OTHER_SWITCHES
ON = {s: True for s in SWITCHES} | {"PIXEL_TILE": 8, "POINT_BUCKET": 8192}
OFF = {s: False for s in SWITCHES} | {"PIXEL_TILE": 0, "POINT_BUCKET": 0}
MODE_LISTS = [["shaded"], ["shaded", "dino_pred"], ["shaded", "flow"], ["shaded", "depth"], ["tangent"], ["tangent", "flow"],
              ["kd", "normal", "geo_normal", "shading"]]
RESOLUTIONS = [(32, 32), (30, 50), (8, 8)]
B, V, NUM_FRAMES = 2, 5, 2
# what may come ON when a switch goes off: the path the call falls back to and what that path brings with it.  Nothing else may.
FALLS_TO_DENSE = {"path:dense"}
GOVERNS = {
    "FUSED_MSAA": FALLS_TO_DENSE, "SHADE_COVERED_ONLY": FALLS_TO_DENSE, "FUSED_GBUFFER": FALLS_TO_DENSE, "FUSED_COVER_GBUFFER": FALLS_TO_DENSE,
    "FUSED_DEPTH_TANGENT": FALLS_TO_DENSE, "PIXEL_TILE": FALLS_TO_DENSE,  # (the last three: the supersampled path needs the one-launch list)
    # the mask render becomes an ordinary ['shaded'] call: the covered-point path with its list, its deferral -- and, under
    # FUSED_MASK_RENDER, its compositor; FUSED_COMPOSITE off also sends the supersampled path and a served 'depth' to the dense path
    "FUSED_MASK_RENDER": {"path:covered", "path:dense", "one_launch", "defer", "composite"},
    "FUSED_COMPOSITE": {"path:covered", "path:dense", "one_launch", "defer"},
    "DEFER_RESOLVE": set(), "FUSED_FLOW_DELTA": set(), "ALIAS_POSITIONS": set(),
    **{s: set() for s in OTHER_SWITCHES},
}


def _mesh(nrm_shared=True, tangents="absent"):
    v_pos = torch.zeros(B, V, 3)
    t_pos = torch.zeros(1, 4, 3, dtype=torch.int32)
    m = types.SimpleNamespace(v_pos=v_pos, t_pos_idx=t_pos, t_nrm_idx=t_pos if nrm_shared else t_pos.clone(), v_tex=torch.zeros(1, V, 2),
                              _v_tng=None, _lazy_tng=False, v_tng=None, t_tng_idx=None)
    if tangents == "present":
        m._v_tng = m.v_tng = torch.zeros(B, V, 3)
        m.t_tng_idx = t_pos
    elif tangents == "pending":  # (Mesh.v_tng would compute them: the planner must not ask)
        m._lazy_tng, m.t_tng_idx = True, t_pos
        m.v_tng = "the planner asked for pending tangents"
    return m


_MESHES = {(n, t): _mesh(n, t) for n in (True, False) for t in ("present", "pending", "absent")}
_W2C = {False: torch.eye(4).repeat(B, 1, 1), True: torch.eye(4).repeat(B, 1, 1).requires_grad_(True)}
_MTX = torch.eye(4).repeat(B, 1, 1)
_NETS = object()


def _background(kind, res):
    return None if kind == "none" else torch.zeros(B, res[0], res[1], 3, requires_grad=kind == "grad")


_BG = {(k, r): _background(k, r) for k in ("none", "plain", "grad") for r in RESOLUTIONS}


def arg_sets(full):
    """-> dicts of the argument factors.  ``full``: every combination (pruned as the module docstring says); else a small set in which
    every value of every factor occurs and every path is reached."""
    out = []
    for modes, res, spp, msaa, layers, bg, autocast, nrm in itertools.product(MODE_LISTS, RESOLUTIONS, (1, 2, 4), (False, True), (1, 2),
                                                                              ("none", "plain", "grad"), (False, True), (True, False)):
        for w2c_grad in ((False, True) if "depth" in modes else (False,)):
            for tng in (("present", "pending", "absent") if "tangent" in modes else ("absent",)):
                for nets in ((True, False) if modes == ["shaded"] else (True,)):
                    out.append(dict(modes=modes, res=res, spp=spp, msaa=msaa, layers=layers, bg=bg, autocast=autocast, nrm=nrm, w2c_grad=w2c_grad,
                                    tng=tng, nets=nets))
    if full:
        return out
    base = dict(res=(32, 32), spp=1, msaa=False, layers=1, bg="none", autocast=False, nrm=True, w2c_grad=False, tng="present", nets=True)
    small = [dict(base, modes=m) for m in MODE_LISTS] + [dict(base, modes=["shaded"], nets=False), dict(base, modes=["shaded"], nets=False, bg="grad")]
    for m in (["shaded"], ["shaded", "flow"], ["shaded", "depth"], ["tangent"]):
        small += [dict(base, modes=m, spp=2, msaa=True), dict(base, modes=m, spp=4, msaa=True, bg="plain"), dict(base, modes=m, spp=2),
                  dict(base, modes=m, layers=2), dict(base, modes=m, res=(30, 50)), dict(base, modes=m, res=(8, 8), bg="plain"),
                  dict(base, modes=m, bg="grad"), dict(base, modes=m, autocast=True), dict(base, modes=m, nrm=False),
                  dict(base, modes=m, w2c_grad=True), dict(base, modes=m, tng="pending"), dict(base, modes=m, tng="absent"),
                  dict(base, modes=m, spp=2, msaa=True, res=(30, 50)), dict(base, modes=m, spp=2, msaa=True, bg="grad")]
    return small


def plan(a, autocast_flag):
    autocast_flag[0] = a["autocast"]
    nets = _NETS if a["nets"] else None
    return R._plan_route(a["modes"], _MESHES[a["nrm"], a["tng"]], _W2C[a["w2c_grad"]], a["res"], a["spp"], a["layers"], a["msaa"], _BG[a["bg"], a["res"]],
                         nets, nets, nets, mtx=_MTX, num_frames=NUM_FRAMES)


def fields(route):
    """The record as the set of what is ON in it."""
    on = {"path:" + route.path}
    on |= {f for f in ("one_launch", "defer", "composite", "alias", "flow_delta") if getattr(route, f)}
    on |= {"extra:" + route.extra} if route.extra else set()
    return on | {"served:" + m for m in route.served}


def check_invariants(route, a, sw):
    ctx = (route, a, {k: v for k, v in sw.items() if v != ON[k]})
    modes, plain_bg = a["modes"], a["bg"] != "grad"
    assert route.path in ("layers", "msaa", "mask", "covered", "dense"), ctx
    assert (route.path == "layers") == (a["layers"] != 1), ctx
    if route.path in ("covered", "mask"):  # (the point list and the mask render exist at spp 1 only, whatever DEFER_RESOLVE says)
        assert a["spp"] == 1, ctx
    if route.defer:  # a deferred resolve: the covered-point path with the one-launch list at spp 1
        assert route.path == "covered" and route.one_launch and a["spp"] == 1 and sw["DEFER_RESOLVE"], ctx
    if route.one_launch:
        assert route.covered_points and a["res"][0] % 8 == 0 and a["res"][1] % 8 == 0 and sw["PIXEL_TILE"] == 8 and sw["FUSED_COVER_GBUFFER"], ctx
    if route.path == "msaa":  # the supersampled path: its inner layer is the covered-point path, with the one-launch list, not deferred
        assert route.covered_points and route.one_launch and not route.defer and route.composite and not route.alias, ctx
        assert sw["FUSED_MSAA"] and a["msaa"] and a["spp"] in (2, 4) and plain_bg and not a["autocast"] and not route.served, ctx
    assert route.covered_points == (route.path in ("covered", "msaa")), ctx
    if not route.covered_points:
        assert not (route.one_launch or route.defer or route.extra or route.served or route.composite), ctx
    else:
        assert sw["SHADE_COVERED_ONLY"] and sw["FUSED_GBUFFER"] and a["nrm"], ctx
        assert route.served == frozenset(modes) & {"depth", "tangent"}, ctx  # all that are asked for; with one unserved the call is dense
    if "depth" in route.served:  # 'depth' on the covered-point path leaves as a recipe for the fused compositor
        assert route.composite and not a["w2c_grad"] and plain_bg, ctx
    if route.served:
        assert sw["FUSED_DEPTH_TANGENT"] and a["spp"] == 1 and not a["autocast"], ctx
    if route.composite:
        assert sw["FUSED_COMPOSITE"] and plain_bg, ctx
    if route.extra == "tangent":  # the launch carries ONE extra attribute
        assert "flow" not in modes and "tangent" in route.served and a["tng"] != "absent", ctx
    if route.extra == "flow":
        assert "flow" in modes and "tangent" not in route.served, ctx
    if route.covered_points:
        assert (route.extra is not None) == bool({"flow", "tangent"} & set(modes)), ctx
    # the mask-only render: exactly its conditions (and one layer)
    mask = (sw["FUSED_MASK_RENDER"] and sw["FUSED_COMPOSITE"] and not a["nets"] and list(modes) == ["shaded"] and a["spp"] == 1 and plain_bg
            and a["layers"] == 1)
    assert (route.path == "mask") == bool(mask), ctx
    if route.alias:
        assert sw["ALIAS_POSITIONS"] and a["spp"] == 1 and a["layers"] == 1 and not a["autocast"], ctx
    if route.flow_delta:
        assert sw["FUSED_FLOW_DELTA"] and "flow" in modes and not a["autocast"], ctx
    if sw == OFF:  # every switch off: the dense path or the layers, nothing deferred, nothing aliased
        assert route.path in ("dense", "layers") and fields(route) == {"path:" + route.path}, ctx


@pytest.fixture
def planner(monkeypatch):
    """The switches are set by the caller through set_switches (restored afterwards); the device helper says yes; autocast is a flag."""
    flag = [False]
    monkeypatch.setattr(R, "_on_gpu_f32", lambda t: torch.is_tensor(t))
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: flag[0])
    for s in SWITCHES:
        monkeypatch.setattr(R, s, getattr(R, s))  # (restores whatever set_switches leaves behind)
    return flag


def set_switches(sw):
    for k, v in sw.items():
        setattr(R, k, v)


def run(switch_sets, args, flag):
    routes = {}
    for key, sw in switch_sets.items():
        set_switches(sw)
        for i, a in enumerate(args):
            route = routes[key, i] = plan(a, flag)
            check_invariants(route, a, sw)
    return routes


def check_switch_off_turns_nothing_else_on(routes, pairs, n_args):
    """``pairs``: (switch, key with it on, key with it off, everything else equal)."""
    seen = {s: set() for s in SWITCHES}
    for s, k_on, k_off in pairs:
        for i in range(n_args):
            came_on = fields(routes[k_off, i]) - fields(routes[k_on, i])
            seen[s] |= came_on
            assert came_on <= GOVERNS[s], (s, came_on - GOVERNS[s], routes[k_on, i], routes[k_off, i])
    return seen


def test_every_argument_combination_under_the_single_switch_sets(planner):
    args = arg_sets(full=True)
    sets = {"on": dict(ON), "off": dict(OFF)}
    sets |= {("-", s): dict(ON, **{s: OFF[s]}) for s in SWITCHES} | {("+", s): dict(OFF, **{s: ON[s]}) for s in SWITCHES}
    routes = run(sets, args, planner)
    pairs = [(s, "on", ("-", s)) for s in SWITCHES] + [(s, ("+", s), "off") for s in SWITCHES]
    seen = check_switch_off_turns_nothing_else_on(routes, pairs, len(args))
    assert all(not seen[s] for s in OTHER_SWITCHES)
    for s in OTHER_SWITCHES:  # ... and they turn nothing off either: the planner does not read them
        assert all(routes["on", i] == routes[("-", s), i] for i in range(len(args))), s
    reached = {routes["on", i].path for i in range(len(args))}
    assert reached == {"layers", "msaa", "mask", "covered", "dense"}
    assert any(routes["on", i].defer for i in range(len(args))) and any(routes["on", i].alias for i in range(len(args)))
    assert {routes["on", i].extra for i in range(len(args))} == {None, "flow", "tangent"}
    assert {m for i in range(len(args)) for m in routes["on", i].served} == {"depth", "tangent"}
    assert any(routes["on", i].path == "covered" and not routes["on", i].one_launch for i in range(len(args)))  # (30 x 50: two launches)


def test_every_switch_combination_over_the_small_argument_set(planner):
    args = arg_sets(full=False)
    for factor, values in dict(res=RESOLUTIONS, spp=(1, 2, 4), msaa=(False, True), layers=(1, 2), bg=("none", "plain", "grad"), autocast=(False, True),
                               nrm=(True, False), w2c_grad=(False, True), tng=("present", "pending", "absent"), nets=(True, False)).items():
        assert {a[factor] for a in args} == set(values), factor
    assert [m for m in MODE_LISTS if not any(a["modes"] == m for a in args)] == []
    n = len(PLANNER_SWITCHES)
    sets = {bits: dict(ON, **{s: (ON if bit else OFF)[s] for s, bit in zip(PLANNER_SWITCHES, bits)}) for bits in itertools.product((1, 0), repeat=n)}
    routes = run(sets, args, planner)
    pairs = [(s, bits, bits[:j] + (0,) + bits[j + 1:]) for j, s in enumerate(PLANNER_SWITCHES) for bits in sets if bits[j]]
    seen = check_switch_off_turns_nothing_else_on(routes, pairs, len(args))
    assert all(seen[s] == GOVERNS[s] for s in PLANNER_SWITCHES), {s: GOVERNS[s] - seen[s] for s in PLANNER_SWITCHES}  # (the table claims no more than happens)


def test_with_cpu_tensors_the_planner_refuses_the_gpu_only_fields(monkeypatch):
    """No patch: the same calls with tensors that are where they are.  What only exists as a kernel over device float32 operands -- the
    aliasing clip transform, ops.flow_delta, 'depth' / 'tangent' on the covered-point path, the supersampled path -- is refused."""
    flag = [False]
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: flag[0])
    for s in SWITCHES:
        monkeypatch.setattr(R, s, ON[s])
    assert not R._on_gpu_f32(_MTX) and not R._on_gpu_f32(None) and not R._on_gpu_f32(_MTX.double())
    paths = set()
    for a in arg_sets(full=True):
        route = plan(a, flag)
        paths.add(route.path)
        assert not route.alias and not route.flow_delta and not route.served and route.path != "msaa", (route, a)
        if {"depth", "tangent"} & set(a["modes"]) and a["layers"] == 1:
            assert route.path == "dense", (route, a)
    assert paths == {"layers", "mask", "covered", "dense"}


def test_a_lone_render_layer_call_plans_the_covered_path_from_its_clip_alone(planner):
    """render_layer without a route: ``clip`` decides (not FUSED_GBUFFER, which is render_mesh's reason to hand one over), nothing around
    the call is planned, and 'depth' / 'tangent' keep the dense path."""
    set_switches(dict(ON, FUSED_GBUFFER=False))
    mesh, clip = _MESHES[True, "present"], torch.zeros(B, V, 4)
    r = R._plan_route(["shaded", "flow"], mesh, _W2C[False], (32, 32), 1, clip=clip, flow_cols=2)
    assert r == R._Route("covered", one_launch=True, extra="flow")
    assert R._plan_route(["shaded", "flow"], mesh, _W2C[False], (32, 32), 1, clip=clip, flow_cols=4) == R._Route("covered", one_launch=True)
    assert R._plan_route(["shaded"], mesh, _W2C[False], (30, 50), 1, clip=clip, flow_cols=0) == R._Route("covered")
    for modes, spp, c in ((["shaded"], 1, None), (["shaded"], 2, clip), (["tangent"], 1, clip), (["shaded", "depth"], 1, clip), (["shaded"], 1, clip[:1])):
        assert R._plan_route(modes, mesh, _W2C[False], (32, 32), spp, clip=c, flow_cols=0) == R._Route("dense"), (modes, spp)
    assert R._plan_route(["shaded"], _MESHES[False, "present"], _W2C[False], (32, 32), 1, clip=clip, flow_cols=0) == R._Route("dense")
