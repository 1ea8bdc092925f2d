"""3danimals_amd/articulation.py without a GPU: the chunk width against the registry, argument refusal through the loaded
library, the limits builders, the torch statements against the float64 restatement of tests/articulation_ref.py (the MEASURED table)
and against what the reference's own functions returned (tests/golden/articulation_*.npz), and that the bounds built from that table
bite."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import articulation_cases as C  # noqa: E402
import articulation_ref as R  # noqa: E402

A = importlib.import_module("3danimals_amd.articulation")
L = importlib.import_module("3danimals_amd._lib")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------- running a case
def run_desc(fn, c, device="cpu"):
    """``fn`` (A.bone_inputs or a torch statement) on case ``c`` -> dict pos, feat, g_feat, g_patch (those that apply), and the leaves."""
    dev = lambda t: None if t is None else t.to(device)
    feat = None if c["feat"] is None else dev(c["feat"]).requires_grad_(True)
    patch = None if c["patch"] is None else C.layout_of(dev(c["patch"]), c["layout"]).requires_grad_(True)
    bf, pos = fn(dev(c["bones"]), dev(c["mvp"]), dev(c["w2c"]), C.Z_OFFSET, C.SPATIAL_SCALE, feat, patch, c["mode"])
    out = {"pos": pos, "_feat_leaf": feat, "_patch_leaf": patch}
    assert not pos.requires_grad and pos.dtype == torch.float32
    if bf is None:
        assert feat is None or patch is None
        return out
    out["feat"] = bf
    leaves = {"g_feat": feat} if "global" in c["mode"] else {}
    if "sample" in c["mode"]:
        leaves["g_patch"] = patch
    grads = torch.autograd.grad(bf, list(leaves.values()), dev(c["g"]))
    out.update(dict(zip(leaves, grads)))
    return out


def desc_units(out, c):
    ref = R.evaluate_desc(c, out["pos"][..., :2])
    assert sorted(ref) == sorted(k for k in out if not k.startswith("_")), (sorted(ref), sorted(out))
    return {k: R.units(out[k], *ref[k]) for k in ref}


def run_limits(fn, c, limits, device="cpu", g_angles=True, g_reg=True):
    x = c["x"].to(device).requires_grad_(True)
    angles, reg = fn(x, limits, return_reg=True)
    terms = ([(angles * c["g_angles"].to(device)).sum()] if g_angles else []) + ([reg * c["g_reg"].to(device)] if g_reg else [])
    loss = sum(terms[1:], terms[0])
    return {"angles": angles, "reg": reg, "g_x": torch.autograd.grad(loss, x)[0]}


def limits_of(kind, cfg):
    return (A.limits_base if kind == "base" else A.limits_fauna)(**cfg)


def limits_units(out, c, **which):
    ref = R.evaluate_limits(c, **which)
    return {k: R.units(out[k], *ref[k]) for k in ref}


def _golden_desc_case(name):
    c = C.golden_bones_inputs(name)
    return dict(c, layout="nchw", g=None)


def measure(name):
    """Units the torch float32 statements reach on one case (CPU, one thread)."""
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        kind, _, row = name.partition("/")
        if kind == "desc":
            c = C.build_desc(row)
            c = C.finite_twin(c) if row in C.NON_FINITE else c
            return desc_units(run_desc(A._bone_inputs_torch, c), c)
        if kind == "limits":
            c = C.build_limits(row)
            return limits_units(run_limits(A._constrain_angles_torch, c, limits_of(c["kind"], c["cfg"])), c)
        if kind == "golden_bones":
            c = _golden_desc_case(row)
            bf, pos = A._bone_inputs_torch(c["bones"], c["mvp"], c["w2c"], C.Z_OFFSET, C.SPATIAL_SCALE, c["feat"], c["patch"], c["mode"])
            ref = R.evaluate_desc(c, pos[..., :2])
            return {"pos": R.units(pos, *ref["pos"]), "feat": R.units(bf, *ref["feat"])}
        assert kind == "golden_limits", name
        gkind, cfg = C.GOLDEN_LIMITS[row]
        c = dict(kind=gkind, cfg=cfg, x=C.golden_limits_x(row).reshape(-1, C.golden_limits_x(row).shape[-2], 3))
        angles = A._constrain_angles_torch(c["x"], limits_of(gkind, cfg))
        ref = R.evaluate_limits(dict(c, g_angles=torch.zeros_like(c["x"]), g_reg=torch.zeros(())))
        return {"angles": R.units(angles, *ref["angles"])}
    finally:
        torch.set_num_threads(prev)


NAMES = ([f"desc/{n}" for n in C.DESC_CASES] + [f"limits/{n}" for n in C.LIMIT_CASES] + [f"golden_bones/{n}" for n in C.GOLDEN_BONES]
         + [f"golden_limits/{n}" for n in C.GOLDEN_LIMITS])


def measure_all():
    """The table articulation_ref.MEASURED is written from (third decimal rounded up):
    python -c 'import sys; sys.path.insert(0, "tests"); import test_articulation_cpu as t; t.print_table()'"""
    return {n: {k: float(np.ceil(u * 1000) / 1000) for k, u in measure(n).items()} for n in NAMES}


def print_table():
    for n, row in measure_all().items():
        print(f'    "{n}": {{' + ", ".join(f'"{k}": {v}' for k, v in row.items()) + "},")


@pytest.fixture(scope="module")
def fresh():
    return {n: measure(n) for n in NAMES}


def test_measured_table_is_current(fresh):
    """Every figure of articulation_ref.MEASURED against a fresh measurement: not below it (third decimal rounded up), not more than the
    rounding above it -- with a relative slack of 1e-3 for another BLAS summation order."""
    assert sorted(R.MEASURED) == sorted(NAMES)
    for n, row in fresh.items():
        assert sorted(row) == sorted(R.MEASURED[n]), n
        for k, u in row.items():
            print(f"{n}: {k} {u:.4f} units (table {R.MEASURED[n][k]})")
            assert np.isfinite(u), (n, k)
            assert u <= R.MEASURED[n][k] * (1 + 1e-3) + 1e-9 and R.MEASURED[n][k] <= u * (1 + 1e-3) + 1.001e-3, (n, k, u, R.MEASURED[n][k])


# ---------------------------------------------------------------------------------------------------------------- golden fixtures
@pytest.mark.parametrize("name", list(C.GOLDEN_LIMITS))
def test_limits_golden(name):
    """The reference's own float32 output: the float64 restatement within the row's bound of it, the torch statement (the
    reference's sequence of operations) within that bound and within 4 ulp of it, and the builder's folded table S, as S * tanh(m x) in float64, within the
    same bound."""
    gold = np.load(os.path.join(GOLDEN, "articulation_limits.npz"))[name]
    kind, cfg = C.GOLDEN_LIMITS[name]
    x = C.golden_limits_x(name)
    assert gold.shape == tuple(x.shape) and gold.dtype == np.float32
    c = dict(kind=kind, cfg=cfg, x=x, g_angles=torch.zeros_like(x), g_reg=torch.zeros(()))
    ref, mag = R.evaluate_limits(c)["angles"]
    fig = R.figure(f"golden_limits/{name}", "angles")
    assert len(R.bad_elements(gold, ref, mag, fig)) == 0
    limits = limits_of(kind, cfg)
    stated = A._constrain_angles_torch(x, limits).numpy()  # the reference's own sequence of operations: the same float32 up to tanh's last bit
    assert len(R.bad_elements(stated, ref, mag, fig)) == 0 and (np.abs(stated - gold) <= 2.0 ** -22 * np.abs(gold)).all()
    assert limits.scale.dtype == torch.float32 and limits.scale64.shape == (x.shape[-2], 3)
    folded = limits.scale64 * np.tanh(limits.multiplier * x.double().numpy())
    assert len(R.bad_elements(gold, folded, mag, fig)) == 0
    assert np.array_equal(limits.scale.numpy(), limits.scale64.astype(np.float32))  # rounded once
    assert np.abs(limits.scale64 - R.factors(kind, cfg, x.shape[-2])).max() <= 1e-15


@pytest.mark.parametrize("name", list(C.GOLDEN_BONES))
def test_bones_golden(name):
    """get_bones / get_bones_from_articulation of the reference on a [3,7,3,5] patch grid: the float64 restatement and the torch statement
    within the row's bound of what they returned."""
    g = np.load(os.path.join(GOLDEN, "articulation_bones.npz"))
    gold_feat, gold_pos = g[name + "_feat"], g[name + "_pos"]
    c = _golden_desc_case(name)
    ref = R.evaluate_desc(c, torch.from_numpy(gold_pos[..., :2]))
    for key, gold in (("pos", gold_pos), ("feat", gold_feat)):
        assert len(R.bad_elements(gold, *ref[key], R.figure(f"golden_bones/{name}", key))) == 0, key
    bf, pos = A.bone_inputs(c["bones"], c["mvp"], c["w2c"], C.Z_OFFSET, C.SPATIAL_SCALE, c["feat"], c["patch"], c["mode"])
    assert tuple(bf.shape) == gold_feat.shape and tuple(pos.shape) == gold_pos.shape
    ref = R.evaluate_desc(c, pos[..., :2])
    assert len(R.bad_elements(pos, *ref["pos"], R.figure(f"golden_bones/{name}", "pos"))) == 0
    assert len(R.bad_elements(bf, *ref["feat"], R.figure(f"golden_bones/{name}", "feat"))) == 0
    assert float(np.abs(bf.numpy() - gold_feat).max()) <= 1e-5 and float(np.abs(pos.numpy() - gold_pos).max()) <= 1e-5  # (a coarse net under the bounds)
    flat5 = A.bone_inputs(c["bones"][:, None] if c["bones"].shape[0] > 1 else c["bones"], c["mvp"], c["w2c"], C.Z_OFFSET, C.SPATIAL_SCALE)
    assert flat5[0] is None and torch.equal(flat5[1], pos)  # feat / patch_feat None: no features; a [B,F,K,2,3] skeleton is flattened


# ---------------------------------------------------------------------------------------------------------------- the bounds bite
def _bad(got, ref_mag, name, key):
    return len(R.bad_elements(got, *ref_mag, R.figure(name, key)))


def test_bounds_catch_a_removed_piece():
    """The float64 answer rounded to float32 is inside every bound; with one piece removed it is not: one tap of one sample, one bone of
    one g_feat sum, one tap of one scattered pixel, the float32 spacing of one position column, one pass of the limits (the 0.05 on a
    top leg bone), one element's share of reg and of its gradient."""
    name = "n3_k5_cbelow_dabove_3x5_nhwc_shared"
    c = C.build_desc(name)
    pos64, _ = R.positions(c["bones"], c["mvp"], c["w2c"], C.Z_OFFSET, C.SPATIAL_SCALE)
    xy = torch.from_numpy(pos64[..., :2]).float()
    ref = R.evaluate_desc(c, xy)
    rounded = {k: torch.from_numpy(v[0]).float() for k, v in ref.items()}
    for k in ref:
        assert _bad(rounded[k], ref[k], f"desc/{name}", k) == 0, k
    D, P = c["D"], c["patch"].double().numpy()
    n, k = next((n, k) for n in range(c["N"]) for k in range(c["K"]) if len(R.taps(float(xy[n, k, 0]), float(xy[n, k, 1]), c["h"], c["w"])) == 4)
    r, col, wt = max(R.taps(float(xy[n, k, 0]), float(xy[n, k, 1]), c["h"], c["w"]), key=lambda t: t[2])
    broken = ref["feat"][0].copy()
    broken[n, k, D:] -= wt * P[n, :, r, col]
    assert _bad(broken, ref["feat"], f"desc/{name}", "feat") > 0
    broken = ref["g_feat"][0].copy()
    broken[n] -= c["g"][n, k, :D].double().numpy()
    assert _bad(broken, ref["g_feat"], f"desc/{name}", "g_feat") > 0
    broken = ref["g_patch"][0].copy()
    broken[n, :, r, col] -= wt * c["g"][n, k, D:].double().numpy()
    assert _bad(broken, ref["g_patch"], f"desc/{name}", "g_patch") > 0
    broken = ref["pos"][0].copy()
    broken[n, k, 4] *= 1 + 2.0 ** -17
    assert _bad(broken, ref["pos"], f"desc/{name}", "pos") > 0

    lname = "k20_n3_fauna_constraints"
    lc = C.build_limits(lname)
    lref = R.evaluate_limits(lc)
    for k in lref:
        assert _bad(torch.from_numpy(np.asarray(lref[k][0])).float(), lref[k], f"limits/{lname}", k) == 0, k
    without = dict(lc, cfg=dict(lc["cfg"], use_fauna_constraints=False))
    assert _bad(R.evaluate_limits(without)["angles"][0], lref["angles"], f"limits/{lname}", "angles") > 0
    angles = lref["angles"][0]
    i = np.unravel_index(np.abs(angles).argmax(), angles.shape)
    assert _bad(lref["reg"][0] - angles[i] ** 2 / angles.size, lref["reg"], f"limits/{lname}", "reg") > 0
    only_angles = R.evaluate_limits(lc, g_reg=False)["g_x"][0]  # (the gradient without reg's share)
    assert _bad(only_angles, lref["g_x"], f"limits/{lname}", "g_x") > 0


# ---------------------------------------------------------------------------------------------------------------- the registry
def test_the_chunk_width_everywhere_is_the_registered_constant():
    """(csrc/articulation.h itself is held to its entry of _lib.INTERNAL_SURFACES by tests/test_abi_cpu.py, like every header.)"""
    assert A.CHUNK == L.ARTICULATION_CHUNK and C.CHUNK == A.CHUNK


def test_arguments_are_refused_before_anything_is_launched():
    """Through the loaded library, without a device: K of 0 and 65, a null operand, h = 0, too many angles; an empty list is no work."""
    lib = L.lib()
    fwd = lambda N, K, D, C, h, w: lib.a3d_bone_inputs_fwd(None, 0, None, None, 0.0, 1.0, None, None, 0, 0, 0, 0, N, K, D, C, h, w, None, None, None)
    bwd = lambda N, K, D, C, h, w: lib.a3d_bone_inputs_bwd(None, None, N, K, D, C, h, w, None, None, 1, 1, 1, 1, None)
    for f in (fwd, bwd):
        assert f(1, 0, 4, 4, 3, 5) != 0 and f(1, 65, 4, 4, 3, 5) != 0
        assert f(0, 0, 4, 4, 3, 5) != 0  # (K is checked before an empty list is let through)
        assert f(1, 5, 4, 4, 0, 5) != 0 and f(1, 5, 4, 4, 3, 4097) != 0
        assert f(1, 5, 4, 4, 3, 5) != 0  # a null operand
        assert b"invalid argument" in lib.a3d_last_error()
        assert f(0, 5, 4, 4, 3, 5) == 0  # an empty list is no work
        assert f(65536, 5, 4, 4, 3, 5) != 0 and f(1 << 20, 64, 384, 384, 3, 5) != 0
    ca_f = lambda N, K: lib.a3d_constrain_angles_fwd(None, None, 1.0, N, K, None, None, None)
    ca_b = lambda N, K: lib.a3d_constrain_angles_bwd(None, None, None, None, 1.0, N, K, None, None)
    for f in (ca_f, ca_b):
        assert f(1, 0) != 0 and f(1, 65) != 0 and f(1, 20) != 0
        assert f(0, 20) == 0
        assert f((1 << 20) // 60 + 1, 20) != 0  # N * K * 3 above 2^20


# ---------------------------------------------------------------------------------------------------------------- the builders
def test_builders_refuse_skeletons_the_hard_coded_lists_do_not_fit():
    pony = dict(num_body_bones=8, num_legs=4, num_leg_bones=3, output_multiplier=0.1, max_arti_angle=60)
    short = dict(pony, num_legs=2)  # K = 14
    assert A.limits_base(**short, constrain_legs=True).num_bones == 14  # the plain leg passes take their bones from the counts
    with pytest.raises(ValueError, match="index past"):
        A.limits_base(**short, constrain_legs=True, use_fauna_constraints=True)  # [10, 13, 16, 19]
    with pytest.raises(ValueError, match="index past"):
        A.limits_base(**short, extra_constraints=True)  # [8, 11, 14, 17]
    with pytest.raises(ValueError, match="index past"):
        A.limits_base(**dict(pony, num_body_bones=4, num_legs=0), constrain_legs=True, use_fauna_constraints=True)  # [0..7]
    fauna = dict(static_root_bones=False, total_iter=10, iter_leg_rotation_start=5, forbid_leg_rotate=True, small_leg_angle=True, reg_body_rotate_mult=0.1)
    with pytest.raises(ValueError, match="index past"):
        A.limits_fauna(**short, **fauna)
    with pytest.raises(ValueError, match="index past"):
        A.limits_fauna(**dict(pony, num_body_bones=4, num_legs=0), **dict(fauna, total_iter=1))  # the body list [0..7] is unconditional
    assert A.limits_fauna(**short, **dict(fauna, total_iter=1)).num_bones == 14  # before the switch only the counted leg bones
    with pytest.raises(ValueError):
        A.limits_base(0, 0, 0, 0.1, 60)
    with pytest.raises(ValueError):
        A.ArticulationLimits(1.0, [[1.0, 2.0]])
    with pytest.raises(ValueError):
        A.ArticulationLimits(float("nan"), np.ones((3, 3)))
    plain = A.ArticulationLimits(0.5, np.full((3, 3), 2.0))
    x = torch.linspace(-3, 3, 18).reshape(2, 3, 3)
    assert torch.equal(A.constrain_angles(x, plain), (x * 0.5).tanh() * 2.0)
    # the bird's static roots [3, 7] before the tanh are a factor of 0 behind it
    bird = A.limits_base(8, 0, 0, 0.1, 45, static_root_bones=True)
    assert (bird.scale[[3, 7]] == 0).all() and (bird.scale[[0, 1, 2, 4, 5, 6]] == np.float32(45 / 180 * np.pi)).all()


def test_malformed_arguments_raise_value_error():
    c = C.build_desc("n3_k5_cbelow_dabove_3x5_nhwc_shared")
    args = (c["bones"], c["mvp"], c["w2c"], C.Z_OFFSET, C.SPATIAL_SCALE)
    for bad in ((c["bones"][0],) + args[1:], (c["bones"], c["mvp"][:2]) + args[2:], (c["bones"].long(),) + args[1:],
                args[:4] + (0.0,), args[:3] + (float("inf"), 7.0)):
        with pytest.raises(ValueError):
            A.bone_inputs(*bad)
    with pytest.raises(ValueError):
        A.bone_inputs(*args, c["feat"], c["patch"], feature_mode="dino")
    with pytest.raises(ValueError):
        A.bone_inputs(*args, c["feat"][:2], c["patch"])
    with pytest.raises(ValueError):
        A.bone_inputs(*args, c["feat"], c["patch"][:, :, 0])
    limits = A.limits_base(8, 4, 3, 0.1, 60)
    for bad in (torch.zeros(3, 19, 3), torch.zeros(20, 3), torch.zeros(3, 20, 3, dtype=torch.int32), [0.0]):
        with pytest.raises(ValueError):
            A.constrain_angles(bad, limits)
    with pytest.raises(ValueError):
        A.constrain_angles(torch.zeros(3, 20, 3), limits.scale)


# ---------------------------------------------------------------------------------------------------------------- dispatch
def test_cpu_tensors_take_the_torch_statement_and_nothing_is_written_into_an_argument(monkeypatch):
    ops = importlib.import_module("3danimals_amd.ops")

    def never(*a, **k):
        raise AssertionError("a CPU tensor reached the device route")

    monkeypatch.setattr(ops, "bone_inputs", never)
    monkeypatch.setattr(ops, "constrain_angles", never)
    assert A.DEVICE is True
    c = C.build_desc("n3_k64_cabove_dat_3x5_slice")
    patch = C.layout_of(c["patch"], c["layout"])
    assert not patch.is_contiguous()
    ins = [c["bones"], c["mvp"], c["w2c"], c["feat"], patch]
    before = [t.clone() for t in ins]
    bf, pos = A.bone_inputs(c["bones"], c["mvp"], c["w2c"], C.Z_OFFSET, C.SPATIAL_SCALE, c["feat"], patch, c["mode"])
    tf, tpos = A._bone_inputs_torch(c["bones"], c["mvp"], c["w2c"], C.Z_OFFSET, C.SPATIAL_SCALE, c["feat"], patch, c["mode"])
    assert torch.equal(bf, tf) and torch.equal(pos, tpos)
    assert bf.shape == (3, 64, c["D"] + c["C"]) and torch.equal(bf[:, :, :c["D"]], c["feat"][:, None].expand(-1, 64, -1))  # global columns first
    assert all(torch.equal(a, b) for a, b in zip(ins, before))
    for mode, width in (("global", c["D"]), ("sample", c["C"])):
        assert A.bone_inputs(c["bones"], c["mvp"], c["w2c"], C.Z_OFFSET, C.SPATIAL_SCALE, c["feat"], patch, mode)[0].shape[-1] == width
    assert A.bone_inputs(c["bones"], c["mvp"], c["w2c"], C.Z_OFFSET, C.SPATIAL_SCALE, c["feat"], None)[0] is None

    lc = C.build_limits("k20_n3_magicpony")
    limits = limits_of(lc["kind"], lc["cfg"])
    x = lc["x"].clone()
    angles, reg = A.constrain_angles(x, limits, return_reg=True)
    assert torch.equal(x, lc["x"])  # (the reference's in-place *= is a plain multiply here)
    ta, treg = A._constrain_angles_torch(x, limits, True)
    assert torch.equal(angles, ta) and torch.equal(reg, treg) and reg.dim() == 0 and reg.dtype == torch.float32
    four = A.constrain_angles(x.reshape(3, 1, 20, 3), limits)
    assert four.shape == (3, 1, 20, 3) and torch.equal(four.reshape(3, 20, 3), angles)
    xg = x.clone().requires_grad_(True)
    a2, r2 = A.constrain_angles(xg, limits, return_reg=True)
    (a2.sum() + r2).backward()
    assert xg.grad is not None and torch.equal(xg.detach(), lc["x"])
