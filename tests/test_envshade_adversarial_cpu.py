"""tests/envshade_hard_ref.py pinned and measured, on the CPU: the hand-written float64 reverse mode of EnvironmentLight.shade against
autograd of tests/envshade_cases.reference on every hard case; every case holds what it names; no filler pixel stands near a kink; the
float32 evaluation's error against the float64 one per case and quantity (envshade_hard_ref.MEASURED: the kernel's bound in
tests/test_envshade_adversarial_gpu.py is 4 x these figures, per element); and a check that this bound bites where the per-tensor bound
of tests/test_envshade_gpu.py does not -- five broken reverse modes are rejected, the first two of which the per-tensor bound accepts.

python tests/test_envshade_adversarial_cpu.py prints the table MEASURED is written from (third decimal rounded up).
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import envshade_cases as C  # noqa: E402
import envshade_hard_ref as M  # noqa: E402

F64, F32 = torch.float64, torch.float32
ALL = M.CASES + tuple(n + "_benign" for n in M.NONFINITE)


def _forwards(name):
    """the forward of a case in float64 and in float32 (on the float32 constants)."""
    case = M.build(name)
    out = []
    for dt in (F64, F32):
        M.evaluate(case, dt, magnitudes=False)
        out.append(M.evaluate.last_forward)
    return case, out


# ---------------------------------------------------------------------------------------------- 1. the hand reverse mode is autograd's
@pytest.mark.parametrize("name", ALL)
def test_hand_reverse_mode_equals_autograd(name):
    """On the reference's own (float64) constants: every element within 1e-12 of its magnitude of autograd of C.reference, an element
    nothing feeds equal, and no NaN but in the non-finite cases -- where the hand reverse mode's NaNs are among autograd's (the module
    docstring of envshade_hard_ref says which autograd has more)."""
    case = M.build(name)
    val, mag = M.evaluate(case, consts=M.CONST64)
    ag = M.autograd(case)
    assert sorted(val) == sorted(ag) == sorted(M.quantities(len(case["spec"])))
    for k in val:
        a, b, m = val[k], ag[k], mag[k]
        assert a.shape == b.shape == m.shape, k
        if name in M.NONFINITE:
            assert not bool((torch.isnan(a) & ~torch.isnan(b)).any()), k
        else:
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and bool(torch.isfinite(m).all()), k
        fin = torch.isfinite(a) & torch.isfinite(b)
        assert bool(((a - b).abs()[fin] <= 1e-12 * m[fin]).all()), (k, float(((a - b).abs()[fin] / m[fin].clamp(min=1e-300)).max()))


# ---------------------------------------------------------------------------------------------- 2. every case holds what it names
def _sorted_abs(d):
    return d.abs().sort(-1).values


def _check_light(name, case, f64, f32):
    sizes, dsize = M.LIGHTS[case["light"]]
    assert tuple(m.shape[1] for m in case["spec"]) == sizes and case["dif"].shape[1] == dsize
    want = {"light_d_64_32_16_dif32": ((64, 32, 16), 32), "light_e_4_2_1_dif1": ((4, 2, 1), 1), "light_f_2_1_1_dif2": ((2, 1, 1), 2),
            "light_g_16_to_1_1": ((16, 8, 4, 2, 1, 1), 16), "light_h_16_levels": ((16, 8, 4, 2) + (1,) * 12, 16)}
    if name in want:
        assert (sizes, dsize) == want[name]
    assert case["shape"] == (1, 1, 130)  # three waves, the last partial
    used = set(int(l) for lv in f64.lv for l in lv)
    assert 0 in used and len(sizes) - 1 in used  # the first and the last level are looked up


def _check_wanted(name, case, f64, f32):
    keys = set(M.quantities(3)) - {"values"}
    missing = {"wanted_no_diffuse": {"g_diffuse"}, "wanted_no_level0": {"g_specular[0]"}, "wanted_only_maps": set(M.PIXEL_KEYS),
               "wanted_only_view": keys - {"g_view"}}[name]
    assert set(case["wants"]) == keys - missing
    assert case["shape"] == (1, 9, 8)  # tiled, with a partial tile row


def _check_concentration(name, case, f64, f32):
    which, P = case["which"], f64.P
    first = torch.stack([torch.nonzero(which == k)[0, 0] for k in range(case["n_dirs"])])[which]
    assert P in (512, 1024) and case["n_dirs"] == {"conc_two_quads": 2, "conc_quad_per_wave": 16}.get(name, 1)
    for f in (f64, f32):
        assert bool(f.Ls.valid.all()) and bool(f.Ld.valid.all())
        assert torch.equal(f.qd.rows, f.qd.rows[first])
        for l in (0, 1):
            assert torch.equal(f.qs[l].rows, f.qs[l].rows[first]) and bool((f.lwl[l] > 0).all())
        assert bool((f.lwl[2] == 0).all())
    if name == "conc_two_quads":
        assert int(f64.Ls.face[0]) != int(f64.Ls.face[1]) and int(f64.Ld.face[0]) != int(f64.Ld.face[1])
    if name == "conc_quad_per_wave":
        assert bool((which == torch.arange(P) // 64).all())
    lds = name.endswith("lds")
    assert (max(f64.sizes[:2]) <= 16) == lds and (f64.dsize <= 16) == lds  # both looked-up levels and the diffuse map on one route


def _check_geometry(name, case, f64, f32):
    na, ne, nc, nb = len(M.AXES), len(M.EDGES), len(M.CORNERS), len(M.BESIDE)
    for f in (f64, f32):
        for d in (f.refl, f.n):  # the specular and the diffuse lookup direction (no transform)
            a = _sorted_abs(d)
            assert bool((a[:na, :2] == 0).all()) and bool((a[:na, 2] > 0).all())
            e = a[na:na + ne]
            assert bool((e[:, 0] == 0).all()) and bool((e[:, 1] == e[:, 2]).all()) and bool((e[:, 2] > 0).all())
            c = a[na + ne:na + ne + nc]
            assert bool((c[:, 0] == c[:, 2]).all()) and bool((c[:, 0] > 0).all())
        b = _sorted_abs(f.n[na + ne + nc:na + ne + nc + nb]).double()
        one = torch.ones(nb, dtype=F64)
        assert torch.equal(torch.minimum(b[:, 1], b[:, 2]), torch.tensor([1.0, M.DN, M.DN, 1.0], dtype=F64))
        assert torch.equal(torch.maximum(b[:, 1], b[:, 2]), torch.tensor([M.UP, 1.0, 1.0, M.UP], dtype=F64)) and bool((b[:, 0] < one).all())
    rows = slice(0, na + ne + nc)
    assert torch.equal(f64.Ls.face[rows], f32.Ls.face[rows]) and torch.equal(f64.Ld.face[rows], f32.Ld.face[rows])  # the tie rule decides alike
    assert set(int(x) for x in f64.Ls.face[:na]) == set(range(6))
    small = {"geo_S1": (1, 1), "geo_S2": (2, 2), "geo_S16": (16, 16), "geo_S32": (16, 32)}[name]
    assert (f64.sizes[-1], f64.dsize) == small and bool((f64.lwl[-1][rows] > 0).all()) and bool((f64.lwl[-2][rows] > 0).all())
    if name == "geo_S32":
        assert f64.sizes[-2] == 32
    if name == "geo_S1":  # at S = 1 every tap of a quad but one leaves the face, and one tap is the corner
        assert bool((f64.qd.corner[rows].sum(1) == 1).all())


def _check_kinks(name, case, f64, f32):
    Ln = len(f64.sizes)
    if name == "kink_n_dot_v":
        for f in (f64, f32):
            got = f.dn[:4 * len(M.NDV_KINKS), 0].double().reshape(-1, 4)
            assert torch.equal(got, torch.tensor(M.NDV_KINKS, dtype=F64)[:, None].expand(-1, 4))
        return
    values = case["rough"]
    for f in (f64, f32):
        assert torch.equal(f.ks[:4 * len(values), 1].double().reshape(-1, 4), torch.tensor(values, dtype=F64)[:, None].expand(-1, 4))
    if name == "kink_roughness":  # lo, hi, 1, 0, 1.5: the level is exactly 0, L - 2, L - 1, 0, L - 1 in both precisions
        for f in (f64, f32):
            assert torch.equal(f.mip[:20].double().reshape(-1, 4), torch.tensor([0.0, Ln - 2, Ln - 1, 0, Ln - 1], dtype=F64)[:, None].expand(-1, 4))
            assert f.live[:12].all() and f.in1[:4].all() and f.in2[4:12].all() and not f.in1[12:20].any() and not f.in2[12:20].any()
    else:
        assert values == [M.nextafter32(v, up) for v in (M.CONST32.lo, 0.5, 1.0) for up in (False, True)]


def _check_degenerate(name, case, f64, f32):
    r = lambda i: slice(4 * i, 4 * i + 4)
    for f in (f64, f32):
        assert bool((f.n[r(0)] == 0).all()) and not bool(f.Ld.valid[r(0)].any())
        assert bool((f.d1[r(1)] == 0).all())
        assert bool((f.d1[r(2)] < M.CONST32.eps).all()) and bool((f.d1[r(2)] > 0).all())
        assert bool((f.d1[r(3)] > M.CONST32.eps).all()) and bool((f.d1[r(3)] < 1e-17).all())
        assert torch.allclose(f.n[r(4)].norm(dim=-1).double(), torch.full((4,), 1e-3, dtype=F64), rtol=1e-6)
        assert torch.allclose(f.n[r(5)].norm(dim=-1).double(), torch.full((4,), 1e3, dtype=F64), rtol=1e-6)


def _check_transforms(name, case, f64, f32):
    m = case["mtx"]
    assert torch.equal(m[:, :3, 3], torch.tensor([5.0, -7.0, 11.0], dtype=F64).expand(m.shape[0], 3))
    r, kind = m[:, :3, :3], name[len("xfm_"):]
    if kind == "zero":
        assert bool((r == 0).all()) and not bool(f64.Ld.valid.any()) and not bool(f32.Ls.valid.any())
    elif kind == "reflection":
        assert float(torch.linalg.det(r[0])) < -0.99 and torch.allclose(r[0] @ r[0].T, torch.eye(3, dtype=F64), atol=1e-6)
    elif kind == "shear":
        assert float((r[0] @ r[0].T - torch.eye(3, dtype=F64)).abs().max()) > 0.5
    elif kind.startswith("scale"):
        assert torch.equal(r[0], torch.eye(3, dtype=F64) * M.f32(float(kind[len("scale_"):])))
    else:
        assert m.shape[0] == 3 == case["shape"][0] and not torch.equal(r[0], r[1]) and not torch.equal(r[1], r[2])
        assert float(torch.linalg.det(r[1])) < 0 and abs(float(torch.linalg.det(r[2]))) > 300
    if kind != "zero":
        assert bool(f64.Ld.valid.all()) and bool(f32.Ls.valid.all())


def _check_frames(name, case, f64, f32):
    B, H, W = case["shape"]
    assert (B, H, W) == M.FRAME_SHAPES[name]
    tiled = H >= 8 and W >= 8
    assert tiled == (name in ("frame_1x8x8", "frame_1x8x9", "frame_3x16x8"))
    waves = B * math.ceil(H / 8) * math.ceil(W / 8) if tiled else math.ceil(B * H * W / 64)
    assert waves == {"frame_1x8x8": 1, "frame_1x8x9": 2, "frame_1x7x64": 7, "frame_3x16x8": 6, "frame_list255": 4, "frame_list256": 4}[name]
    assert tuple(case["leaves"][4].shape) == (B, 1, 1, 3)


def _check_magnitudes(name, case, f64, f32):
    if name == "mag_hdr_maps":
        for m in case["spec"] + [case["dif"]]:
            a = m.abs()
            assert bool((a > 1e29).any()) and bool(((a > 0) & (a < 1e-29)).any()) and bool((a == 0).any()) and bool(((a > 1e-3) & (a < 4)).any())
    elif name == "mag_g_out_1e20":
        assert 1e19 < float(case["go"].abs().max()) < 1e22 and float(case["go"].abs().min()) < 1.0
    else:
        pos, view = case["leaves"][0], case["leaves"][4]
        assert float(pos.abs().amax(-1).median()) > 5e3
        assert torch.allclose((view - pos).norm(dim=-1), torch.full(pos.shape[:3], 1e-2, dtype=F64), rtol=0.1)


def _check_operands(name, case, f64, f32):
    shapes = [tuple(t.shape) for t in case["leaves"]]
    if name == "operands_broadcast":
        assert shapes == [(2, 9, 8, 3), (1, 9, 8, 3), (1, 1, 1, 3), (2, 1, 1, 3), (2, 1, 1, 3)] and case["expanded"] == (4,)
    else:
        assert shapes == [(2, 9, 1, 3), (2, 9, 8, 3), (2, 9, 8, 3), (2, 9, 8, 3), (2, 1, 1, 3)]


def _check_nonfinite(name, case, f64, f32):
    which, v = M.NONFINITE[name]
    for i, t in enumerate(case["leaves"] + [case["go"]]):
        bad = ~torch.isfinite(t).all(-1).reshape(-1)
        here = (i == 5 and which is None) or i == which
        assert int(bad.sum()) == (1 if here else 0) and (not here or bool(bad[M.BAD_PIXEL]))
    benign = M.build(name + "_benign")
    for a, b in zip(case["leaves"] + [case["go"]], benign["leaves"] + [benign["go"]]):
        keep = torch.ones(65, dtype=torch.bool)
        keep[M.BAD_PIXEL] = False
        assert torch.equal(a.reshape(65, 3)[keep], b.reshape(65, 3)[keep]) and bool(torch.isfinite(b).all())


def _check_hidden(name, case, f64, f32):
    for f in (f64, f32):
        a = _sorted_abs(f.refl[:8])
        assert bool((a[:, 0] == a[:, 2]).all()) and bool((f.qs[0].corner[:8].sum(1) == 1).all()) and bool((f.qd.corner[:8].sum(1) == 1).all())
        assert float(f.ks[M.HIDDEN_KINK, 1]) == M.CONST32.lo and bool(f.in1[M.HIDDEN_KINK]) and bool(f.live[M.HIDDEN_KINK])
    go = case["go"].reshape(-1, 3).abs().amax(-1)
    assert float(go[list(M.HIDDEN_BIG)].min()) > 2.0 ** 18 * float(go[:M.HIDDEN_BIG[0]].max()) and f64.P == 300
    assert [int(f64.lv[0][p]) for p in M.HIDDEN_BIG] == [0, 1] and bool((f64.lw[1][list(M.HIDDEN_BIG)] > 0.1).all())


_CHECKS = {M._lights: _check_light, M._wanted: _check_wanted, M._concentration: _check_concentration, M._geometry: _check_geometry,
           M._kinks: _check_kinks, M._degenerate: _check_degenerate, M._transforms: _check_transforms, M._frames: _check_frames,
           M._magnitudes: _check_magnitudes, M._operands: _check_operands, M._nonfinite: _check_nonfinite, M._hidden: _check_hidden}


@pytest.mark.parametrize("name", M.CASES)
def test_case_holds_what_it_names(name):
    case, (f64, f32) = _forwards(name)
    assert case["holds"]
    _CHECKS[M._BUILDERS[name]](name, case, f64, f32)
    for t in case["leaves"] + case["spec"] + [case["dif"], case["go"]] + ([] if case["mtx"] is None else [case["mtx"]]):
        fin = torch.isfinite(t)
        assert t.dtype == F64 and torch.equal(t[fin].float().double(), t[fin])  # every value is a float32 number


def test_the_families_of_the_issue_are_all_there():
    assert len(M.CASES) == len(set(M.CASES)) == sum(len(names) for _, names in M.FAMILIES) and len(M.FAMILIES) == 12
    assert max(M.build(n)["shape"][0] * M.build(n)["shape"][1] * M.build(n)["shape"][2] for n in M.CASES) <= 1100


@pytest.mark.parametrize("name", M.CASES)
def test_no_filler_pixel_stands_near_a_kink(name):
    """The share of filler pixels tests/envshade_cases.near_kink finds is 0: nothing is left out of a comparison, so nothing random
    may sit where float32 can legitimately stand on the other side.  (Hand-placed pixels are where they are on purpose.)"""
    case = M.build(name)
    B, H, W = case["shape"]
    leaves = [t.expand(B, H, W, 3) if i < 4 else t for i, t in enumerate(case["leaves"])]
    sizes, dsize = M.LIGHTS[case["light"]]
    near = C.near_kink(sizes, dsize, leaves, True, case["mtx"])
    assert int((near & case["filler"]).sum()) == 0
    assert not bool((case["go"].abs().amax(-1) == 0).any())  # no pixel is taken out through a zero g_out either


# ---------------------------------------------------------------------------------------------- 3. the measured yardstick
def _up3(u):
    return math.ceil(u * 1000 - 1e-9) / 1000


@pytest.mark.parametrize("name", M.CASES)
def test_measured_table_is_current(name):
    """Every figure of envshade_hard_ref.MEASURED against a fresh measurement: not below it (third decimal rounded up), not more than
    the rounding above it -- with a relative slack of 1e-3 for another summation order inside torch."""
    fresh = M.measure(name)
    assert sorted(fresh) == sorted(M.MEASURED[name])
    for k, u in fresh.items():
        t = M.MEASURED[name][k]
        print(f"{name}: {k} {u:.4f} units (table {t})")
        assert math.isfinite(u) and u <= t * (1 + 1e-3) + 1e-9 and t <= u * (1 + 1e-3) + 1.001e-3, (name, k, u, t)


# ---------------------------------------------------------------------------------------------- 4. the bound bites
HIDDEN = "hidden_under_the_largest"


def _mutation_site(mutation):
    _, _, f = M.reference(HIDDEN)
    if mutation == "drop_one_tap":  # pixel 100's first tap with a weight, on the finer of its two levels
        p, l = 100, int(f.lv[0][100])
        t = int(torch.nonzero(f.qs[l].w[p] > 0.05)[0, 0])
        return (p, l, t)
    if mutation == "level_lost_for_a_work_group":
        return (0, 1)
    return (M.HIDDEN_KINK,)


@pytest.mark.parametrize("mutation", M.MUTATIONS)
def test_the_per_element_bound_rejects_a_broken_reverse_mode(mutation):
    """The float64 reverse mode with one piece broken, held to the kernel's bound (4 x MEASURED units + 4 ulp per element): rejected.
    The first two -- one tap of one pixel not scattered, the corner tap's third not handed on -- pass the per-tensor bound of
    tests/test_envshade_gpu.py (C.tolerance) on every tensor: they hide under the error of the tensor's largest element."""
    case = M.build(HIDDEN)
    ref, mag, _ = M.reference(HIDDEN)
    x32, _ = M.evaluate(case, F32, magnitudes=False)
    broken, _ = M.evaluate(case, mutate=mutation, at=_mutation_site(mutation), magnitudes=False)
    bad = {k: len(M.violations(broken[k], ref[k], mag[k], M.figure(HIDDEN, k))) for k in ref}
    old = {k: float((broken[k] - ref[k]).abs().max()) <= C.tolerance(x32[k], ref[k]) for k in ref}
    print(mutation, "elements outside the per-element bound:", {k: v for k, v in bad.items() if v}, "| per-tensor bound passes:", all(old.values()))
    where = {"drop_one_tap": "g_specular", "corner_third_kept": "g_", "level_lost_for_a_work_group": "g_specular[1]",
             "wrong_side_at_a_kink": "g_ks", "g_view_not_negated": "g_view"}[mutation]
    assert sum(v for k, v in bad.items() if k.startswith(where)) > 0
    assert all(v == 0 for k, v in bad.items() if not k.startswith(where))  # (and nothing else moved)
    if mutation in M.MUTATIONS[:2]:
        assert all(old.values()), old
    unbroken, _ = M.evaluate(case, magnitudes=False)
    assert all(len(M.violations(x32[k], ref[k], mag[k], M.figure(HIDDEN, k))) == 0 and torch.equal(unbroken[k], ref[k]) for k in ref)


if __name__ == "__main__":
    print("MEASURED = {")
    for n in M.CASES:
        print(f'    "{n}": {{' + ", ".join(f'"{k}": {_up3(v):.3f}' for k, v in M.measure(n).items()) + "},")
    print("}")
