"""tests/meshgeom_ref.py pinned and measured, on the CPU: the restatement of the DMTet vertex placement and of the vertex normals
against the oracle (bit for bit in float32) and the reference goldens; the float32 evaluation's error against the float64 one on every
case tests/test_meshgeom_adversarial_gpu.py runs (meshgeom_ref.MEASURED: the kernels' bounds are 4 x these figures); the conditions
the cases are built under (same branch at every vertex in both precisions, nothing subnormal, excluded candidates really out of the
float32 range, the vertex counts); and a check that the bounds bite -- float32 emulations of three mistakes violate them, and the
emulation of the statement csrc/dmtet.hip uses now does not.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden, seeded

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshgeom_ref as M  # noqa: E402

from oracle import dmtet_ref  # noqa: E402

F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------- measurement
def measure(name):
    """key -> units of the float32 evaluation of the restatement on one case (every element)."""
    torch.set_num_threads(1)
    if name in M.DM_CASES:
        c = M.dm_build(name)
        ref, got = M.dm_evaluate(c), M.dm_evaluate(c, F32)
        return {k: M.units(got[k], *ref[k]) for k in M.dm_keys(c)}
    c = M.nr_build(name)
    ref, got = M.nr_evaluate(c), M.nr_evaluate(c, F32)
    return {k: M.units(got[k], *ref[k]) for k in M.NR_KEYS}


def measure_all():
    """The table meshgeom_ref.MEASURED is written from: python tests/test_meshgeom_cpu.py (third decimal rounded up)."""
    return {n: {k: float(np.ceil(u * 1000) / 1000) for k, u in measure(n).items()} for n in list(M.DM_CASES) + list(M.NR_CASES)}


@pytest.fixture(scope="module")
def fresh():
    return {n: measure(n) for n in list(M.DM_CASES) + list(M.NR_CASES)}


def test_measured_table_is_current(fresh):
    """Every figure of meshgeom_ref.MEASURED against a fresh measurement: not below it (third decimal rounded up), not more than the
    rounding above it -- with a relative slack of 1e-3 for another summation order inside torch."""
    assert sorted(M.MEASURED) == sorted(fresh)
    for n, row in fresh.items():
        assert sorted(row) == sorted(M.MEASURED[n]), n
        for k, u in row.items():
            print(f"{n}: {k} {u:.4f} units (table {M.MEASURED[n][k]})")
            assert np.isfinite(u), (n, k)
            assert u <= M.MEASURED[n][k] * (1 + 1e-3) + 1e-9 and M.MEASURED[n][k] <= u * (1 + 1e-3) + 1.001e-3, (n, k, u, M.MEASURED[n][k])


# ---------------------------------------------------------------------------------------------------------------- conditions
def test_dmtet_cases_cover_the_vertex_counts_and_stay_in_range():
    """0, 1, 255, 256, 257 and about 1500 surface vertices (and 3 < V < 20: the island and the hole, every edge of one grid vertex);
    no included case has a float64 result outside the float32 normal range or a subnormal float32 intermediate; the excluded
    candidates (the scale family at 2^-126 and 2^126) have such a result."""
    counts = {n: M.dm_build(n)["interp_v"].shape[0] for n in M.DM_CASES}
    print(counts)
    assert {0, 1, 14, 255, 256, 257, 1500} <= set(counts.values())
    assert counts["dm_island_kuhn3"] == counts["dm_hole_kuhn3"] == 14  # an interior vertex of a Kuhn grid has 14 edges
    for n in M.DM_CASES:
        c = M.dm_build(n)
        assert not M.out_of_range(M.dm_evaluate(c)), n
        assert not M.has_subnormal(c), n
    for n in M.EXCLUDED:
        assert M.out_of_range(M.dm_evaluate(M.dm_build(n))), n


def test_dmtet_special_endpoints_are_what_the_names_say():
    c = M.dm_build("dm_zero_endpoints_kuhn3")
    s = c["sdf"][c["interp_v"]]
    zero = s == 0
    neg0 = zero & torch.signbit(s)
    assert int((zero & ~neg0).sum()) > 5 and int(neg0.sum()) > 5 and bool((s[:, 0] > 0).logical_xor(s[:, 1] > 0).all())
    s = M.dm_build("dm_near_tie_kuhn4")["sdf"][M.dm_build("dm_near_tie_kuhn4")["interp_v"]]
    pairs = {(float(a), float(b)) for a, b in s.tolist()}
    t = 2.0 ** -23
    assert {(1.0, -t), (-t, 1.0), (t, -1.0), (-1.0, t)} <= pairs
    s = M.dm_build("dm_ratio_spread_kuhn6")["sdf"][M.dm_build("dm_ratio_spread_kuhn6")["interp_v"]].double()
    r = torch.log2((s[:, 0] / s[:, 1]).abs())
    assert float(r.max()) > 30 and float(r.min()) < -30
    assert M.dm_build("dm_sdf_column_kuhn3")["sdf"].dim() == 2 and M.dm_build("dm_scale_k0_kuhn4")["sdf"].dim() == 1
    e = M.dm_build("dm_empty_kuhn3")
    assert e["interp_v"].shape[0] == 0 and bool((e["sdf"] == 0).any()) and bool(torch.signbit(e["sdf"][e["sdf"] == 0]).any())
    assert float(M.dm_build("dm_g_huge_row_kuhn5")["g_verts"].abs().max()) > 1e17


def test_normals_cases_take_the_same_branch_in_both_precisions():
    """The condition the normals cases are built under: at every vertex the float32 and the float64 evaluation agree on dot <= 1e-20,
    and no vertex's dot is within a factor 1e5 of the switch.  Also: the shapes, the valences the fans promise, what the special cases
    promise (all rows defaulted; the poisoned rows unreferenced)."""
    seen_V, seen_B = set(), set()
    for n in M.NR_CASES:
        c = M.nr_build(n)
        ref, got = M.nr_evaluate(c), M.nr_evaluate(c, F32)
        assert torch.equal(ref["default"], got["default"]), n
        assert M.switch_margin(c) > 1e5, (n, M.switch_margin(c))
        seen_V.add(c["V"])
        seen_B.add(c["B"])
    assert {1, 3, 255, 256, 257, 600} <= seen_V and seen_B == {1, 3}
    fans = M.nr_build("nr_fans_v255")
    assert {1, 2, 7, 8, 9, 16, 17, 40} <= set(torch.bincount(fans["tri"].reshape(-1)).tolist())
    for n in ("nr_cancel_exact_v3", "nr_scaled_1e-6_v255", "nr_v1_no_faces"):
        assert bool(M.nr_evaluate(M.nr_build(n))["default"].all()), n
    for n in ("nr_cancel_exact_v3",):  # exactly zero in both precisions
        c = M.nr_build(n)
        assert bool((M.nr_evaluate(c)["acc"][0] == 0).all()) and bool((M.nr_evaluate(c, F32)["acc"] == 0).all())
    nc = M.nr_build("nr_near_cancel_v257")
    ref = M.nr_evaluate(nc)
    ratio = ref["acc"][0][:, 0].norm(dim=-1) / ref["acc"][1][:, 0].norm(dim=-1)
    assert bool((ratio < 3e-3).all()) and bool((ratio > 1e-4).all()), ratio  # |acc| ~ 1e-3 x sum |terms| at the apex
    p = M.nr_build("nr_nan_unreferenced_v256")
    assert not bool(torch.isin(p["tri"], torch.tensor(p["poisoned"])).any()) and not bool(torch.isfinite(p["v"][:, p["poisoned"]]).all())
    ref = M.nr_evaluate(p)
    keep = torch.ones(p["V"], dtype=torch.bool)
    keep[p["poisoned"]] = False
    assert all(bool(torch.isfinite(ref[k][0]).all()) for k in M.NR_KEYS)
    assert bool((ref["nrm"][0][:, p["poisoned"]] == torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)).all()) and bool((ref["g_v"][0][:, p["poisoned"]] == 0).all())
    dg = M.nr_build("nr_degenerate_faces_v256")
    assert bool(M.nr_evaluate(dg)["default"][:, dg["collinear"]].all()) and bool(torch.isin(torch.tensor(dg["collinear"]), dg["tri"]).all())
    assert any(len(set(f)) < 3 for f in dg["tri"].tolist()) and len({tuple(f) for f in dg["tri"].tolist()}) < dg["tri"].shape[0]
    d = M.nr_build("nr_dmtet_noise_kuhn5")
    assert int(torch.bincount(d["tri"].reshape(-1)).max()) > M_NR_SLOTS


M_NR_SLOTS = 8  # csrc/normals_common.h: NR_SLOTS


# ---------------------------------------------------------------------------------------------------------------- pins
@pytest.mark.parametrize("name", sorted(M.DM_CASES))
def test_placement_in_float32_equals_the_oracle_bit_for_bit(name):
    c = M.dm_build(name)
    want = dmtet_ref.interpolate_verts(c["pos"], c["sdf"], c["interp_v"])
    got = M.place(c["pos"], c["sdf"], c["interp_v"], F32)
    assert got.dtype == F32 and torch.equal(got, want.reshape(-1, 3))


def test_scale_family_is_exact_in_the_restatement():
    """One SDF at seven scales: the float32 restatement's vertices are bit-equal and its gradients scale by 2^-k exactly (every
    operation of the placement and of autograd through it commutes with a power of two while nothing leaves the normal range)."""
    base = M.dm_evaluate(M.dm_build("dm_scale_k0_kuhn4"), F32)
    for k in M.SCALE_POWERS:
        c = M.dm_build(f"dm_scale_k{k}_kuhn4")
        assert torch.equal(c["sdf"], M.dm_build("dm_scale_k0_kuhn4")["sdf"] * float(2.0 ** k))
        got = M.dm_evaluate(c, F32)
        assert torch.equal(got["verts"], base["verts"]) and torch.equal(got["g_pos"], base["g_pos"]), k
        assert torch.equal(got["g_sdf"].double() * 2.0 ** k, base["g_sdf"].double()), k


@pytest.mark.parametrize("name", ["mesh_b1.npz", "mesh_b4.npz", "mesh_isolated.npz"])
def test_normals_restatement_matches_reference_golden(name):
    """Float32 and float64 against the goldens the reference wrote in float32, at the tolerances tests/test_gpu_parity.py holds the
    kernels to on the same files (the goldens' own precision: their sums ran as atomics in another order)."""
    g = golden(name)
    for dtype in (F32, torch.float64):
        c = dict(v=torch.from_numpy(g["v_pos"]), tri=torch.from_numpy(g["faces"]).long())
        c["g_nrm"] = seeded(c["v"].shape, int(g["grad_wgt_seed"]), -1, 1) if "grad_wgt_seed" in g.files else torch.zeros_like(c["v"])
        got = M.nr_evaluate(c, dtype)
        val = (lambda k: got[k][0]) if dtype == torch.float64 else (lambda k: got[k])
        np.testing.assert_allclose(val("nrm").numpy(), g["v_nrm"], atol=2e-6)
        if "grad_v" in g.files:
            np.testing.assert_allclose(val("g_v").numpy(), g["grad_v"], rtol=1e-3, atol=2e-5)
        else:
            assert bool((val("nrm")[0, -1] == torch.tensor([0.0, 0.0, 1.0], dtype=dtype)).all())


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def dm_backward_fp32(c, statement):
    """dm_bwd_kernel's arithmetic in float32, operation by operation, summed per grid vertex in edge order: ``statement`` 'inv2' = the
    product through inv * inv the kernel had, 'split' = (g * inv) * (s * inv), the statement it has now."""
    iv = c["interp_v"]
    s = c["sdf"].reshape(-1)
    sa, sb = s[iv[:, 0]], s[iv[:, 1]]
    pa, pb, g = c["pos"][iv[:, 0]], c["pos"][iv[:, 1]], c["g_verts"]
    inv = 1.0 / (sa - sb)
    dot = lambda p: (g[:, 0] * p[:, 0] + g[:, 1] * p[:, 1]) + g[:, 2] * p[:, 2]
    gwa, gwb = dot(pa), dot(pb)
    if statement == "inv2":
        inv2 = inv * inv
        ca, cb = (gwa - gwb) * sb * inv2, (gwb - gwa) * sa * inv2
    else:
        gd = (gwa - gwb) * inv
        ca, cb = gd * (sb * inv), -gd * (sa * inv)
    g_sdf = torch.zeros_like(s).index_add(0, iv[:, 0], ca).index_add(0, iv[:, 1], cb)
    wa, wb = -sb * inv, sa * inv
    g_pos = torch.zeros_like(c["pos"]).index_add(0, iv[:, 0], g * wa[:, None]).index_add(0, iv[:, 1], g * wb[:, None])
    return dict(g_sdf=g_sdf, g_pos=g_pos)


def _dm_violations(name, got, ref, keys):
    return {k: int(M.bad_elements(got[k], *ref[k], name, k).shape[0]) for k in keys}


@pytest.mark.parametrize("name", sorted(M.DM_CASES))
def test_the_backward_statement_of_the_kernel_is_inside_the_bound(name):
    """The float32 emulation of dm_bwd_kernel as it stands is inside the bound on every case and quantity; so is the float64 answer
    rounded to float32."""
    c = M.dm_build(name)
    ref = M.dm_evaluate(c)
    keys = [k for k in M.dm_keys(c) if k != "verts"]
    assert not any(_dm_violations(name, {k: ref[k][0].float() for k in keys}, ref, keys).values()), name
    bad = _dm_violations(name, dm_backward_fp32(c, "split"), ref, keys)
    assert not any(bad.values()), (name, bad)


def test_bounds_catch_the_inv2_statement():
    """(g_wa - g_wb) * s * (inv * inv), the statement dm_bwd_kernel had: inv * inv overflows for |sdf| below 2.7e-20 (-> inf where the
    gradient is ~1e19) and underflows to zero for |sdf| above ~1e22 (where the gradient is ~1e-31).  It violates the g_sdf bound on
    the scale cases 2^-100, 2^-66 and 2^100 and on none between (at 2^64 inv * inv is subnormal but keeps 21 of its bits)."""
    bad = {}
    for k in (0,) + M.SCALE_POWERS:
        name = f"dm_scale_k{k}_kuhn4"
        c = M.dm_build(name)
        bad[k] = _dm_violations(name, dm_backward_fp32(c, "inv2"), M.dm_evaluate(c), ["g_sdf"])["g_sdf"]
    print("elements of g_sdf outside the bound per scale power:", bad)
    assert all(bad[k] > 0 for k in (-100, -66, 100)), bad
    assert all(bad[k] == 0 for k in (-30, 0, 30, 64)), bad


def _first_keys_only(c, slots):
    """acc (float64) summed over each vertex's ``slots`` smallest keys only (key = corner * F + face)."""
    tri, v = c["tri"], c["v"].double()
    F = tri.shape[0]
    vert = tri.t().reshape(-1)  # entry index = key
    order = torch.argsort(vert, stable=True)
    rank = torch.empty_like(order)
    start = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(vert, minlength=c["V"]), 0)[:-1]])
    rank[order] = torch.arange(3 * F) - start[vert[order]]
    p0, p1, p2 = v[:, tri[:, 0]], v[:, tri[:, 1]], v[:, tri[:, 2]]
    fn = M._cross(p1 - p0, p2 - p0)
    keep = (rank < slots).reshape(3, F)
    acc = torch.zeros_like(v)
    for corner in range(3):
        acc = acc.index_add(1, tri[:, corner], fn * keep[corner][None, :, None])
    return acc


def test_bounds_catch_a_sum_that_stops_after_eight_entries():
    """A vertex's sum over its eight smallest keys only (the register slots, without the tail loop): outside the bound on the fans
    (apex valences 9, 16, 17, 40), on the near-cancelling fan (24) and on the DMTet extraction (up to 12) -- and inside it on a mesh
    whose valence stays below nine."""
    for name, want in (("nr_fans_v255", True), ("nr_near_cancel_v257", True), ("nr_dmtet_noise_kuhn5", True), ("nr_patch_v600", False)):
        c = M.nr_build(name)
        ref = M.nr_evaluate(c)
        broken = _first_keys_only(c, M_NR_SLOTS).float()
        assert (M.bad_elements(broken, *ref["acc"], name, "acc").shape[0] > 0) == want, name
        assert (M.bad_elements(M.normalize(broken.double())[0].float(), *ref["nrm"], name, "nrm").shape[0] > 0) == want, name


def test_bounds_catch_a_gradient_kept_on_defaulted_rows():
    """The backward through x / sqrt(clamp(dot, 1e-20)) without the ``where`` in front (a defaulted row then passes g / 1e-10 on):
    outside the g_v bound where rows that have faces default -- the mesh scaled to 1e-6 (every row) and the collinear faces (on the
    exactly cancelling pair the two windings' adjoints cancel too) -- and the float64 answer itself is inside on every case."""
    for name in M.NR_CASES:
        c = M.nr_build(name)
        ref = M.nr_evaluate(c)
        for k in M.NR_KEYS:
            assert M.bad_elements(ref[k][0].float(), *ref[k], name, k).shape[0] == 0, (name, k)
    for name in ("nr_scaled_1e-6_v255", "nr_degenerate_faces_v256"):
        c = M.nr_build(name)
        ref = M.nr_evaluate(c)
        v = c["v"].double().requires_grad_(True)
        acc = M.accumulate(v, c["tri"])
        nrm = acc / torch.sqrt(torch.clamp((acc * acc).sum(-1, keepdim=True), min=1e-20))
        (gv,) = torch.autograd.grad((nrm * c["g_nrm"].double()).sum(), v)
        assert M.bad_elements(gv.float(), *ref["g_v"], name, "g_v").shape[0] > 0, name


if __name__ == "__main__":
    import pprint

    pprint.pprint(measure_all(), width=150, sort_dicts=False)
