"""tests/aa_ref.py and tests/aa_cases.py pinned and measured, on the CPU:

  * the restatement IS the specification: evaluate(decide(...)) in float64 equals oracle.raster_ref.antialias on every case, to 1e-12 in
    value and 1e-10 in gradient (relative to the largest element);
  * the conditions the cases are built under: on the lattice cases float32 and float64 decide the identical record set and alpha
    differs by at most 1 ulp; off the lattice at most 1 % of the candidate pairs are marginal and only marginal pairs are decided
    differently; the cases hold what their names say (the pool fills, the four blends, the four roles, the clamp window, 45 degrees,
    the opposite-vertex rule);
  * aa_ref.MEASURED: what the float32 evaluation of the restatement reaches against the float64 one, per run and quantity, measured
    afresh and compared (the kernels' bound in tests/test_aa_adversarial_gpu.py is 4 x these figures + 4 ulp of the float64 value);
  * the bounds bite: six deliberate mistakes in the float32 evaluation each put at least one element outside that bound, and the
    unmutated float32 evaluation and the rounded float64 answer put none;
  * the index identity behind ca_compose_kernel / ca_gather_kernel, int((j + 0.5f) * (1.0f / C)) == j // C, for every C in 1..4096 and
    every j < 256 C, in numpy float32 with the kernel's operation order.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aa_cases as K  # noqa: E402
import aa_ref as A  # noqa: E402

from oracle import raster_ref  # noqa: E402

F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------------------------- the specification
def _close(got, want, tol, what):
    scale = max(1.0, float(want.abs().max()) if want.numel() else 0.0)
    err = float((got - want).abs().max()) if want.numel() else 0.0
    assert got.shape == want.shape and err <= tol * scale, (what, err, scale)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_restatement_equals_the_oracle_in_float64(name):
    """decide + evaluate against oracle.raster_ref.antialias, float64: the dense form on the case's colour image and the rows form on the
    image composited with torch -- images to 1e-12, the gradients in colour / rows and in clip to 1e-10."""
    c = K.build(name)
    d = K.decided(name, F64)
    clip0 = c["clip"]
    for run in (f"{name}:dense", f"{name}:rows"):
        if run not in K.RUNS:
            continue
        (buf,) = K.buffers(run)
        got = A.evaluate(c, d["rec"], d["alpha"], [buf])
        clip = clip0.double().requires_grad_(True)
        if buf.form == "dense":
            leaf = buf.kw["color"].double().requires_grad_(True)
            pre, key = leaf, "g_color0"
        else:
            leaf = buf.kw["vals"].double().requires_grad_(True)
            pix = A.covered_list(c["rast"])
            pre = buf.kw["bg"].double().expand(c["B"], -1, -1, -1).reshape(-1, leaf.shape[1] + 1)
            pre = pre.index_copy(0, pix, torch.cat([leaf[:pix.shape[0]], torch.ones(pix.shape[0], 1, dtype=F64)], 1)).view(c["B"], c["H"], c["W"], -1)
            key = "g_vals0"
        want = raster_ref.antialias(pre, c["rast"], clip, c["tri"])
        gl, gc = torch.autograd.grad((want * buf.g.double()).sum(), [leaf, clip], allow_unused=True)
        gl, gc = (torch.zeros_like(leaf) if gl is None else gl), (torch.zeros_like(clip) if gc is None else gc)
        _close(got["out0"][0], want.detach(), 1e-12, (run, "out"))
        _close(got[key][0], gl, 1e-10, (run, key))
        _close(got["g_clip"][0], gc, 1e-10, (run, "g_clip"))
        for k, (v, m) in got.items():
            assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(m).all()) and bool((m >= 0).all()), (run, k)
            assert bool((m * (1 + 1e-12) >= v.abs()).all()), (run, k)  # a magnitude is never below the value it belongs to


def test_records_are_the_oracles_blends():
    """The record list read back as blends gives the oracle's image bit for bit in float32 on a lattice case with integer colours (every
    blend exact): (pix0, flags bit 0, alpha) mean what ``struct AaRec`` says."""
    c = K.build("checker_16x16")
    d = K.decided("checker_16x16")
    color = torch.randint(0, 8, (1, 16, 16, 3), generator=torch.Generator().manual_seed(1)).float()
    out = A.blend(color, d["rec"], d["alpha"], A.destinations(d["rec"], d["alpha"], 16), 16)
    assert torch.equal(out, raster_ref.antialias(color, c["rast"], c["clip"], c["tri"]))


# ---------------------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("name", sorted(n for n in K.CASES if K.build(n)["lattice"]))
def test_lattice_cases_decide_identically_in_both_precisions(name):
    d32, d64 = K.decided(name), K.decided(name, F64)
    assert torch.equal(d32["rec"], d64["rec"]), name
    a32 = d32["alpha"].double()
    ulp = torch.from_numpy(np.spacing(np.abs(d32["alpha"].numpy()))).double()
    assert bool(((a32 - d64["alpha"]).abs() <= ulp).all()), name


@pytest.mark.parametrize("name", sorted(n for n in K.CASES if not K.build(n)["lattice"]))
def test_off_lattice_cases_have_few_marginal_pairs(name):
    """At most 1 % of the candidate pairs are marginal (a decision margin below 1e-4 in its own scale that can change the pair's outcome),
    and float32 and float64 differ on marginal pairs only.  A condition on the inputs: the seeds are chosen so that it holds."""
    d32, d64 = K.decided(name), K.decided(name, F64)
    n, m = d32["cand"].shape[0], int(d32["marginal"].sum())
    print(f"{name}: {n} candidate pairs, {d32['rec'].shape[0]} records, {m} marginal")
    assert m <= 0.01 * n, (name, m, n)
    marginal = set((d32["cand"][:, 0] * 2 + d32["cand"][:, 1])[d32["marginal"]].tolist())
    rows32 = {tuple(r) for r in d32["rec"].tolist()}
    rows64 = {tuple(r) for r in d64["rec"].tolist()}
    assert all(r[0] * 2 + (r[2] & 1) in marginal for r in rows32 ^ rows64), name


def _per_group(cand, H, W):
    """Candidate pairs per analysis work-group (256 consecutive pixels of an image, both directions of each)."""
    return torch.bincount(cand[:, 0] // 256) if (H * W) % 256 == 0 else None


def test_cases_hold_what_their_names_say():
    d = K.decided("checker_16x16")
    assert d["cand"].shape[0] == 480  # one work-group: two trips of the pool loop, the second with 224 of its 256 lanes
    assert K.decided("partial_16x16")["cand"].shape[0] == 302  # 256 + 46: the second trip is wave 0's alone
    d = K.decided("checker_3x512")
    groups = _per_group(d["cand"], 3, 512).tolist()
    assert groups == [512, 511, 512, 511, 256, 255], groups  # the pool exactly full; row 2 right pairs only
    e = K.build("every_3x512")
    assert bool((e["rast"][..., 3] > 0).all()) and set(e["rast"][..., 2].unique().tolist()) == {0.0, 0.125, 0.25, 0.375}
    z = e["rast"][0, :, :, 2]
    assert int((z[:, 1:] == z[:, :-1]).sum()) > 100 and int((z[1:] == z[:-1]).sum()) > 100  # exact depth ties in both directions
    assert _per_group(K.decided("every_3x512")["cand"], 3, 512).tolist() == [512, 511, 512, 511, 256, 255]
    sizes = {n: (K.build(n)["H"], K.build(n)["W"]) for n in K.CASES}
    assert {(1, 1), (1, 257), (300, 1), (5, 7), (17, 15), (16, 16)} <= set(sizes.values())
    assert all(h * w < 2000 for h, w in sizes.values())
    for n in ("batch3_shared_17x15", "batch3_own_17x15"):
        c = K.build(n)
        assert c["clip"].shape[0] == (1 if "shared" in n else 3) and not bool((c["rast"][1, ..., 3] > 0).any())
        assert bool((c["rast"][2, ..., 3] == 1).all())
        assert set((K.decided(n)["cand"][:, 0] // (17 * 15)).tolist()) == {0}  # images 1 and 2 have no candidate pair
    # four blends land on one uncovered pixel; one covered pixel plays all four roles
    for n, covered in (("four_blends_8x8", False), ("four_roles_8x8", True), ("four_roles_12x12", True)):
        c, d = K.build(n), K.decided(n)
        W, p = c["W"], c["centre"]
        assert bool(c["rast"].reshape(-1, 4)[p, 3] > 0) == covered
        dst = A.destinations(d["rec"], d["alpha"], W)
        assert int((dst == p).sum()) == 4, n
        roles = {(int(r[0]) == p, int(r[2]) & 1) for r in d["rec"].tolist() if int(r[0]) == p or int(r[0]) + (W if r[2] & 1 else 1) == p}
        assert roles == {(True, 0), (True, 1), (False, 0), (False, 1)}, n
    # w < 0 and w != 1
    c = K.build("perspective_16x16")
    assert int((c["clip"][..., 3] < 0).sum()) == 1 and set(c["clip"][..., 3].abs().unique().tolist()) == {0.25, 0.5, 2.0, 4.0}
    r = K.build("rasterised_24x40")
    assert r["B"] == 2 and K.decided("rasterised_24x40")["rec"].shape[0] > 100


@pytest.mark.parametrize("name", ["clamp_window_32x32", "slope_45_32x32", "topology_16x32"])
def test_expected_records_of_the_hand_made_sites(name):
    """Per site: no record (None) or a record whose clamp flag is the expected one; a clamped record has alpha +-1/2 exactly."""
    c, d = K.build(name), K.decided(name)
    by_pair = {(int(r[0]), int(r[2]) & 1): (int(r[2]), float(a)) for r, a in zip(d["rec"].tolist(), d["alpha"].tolist())}
    assert c["expect"]
    for pair, want in c["expect"].items():
        if want == "any":
            continue
        if want is None:
            assert pair not in by_pair, (name, pair)
        else:
            assert pair in by_pair and bool(by_pair[pair][0] & 16) == want, (name, pair, by_pair.get(pair))
            if want:
                assert abs(by_pair[pair][1]) == 0.5
    if name == "clamp_window_32x32":
        assert sum(1 for f, _ in by_pair.values() if f & 16) == 8 and sum(1 for v in c["expect"].values() if v is None) == 8
    if name == "slope_45_32x32":
        assert sum(1 for v in c["expect"].values() if v is None) == 8 and sum(1 for v in c["expect"].values() if v is False) == 16
    if name == "topology_16x32":
        online = [p for p, v in c["expect"].items() if v == "any"][:2]  # the opposite vertex on the edge line, the two windings:
        assert sum(p in by_pair for p in online) == 1  # w is +0, bb changes sign with the winding: exactly one is a silhouette
        opp = raster_ref.edge_opposites(c["tri"].numpy())
        assert int((opp >= 0).sum()) >= 8 and int((opp < 0).sum()) >= 3


def test_depth_runs_have_distinct_extremes():
    """No tie at the minimum or the maximum of any image of a depth run (tests/depth_ref.py: extreme_gaps >= 1e-4), so float32 and
    float64 agree on which points take the range's gradient."""
    import depth_ref

    for run in K.RUNS:
        buf = K.buffers(run)[0]
        if buf.form != "depth":
            continue
        c = K.build(K.run_case(run))
        gaps = depth_ref.extreme_gaps(buf.kw["gb"], A.covered_list(c["rast"]), c["rast"][..., 3] > 0, buf.kw["w2c"].expand(c["B"], -1, -1))
        assert gaps and min(min(g) for g in gaps) >= 1e-4, (run, gaps)


# ---------------------------------------------------------------------------------------------------------------- measurement
NULL_ORDERS = 8


def measure(run):
    """quantity -> units of the float32 evaluation of the restatement on one run (every element).  g_null and g_vals of a supersampled
    buffer: the largest of that figure and of the flat float32 sum of the restatement's own per-block and per-record terms in
    NULL_ORDERS seeded orders (aa_ref.evaluate, flat_null: the sums the kernels form)."""
    ref, got = K.reference(run)
    out = {k: A.units(got[k], *ref[k]) for k in K.keys(run)}
    flat_keys = _flat_keys(run)
    if flat_keys:
        c, d = K.build(K.run_case(run)), K.decided(K.run_case(run))
        for seed in range(NULL_ORDERS):
            flat = A.evaluate(c, d["rec"], d["alpha"], K.buffers(run), dtype=F32, flat_null=seed)
            for k in flat_keys:
                out[k] = max(out[k], A.units(flat[k], *ref[k]))
    return out


def _flat_keys(run):
    """g_vals and g_null of the supersampled buffers of a run."""
    return [f"g_{n}{i}" for i, b in enumerate(K.buffers(run)) if b.form == "msaa" for n in ("vals", "null")]


def test_flat_null_sum_is_the_same_sum():
    """The flat sums of g_vals' and g_null's terms (aa_ref.evaluate, flat_null) in float64 equal autograd's to 1e-12: the same terms, only
    grouped differently."""
    for run in K.RUNS:
        if not _flat_keys(run):
            continue
        c, d = K.build(K.run_case(run)), K.decided(K.run_case(run))
        ref = K.reference(run)[0]
        flat = A.evaluate(c, d["rec"], d["alpha"], K.buffers(run), dtype=F64, flat_null=0)
        for k in _flat_keys(run):
            _close(flat[k][0], ref[k][0], 1e-12, (run, k))


def measure_all():
    """The table aa_ref.MEASURED is written from: python tests/test_aa_cpu.py (third decimal rounded up)."""
    return {r: {k: float(np.ceil(u * 1000) / 1000) for k, u in measure(r).items()} for r in K.RUNS}


def test_measured_table_is_current():
    """Every figure of aa_ref.MEASURED against a fresh measurement: not below it (third decimal rounded up), not more than the rounding
    above it -- with a relative slack of 1e-3 for another summation order inside torch."""
    assert sorted(A.MEASURED) == sorted(K.RUNS)
    for r in K.RUNS:
        row = measure(r)
        assert sorted(row) == sorted(A.MEASURED[r]), r
        for k, u in row.items():
            print(f"{r}: {k} {u:.4f} units (table {A.MEASURED[r][k]})")
            assert np.isfinite(u), (r, k)
            assert u <= A.MEASURED[r][k] * (1 + 1e-3) + 1e-9 and A.MEASURED[r][k] <= u * (1 + 1e-3) + 1.001e-3, (r, k, u, A.MEASURED[r][k])


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _violations(run, got):
    ref = K.reference(run)[0]
    return {k: int(A.bad_elements(got[k], *ref[k], run, k).shape[0]) for k in K.keys(run)}


@pytest.mark.parametrize("run", sorted(K.RUNS))
def test_float32_restatement_and_rounded_answer_are_inside_the_bound(run):
    ref, got = K.reference(run)
    assert not any(_violations(run, got).values()), (run, _violations(run, got))
    assert not any(_violations(run, {k: ref[k][0].float() for k in K.keys(run)}).values()), run


def _mutated(run, kind, which):
    c, d = K.build(K.run_case(run)), K.decided(K.run_case(run))
    return _violations(run, A.evaluate(c, d["rec"], d["alpha"], K.buffers(run), dtype=F32, mutate=(kind, which)))


def test_bounds_catch_six_mistakes():
    """One record dropped, one alpha with its sign flipped, the destination pixel swapped, a clamped record given a position gradient, the
    w-gradient term omitted, one role of g_slots overwritten: the float32 evaluation with each mistake is outside the GPU tests' bound
    in the quantities the mistake touches."""
    run = "checker_16x16:rows"
    for kind in ("drop", "flip", "swap"):
        bad = _mutated(run, kind, 7)
        print(kind, bad)
        assert bad["out0"] > 0 and bad["g_vals0"] > 0 and bad["g_clip"] > 0, (kind, bad)
    d = K.decided("clamp_window_32x32")
    clamped = torch.nonzero((d["rec"][:, 2] & 16) != 0)[:, 0].tolist()
    assert len(clamped) == 8
    for which in clamped:
        bad = _mutated("clamp_window_32x32:dense", "unclamp", which)
        assert bad["g_clip"] > 0 and bad["out0"] == 0 and bad["g_color0"] == 0, (which, bad)
    bad = _mutated("perspective_16x16:dense", "no_w", None)
    print("no_w", bad)
    assert bad["g_clip"] > 0 and bad["out0"] == 0 and bad["g_color0"] == 0, bad
    c, d = K.build("four_roles_8x8"), K.decided("four_roles_8x8")
    first = [i for i, r in enumerate(d["rec"].tolist()) if r[0] == c["centre"]]
    assert len(first) == 2  # the centre is the first pixel of a right and of a lower record
    for which in first:
        bad = _mutated("four_roles_8x8:rows_C1", "slot", which)
        assert bad["g_vals0"] > 0, (which, bad)


# ---------------------------------------------------------------------------------------------------------------- index identity
def test_float_division_index_identity():
    """pl = (int)((j + 0.5f) * rc), rc = 1.0f / C (ca_compose_kernel: C = the stored channels of a pixel, up to 4096; ca_gather_kernel:
    C = the channels of a value row) equals j // C for every C in 1..4096 and every j < 256 C -- every element a work-group moves."""
    half = np.float32(0.5)
    pixel = np.arange(256, dtype=np.int32)
    for C in range(1, 4097):
        rc = np.float32(1.0) / np.float32(C)
        j = np.arange(256 * C, dtype=np.int32)
        pl = ((j.astype(np.float32) + half) * rc).astype(np.int32)
        assert pl.dtype == np.int32 and np.array_equal(pl.reshape(256, C), np.broadcast_to(pixel[:, None], (256, C))), C


if __name__ == "__main__":
    import pprint

    pprint.pprint(measure_all(), width=170, sort_dicts=False)
