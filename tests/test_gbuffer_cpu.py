"""tests/gbuffer_ref.py checked on the CPU: every list pattern forces the stage of gb_bwd_kernel it names (replayed by ``simulate``),
the exact mode is exact in fp32 whatever the summation order, the Err chain of columns 0..2 reproduces autograd, and the bounds catch
one dropped (entry, corner) contribution."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gbuffer_ref as G  # noqa: E402

B, H, W = 2, 24, 40


def _case(name, table, P=None, B_=B, seed=0):
    return G.finish(G.make_list(name, table, B_, seed, P), B_, H, W, seed)


def test_hash_is_the_kernels():
    """(key * 2654435761 mod 2^32) >> 23 resp. >> 22, by hand for two keys."""
    assert int(G.gb_hash(1, 512)) == 2654435761 >> 23 == 316 and int(G.gb_hash(1, 1024)) == 2654435761 >> 22 == 632
    assert int(G.gb_hash(3, 512)) == ((3 * 2654435761) % 2 ** 32) >> 23


@pytest.mark.parametrize("table", ["small", "big"])
@pytest.mark.parametrize("name", [p for p in G.PATTERNS if p != "holes"])
def test_pattern_forces_its_stage(name, table):
    """The merge distance, the entry overflow, the slot overflow, the single hash value, the long list and the unmerged boundary, each
    asserted on the CPU replay of the work-groups (gbuffer_ref.assert_forced), under the table size the case is built for."""
    G.assert_forced(_case(name, table))


@pytest.mark.parametrize("table", ["small", "big"])
@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_holes_lists(P, table):
    case = _case("holes", table, P, B_=1 if (P == 1 and table == "small") else B)
    assert case["P"] == P and (P < 0.6 * case["B"] * case["F"]) == (table == "big")
    if P > 1:
        f = case["f"]
        assert (f < 0).any() and (f >= case["F"]).any() and ((f >= 0) & (f < case["F"])).sum() > P // 2
    assert len(np.unique(case["pix"])) == P, "every entry a pixel of its own"


@pytest.mark.parametrize("name,E,pb", [("runs", 0, None), ("fan", 3, 1), ("holes", 2, None)])
def test_exact_mode_is_exact_in_fp32_in_any_order(name, E, pb):
    """The forward in plain fp32 torch equals the float64 reference; every gradient-row term is exact in fp32 and the fp32 sums in
    list order, reversed and shuffled are the same numbers as the float64 sums."""
    case = _case(name, "small", 257 if name == "holes" else None)
    t = G.exact_tensors(case, E=E, prior_batch=pb)
    out, ex, live = G.forward_reference(case, t)
    assert torch.equal(out[:, [0, 1, 2, 6, 7, 8, 9, 10, 11]].float().double(), out[:, [0, 1, 2, 6, 7, 8, 9, 10, 11]])
    _, idx, rows, bary, _ = G.gather(case, t["rast"])
    b32 = bary.float()
    got = (b32[..., None] * t["v_nrm"].reshape(-1, 3)[rows]).sum(1)
    assert torch.equal(got.double(), out[idx, 6:9])
    assert torch.equal(out[~live], torch.zeros_like(out[~live]))
    ref, g_rast, _, _ = G.backward_reference(case, t)
    assert torch.equal(ref.float().double(), ref) and torch.equal(g_rast.float().double(), g_rast)
    assert torch.equal(g_rast, g_rast.round()), "(gu, gv) are integers"
    terms = (b32[..., None] * t["g_out"][idx][:, None, 6:9]).reshape(-1, 3)
    flat = rows.reshape(-1)
    for order in (torch.arange(len(flat)), torch.arange(len(flat)).flip(0), torch.from_numpy(np.random.default_rng(0).permutation(len(flat)))):
        s32 = torch.zeros(case["B"] * case["V"], 3).index_add_(0, flat[order], terms[order])
        assert torch.equal(s32.double(), ref[:, 3:6])
    assert torch.equal(ref[:, 12:], torch.zeros_like(ref[:, 12:]))
    if not E:
        assert torch.equal(ref[:, 9:12], torch.zeros_like(ref[:, 9:12]))


def _normal_case(seed=0):
    """'unique' (private vertices) with a quarter of the triangles near the 1e-20 clamp of d = |cross|^2: d a factor >= 4 above resp.
    below, so that fp32 and float64 take the same branch."""
    case = _case("unique", "small", seed=seed)
    above = [(tr, (4e-20 * (4 + tr % 5)) ** 0.25) for tr in range(0, 64, 2)]
    below = [(tr, (1e-20 / (8 + tr % 5)) ** 0.25) for tr in range(1, 64, 2)]
    return case, G.normal_tensors(case, seed, tiny=above + below), [a[0] for a in above], [b_[0] for b_ in below]


def test_near_degenerate_triangles_sit_a_factor_4_from_the_clamp():
    case, t, above, below = _normal_case()
    p = t["v_pos"].double()[:, torch.from_numpy(case["tri"])]  # [B,F,3,3]
    n = torch.cross(p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 0], dim=-1)
    d = (n * n).sum(-1)
    assert bool((d[:, above] >= 4e-20).all()) and bool((d[:, above] <= 1e-17).all())
    assert bool((d[:, below] <= 2.5e-21).all()) and bool((d[:, below] > 0).all())
    assert bool((d[:, 64:] > 1e-6).all())


def test_err_chain_reproduces_autograd():
    """vpos_terms restates gb_pixel_adjoint: its values are the float64 autograd terms (both clamp branches)."""
    case, t, _, _ = _normal_case()
    ref, bound, feeds, val, rows, terms_ref = G.vpos_bound(case, t)
    scale = terms_ref.abs().amax(-1, keepdim=True)
    assert bool(((val - terms_ref).abs() <= 1e-9 * scale + 1e-300).all())
    assert bool((bound[feeds > 0] > 0).all()) and bool((bound[feeds == 0] == 0).all())


@pytest.mark.parametrize("name", ["runs", "fan", "period8"])
def test_vpos_bound_catches_one_dropped_contribution(name):
    """Sensitivity self-check: the float64 reference with ONE (entry, corner) term removed -- the one of median magnitude among those
    that feed the row -- must fall outside the bound of columns 0..2, at a sample of rows fed by more than one term."""
    case = _case(name, "small", seed=3)
    t = G.normal_tensors(case, 3)
    ref, bound, feeds, val, rows, _ = G.vpos_bound(case, t)
    assert not bool(((ref - ref).abs() > bound).any())
    fed = (feeds > 1).nonzero().reshape(-1)
    rng = np.random.default_rng(3)
    sample = fed[torch.from_numpy(rng.permutation(fed.numel())[:16])]
    assert sample.numel() >= 1
    for r in sample.tolist():
        where = (rows == r).nonzero()
        size = val[where[:, 0], where[:, 1]].abs().amax(-1)
        pick = where[int(torch.argsort(size)[size.numel() // 2])]
        dropped = ref[r] - val[pick[0], pick[1]]
        assert bool(((dropped - ref[r]).abs() > bound[r]).any()), (name, r, int(feeds[r]), (dropped - ref[r]).tolist(), bound[r].tolist())


def test_attr_bound_catches_one_dropped_contribution():
    case = _case("runs", "small", seed=4)
    t = G.normal_tensors(case, 4)
    ref, _, _, rows = G.backward_reference(case, t)
    bound = G.attr_bound(case, t)
    _, idx, _, bary, _ = G.gather(case, t["rast"])
    terms = bary[..., None] * t["g_out"].double()[idx][:, None, 6:9]
    size = terms.abs().amax(-1).reshape(-1)
    k = int(torch.argsort(size)[size.numel() // 2])  # the (entry, corner) term of median magnitude
    e, c = k // 3, k % 3
    r = int(rows[e, c])
    assert bool((terms[e, c].abs() > bound[r, 0:3]).any()), (terms[e, c].tolist(), bound[r].tolist())
