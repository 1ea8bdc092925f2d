"""tests/losses_ref.py pinned and measured, on the CPU: the float64 restatement of the reconstruction and flow losses against the
reference's own outputs (tests/golden/recon_losses.npz) and central differences; what the cases claim to contain; the float32
evaluation's error against float64 on every case tests/test_losses_adversarial_gpu.py runs (losses_ref.MEASURED: the kernels' bounds
are 4 x these figures); a check that the bounds bite -- a float32 evaluation with one piece wrong falls outside them; and the
knife-edge conditions ``build`` enforces.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import losses_ref as S  # noqa: E402


def measure(name):
    """key -> units of the float32 evaluation on one case (every element); the discrete results must agree exactly."""
    torch.set_num_threads(1)
    c = S.build(name)
    ref, got = S.reference(c), S.evaluate(c, torch.float32)
    assert torch.equal(got["mask"], ref["mask"]), name
    if c["F"] > 1:
        assert torch.equal(got["dropped"], ref["dropped"]), name
    return {k: S.units(got[k], *ref[k]) for k in S.keys_of(c)}


def measure_all():
    """The table losses_ref.MEASURED is written from: python tests/test_losses_cpu.py (third decimal rounded up)."""
    return {n: {k: float(np.ceil(u * 1000) / 1000) for k, u in measure(n).items()} for n in S.CASES}


@pytest.fixture(scope="module")
def fresh():
    return {n: measure(n) for n in S.CASES}


def test_measured_table_is_current(fresh):
    """Every figure of losses_ref.MEASURED against a fresh measurement: not below it (third decimal rounded up), not more than the
    rounding above it -- with a relative slack of 1e-3 for another summation order."""
    assert sorted(S.MEASURED) == sorted(S.CASES)
    for n, row in fresh.items():
        assert sorted(row) == sorted(S.MEASURED[n]), n
        for k, u in row.items():
            print(f"{n}: {k} {u:.4f} units (table {S.MEASURED[n][k]})")
            assert np.isfinite(u), (n, k)
            assert u <= S.MEASURED[n][k] * (1 + 1e-3) + 1e-9 and S.MEASURED[n][k] <= u * (1 + 1e-3) + 1.001e-3, (n, k, u, S.MEASURED[n][k])


# ---------------------------------------------------------------------------------------------------------------- pins
def _golden_case(tag):
    g = golden("recon_losses.npz")
    t = lambda k: torch.from_numpy(g[f"{tag}_in_{k}"])
    B, Fr, _, H, W = g[f"{tag}_in_image_pred"].shape
    N = B * Fr
    c = dict(B=B, F=Fr, H=H, W=W, D=16, N=N, dt1=True, w_loss=torch.ones(N, 5))
    c["shaded"] = torch.cat([t("image_pred").view(N, 3, H, W), t("mask_pred").view(N, 1, H, W)], 1).permute(0, 2, 3, 1).contiguous()
    c["feat"], c["feat_gt"] = t("dino_pred").view(N, 16, H, W).permute(0, 2, 3, 1).contiguous(), t("dino_gt").view(N, 16, H, W)
    c["image_gt"], c["mask_gt"], c["mask_dt"], c["valid"] = t("image_gt").view(N, 3, H, W), t("mask_gt").view(N, H, W), t("mask_dt").view(N, 2, H, W), \
        t("mask_valid").view(N, H, W)
    if f"{tag}_in_flow_pred" in g.files:
        c["flow"] = torch.cat([t("flow_pred"), torch.zeros(B, 1, 2, H, W)], 1).view(N, 2, H, W).permute(0, 2, 3, 1).contiguous()
        c["flow_gt"], c["w_flow"] = t("flow_gt"), torch.ones(B, Fr - 1)
    else:
        c["F"], c["B"] = 1, N  # (no flow: the frames are independent)
    return c, g, (B, Fr)


@pytest.mark.parametrize("tag", ["b3f1", "b2f4_flow"])
def test_restatement_matches_reference_golden(tag):
    """All six terms of both fixtures, which hold the reference implementation's own float32 outputs: sums of at most 16 x 256 terms
    of one sign, so the fixtures carry a few 2^-24 of relative error -- rtol 2e-6."""
    c, g, (B, Fr) = _golden_case(tag)
    S.check_knife_edges(c)
    ev = S.evaluate(c)
    for col, key in enumerate(("mask_loss", "mask_inv_dt_loss", "rgb_loss", "dino_feat_im_loss", "mask_dt_loss")):
        np.testing.assert_allclose(ev["loss"][:, col].view(B, Fr).numpy(), g[f"{tag}_out_{key}"], rtol=2e-6, atol=1e-9, err_msg=key)
    if "flow" in ev:
        want = g[f"{tag}_out_flow_loss"]
        assert (want == 0).any() and (want > 0).any() and np.array_equal(ev["dropped"].numpy(), want == 0)
        np.testing.assert_allclose(ev["flow"].numpy(), want, rtol=2e-6, atol=1e-9)
    else:
        assert f"{tag}_out_flow_loss" not in g.files


@pytest.mark.parametrize("name", ["hw_16x16_b3", "flow_b1_f4_stride3", "no_dt1_sum", "d3"])
def test_restatement_gradients_match_central_differences(name):
    """Step h = 1e-6 on inputs of size <= 1.5 at pixels away from the discrete decisions (alpha >= 0.2, |rgb - image_gt| >= 1e-3): the
    losses are quadratic or piecewise linear there, so the central difference has no truncation error and a rounding error of
    2^-53 x |total| / h ~ 1e-9; tolerance 1e-7 x the gradient's scale.  The alpha gradient also equals the sum of its three terms."""
    c = S.build(name)
    ev = S.evaluate(c)
    assert float((S.alpha_terms(c).sum(0) - ev["g_alpha"]).abs().max()) <= 1e-15 * max(1.0, float(ev["g_alpha"].abs().max()))

    def total(shaded, feat, flow):
        loss, both = S.recon_losses(c, shaded, feat)
        t = (loss * c["w_loss"].double()).sum()
        return t + (S.flow_losses(c, flow, both)[0] * c["w_flow"].double()).sum() if c["F"] > 1 else t

    x = [c["shaded"].double(), c["feat"].double() if c["D"] else None, c["flow"].double() if c["F"] > 1 else None]
    g_shaded = torch.cat([ev["g_rgb"], ev["g_alpha"][..., None]], -1)
    grads = [g_shaded, ev.get("g_feat"), ev.get("g_flow")]
    ok = [torch.cat([(x[0][..., :3] - c["image_gt"].double().permute(0, 2, 3, 1)).abs() >= 1e-3, x[0][..., 3:] >= 0.2], -1), None, None]
    rng = np.random.default_rng(5)
    h, tried = 1e-6, 0
    for which in range(3):
        if x[which] is None:
            continue
        scale = max(1.0, float(grads[which].abs().max()))
        for _ in range(16):
            i = tuple(int(rng.integers(0, n)) for n in x[which].shape)
            if ok[which] is not None and not bool(ok[which][i]):
                continue
            e = torch.zeros_like(x[which])
            e[i] = h
            args_p, args_m = list(x), list(x)
            args_p[which], args_m[which] = x[which] + e, x[which] - e
            with torch.no_grad():
                d = float(total(*args_p) - total(*args_m)) / (2 * h)
            assert abs(d - float(grads[which][i])) <= 1e-7 * scale, (name, which, i, d, float(grads[which][i]))
            tried += 1
    assert tried >= 16


# ---------------------------------------------------------------------------------------------------------------- the cases
def _interior(N, H, W):
    m = torch.zeros(N, H, W, dtype=torch.uint8)
    m[:, 1:H - 1, 1:W - 1] = 1
    return m


def test_cases_contain_what_they_name():
    """All-ones and all-0.995 targets give exactly the interior (zero padding), all-0.98 the empty mask, a single zero its 3 x 3 hole
    and nothing else; the frames of a case differ; every pair kind does what it says (empty: no mask pixel, one: exactly one, half /
    offmask kept, over0 / over1 dropped, offmask with a large value on the next frame's mask), and the list of shapes, feature widths
    and pair kinds is complete."""
    shapes, widths, seen = set(), set(), set()
    for name, s in S.CASES.items():
        c = S.build(name)
        ref = S.reference(c)
        N, H, W, mask = c["N"], c["H"], c["W"], ref["mask"]
        shapes.add((H, W, s["B"]))
        widths.add((s["D"], s["layout"]))
        for a in range(N):
            for b in range(a + 1, N):
                assert not torch.equal(c["shaded"][a], c["shaded"][b]) and not torch.equal(c["image_gt"][a], c["image_gt"][b]), name
        if s["alpha"] == "positive" and s["mask"] in ("ones", "0.995"):
            assert torch.equal(mask, _interior(N, H, W)), name
        if s["mask"] == "0.98":
            assert int(mask.sum()) == 0, name
        if s["mask"] == "hole":
            want = _interior(N, H, W)
            for n in range(N):
                y, x = s["hole"][n % len(s["hole"])]
                want[n, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 0
            assert torch.equal(mask, want), name
        if s["rgb"] == "ties":
            d = c["shaded"][..., :3] - c["image_gt"].permute(0, 2, 3, 1)
            on = mask.bool()
            assert bool(((d == 0).sum(-1) == 1)[on].all()) and bool(((d > 0).sum(-1) == 1)[on].all()) and int(on.sum()) > 0, name
            assert bool((ref["g_rgb"][0][d == 0] == 0).all())
        if not s["dt1"]:
            assert bool((ref["loss"][0][:, 4] == 0).all()), name
        if s["F"] > 1 and H >= 3 and W >= 3:
            B, Fr = s["B"], s["F"]
            counts = mask.view(B, Fr, -1)[:, :-1].sum(2).reshape(-1)
            for p, kind in enumerate(c["kinds"]):
                seen.add(kind)
                dropped = bool(ref["dropped"].reshape(-1)[p])
                if kind == "empty":
                    assert int(counts[p]) == 0 and not dropped and float(ref["flow"][0].reshape(-1)[p]) == 0.0, (name, p)
                else:
                    assert int(counts[p]) == 1 if kind == "one" else int(counts[p]) > 1, (name, p, kind)
                    assert dropped == (kind in ("over0", "over1")), (name, p, kind)
                if kind == "offmask":
                    n = (p // (Fr - 1)) * Fr + p % (Fr - 1)
                    big = (c["flow_gt"].reshape(-1, 2, H, W)[p].abs() > 0.5).any(0)
                    assert not bool((big & mask[n].bool()).any()) and bool((big & mask[n + 1].bool()).any()), (name, p)
                if dropped:
                    n = (p // (Fr - 1)) * Fr + p % (Fr - 1)
                    assert float(ref["flow"][0].reshape(-1)[p]) == 0.0 and float(ref["g_flow"][0][n].abs().max()) == 0.0, (name, p)
    for hw in ((1, 1), (1, 7), (9, 1), (3, 85), (16, 16), (257, 1), (1, 257), (2, 300), (200, 3), (130, 130), (17, 33)):
        assert hw + (1,) in shapes and hw + (3,) in shapes, hw
    for d in (0, 1, 3, 5, 4, 8, 12, 20, 16, 260):
        assert (d, "contig") in widths, d
    assert (16, "wide17") in widths and (16, "offset1") in widths and seen == set(S.ALL_PAIRS)


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _outside(got, ref, name, c):
    """Does an evaluation fall outside what a kernel is allowed on case ``name``: an integer result differs, or a float one violates."""
    if not torch.equal(got["mask"], ref["mask"]) or (c["F"] > 1 and not torch.equal(got["dropped"], ref["dropped"])):
        return True
    return any(S.bad_elements(got[k].float(), *ref[k], name, k).numel() > 0 for k in S.keys_of(c))


@pytest.mark.parametrize("wrong,name", [("no_pad", "mask_ones"), ("no_pad", "hw_9x1_n1"), ("flow_count", "flow_b1_f2"), ("flow_count", "hw_16x16_b3"),
                                        ("large_whole_frame", "flow_b1_f4_stride3"), ("large_whole_frame", "hw_130x130_b3"), ("rgb_hw", "d_none"),
                                        ("rgb_hw", "rgb_wide"), ("pair_frame", "flow_b3_f4"), ("pair_frame", "hw_17x33_b3"), ("sign0", "rgb_ties"),
                                        ("sign0", "hw_16x16_n1")])
def test_bounds_catch_a_wrong_piece(wrong, name):
    """The float32 evaluation is inside every bound of the case; with one piece wrong it is not: erosion without zero padding, the
    flow normaliser count instead of 2 count, the large-flow test over the whole frame, the rgb normaliser HW instead of 3 HW, pair
    (b, f) read from frame ``pair``, sign(0) = 1."""
    assert wrong in S.WRONG
    c = S.build(name)
    ref = S.reference(c)
    assert not _outside(S.evaluate(c, torch.float32), ref, name, c), name
    assert _outside(S.evaluate(c, torch.float32, wrong=wrong), ref, name, c), (wrong, name)


def test_build_rejects_a_case_on_a_knife_edge():
    """A 3 x 3 sum of nine 0.99s, a |flow_gt| of 0.52 or of the float below 0.5, a fractional valid beside a tiny alpha, a denormal
    alpha: each is refused; the untouched case passes."""
    base = lambda: S.build("flow_b1_f2", check=False)
    S.check_knife_edges(base())

    def refused(change, match):
        c = base()
        change(c)
        with pytest.raises(AssertionError, match=match):
            S.check_knife_edges(c)

    def nine(c):
        c["mask_gt"][:] = 0.99
        c["shaded"][..., 3] = 1.0
        c["valid"][:] = 1.0

    refused(nine, "3 x 3 sum")
    refused(lambda c: c["flow_gt"].view(-1).__setitem__(3, 0.52), "flow_gt")
    refused(lambda c: c["flow_gt"].view(-1).__setitem__(3, float(np.nextafter(np.float32(0.5), np.float32(0)))), "flow_gt")

    def tiny(c):
        c["shaded"][0, 2, 2, 3] = 2.0 ** -126
        c["valid"][0, 2, 2] = 0.5

    refused(tiny, "fractional valid")
    refused(lambda c: c["shaded"].__setitem__((0, 2, 2, 3), 2.0 ** -130), "denormal")
    # 8 x 0.995 and 9 x 0.98 lie far below the threshold, 9 x 0.995 far above: none is refused
    for v in (0.995, 0.98):
        c = base()
        c["mask_gt"][:] = v
        S.check_knife_edges(c)


if __name__ == "__main__":
    print("MEASURED = {")
    for n, row in measure_all().items():
        print(f'    "{n}": {row},')
    print("}")
