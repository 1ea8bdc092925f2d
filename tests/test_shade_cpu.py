"""tests/shade_ref.py checked on the CPU: the restated shading equals the project's oracle (pinned on the reference's goldens), the
generated inputs keep clear of the kinks, the hand-placed points sit on the side they are meant for in float32 and float64 alike, the
per-image lists have the boundaries they promise, and the reduction bound catches one dropped point."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shade_ref as S  # noqa: E402

SEEDS = (11, 12, 13)  # the generated sets of tests/test_shade_adversarial_gpu.py
P_GEN = 8192
F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("two_sided", [True, False])
def test_shade_is_the_oracles_shading(two_sided):
    from oracle import mesh_ref, render_ref

    gb, rot, view, light, kd = [x.double() for x in S.make_points(2000, 5)]
    nrm, shading, shaded = S.shade(gb, rot, view, light, kd, two_sided)
    want = render_ref.shading_normal(gb[:, 0:3], view, gb[:, 6:9], gb[:, 3:6], two_sided)
    assert torch.equal(nrm, want)
    cam = mesh_ref.safe_normalize((rot * want[:, None, :]).sum(-1))
    sh = light[:, 3:4] + light[:, 4:5] * torch.clamp((light[:, 0:3] * cam).sum(-1, keepdim=True), min=0.0)
    assert torch.equal(shading, sh) and torch.equal(shaded, sh * kd)


@pytest.mark.parametrize("two_sided", [True, False])
@pytest.mark.parametrize("seed", SEEDS)
def test_generated_inputs_stay_under_the_kink_cap(seed, two_sided):
    """The share of points left out of the gradient comparison is capped at 1 %; the generated sets alone use far less."""
    bad = S.near_kink(S.make_points(P_GEN, seed), two_sided)
    assert float(bad.double().mean()) <= 0.01 / 4, float(bad.double().mean())


def test_twin_is_close_to_float64_away_from_kinks():
    inputs, w = S.make_points(P_GEN, SEEDS[0]), S.make_weights(P_GEN, SEEDS[0])
    keep = ~S.near_kink(inputs)
    (o32, g32), (o64, g64) = S.run(inputs, w, True, F32), S.run(inputs, w, True, F64)
    for a, b in zip(o32, o64):
        assert float((a.double() - b).abs().max()) < 1e-5
    for a, b in zip(g32, g64):
        scale = b.abs().reshape(P_GEN, -1).amax(-1).clamp(min=1.0)
        assert float(((a.double() - b).abs().reshape(P_GEN, -1).amax(-1) / scale)[keep].max()) < 1e-3


@pytest.mark.parametrize("two_sided", [True, False])
def test_kink_points_take_the_intended_side_in_both_precisions(two_sided):
    inputs, group, names = S.kink_points()
    n = group.numel()
    assert set(names) == {"dot(geo, v) = 0", "t_raw = 0", "t_raw = 1", "t = 0.5", "l = 0", "|a| at 1e-12", "qq at 1e-20", "view == pos"}
    w = S.make_weights(n, 1)
    (o32, g32), (o64, g64) = S.run(inputs, w, two_sided, F32), S.run(inputs, w, two_sided, F64)
    for a, b in zip(o32 + g32, o64 + g64):
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
    gb, rot, view, light, kd = inputs
    sel = lambda name: (group == names.index(name)).nonzero().reshape(-1)
    # l = 0: below -> shading == ambient and no gradient to the light direction; on and above -> the clamp passes it
    s = sel("l = 0")
    d = light[s, 2]
    for o, g in ((o32, g32), (o64, g64)):
        assert bool((o[1][s][d < 0, 0] == light[s][d < 0, 3].to(o[1].dtype)).all())
        assert bool((g[3][s][d < 0, 0:3] == 0).all()) and bool((g[3][s][d >= 0, 0:3].abs().amax(-1) > 0).all())
    # dot(geo, v) = 0: two-sided flips geo and the normal for d <= 0 (the shading normal's sign follows the face normal's side)
    s = sel("dot(geo, v) = 0")
    d = gb[s, 5]
    for o in (o32, o64):
        flipped = o[0][s, 0] < 0  # unflipped: t = 1 and the normal is the smooth one (x > 0); flipped: t = 0 and it is -geo (x = -0.8)
        assert bool((flipped == ((d <= 0) if two_sided else torch.zeros_like(d, dtype=torch.bool))).all())
    # t_raw = 0: below the clamp the smooth normal gets no gradient through t; qq: below the floor cam = q * 1e10
    s = sel("t_raw = 0")
    d = gb[s, 8]
    for o in (o32, o64):
        assert bool((o[0][s][d <= 0] == gb[s][d <= 0, 3:6].to(o[0].dtype)).all()), "t = 0: the shading normal IS the face normal"
    # |a| below 1e-12 / a = 0 and view == pos: finite everywhere (checked above), a = 0 gives the face normal
    s = sel("|a| at 1e-12")
    assert bool((o64[0][s[0]] == gb[s[0], 3:6].double()).all())


def test_image_list_has_the_promised_boundaries():
    img = S.image_list(1000)
    assert bool((img[1:] >= img[:-1]).all()) and img.numel() == 1000
    assert (int(img[15]), int(img[16]), int(img[63]), int(img[64]), int(img[255]), int(img[256])) == (0, 1, 1, 2, 2, 4)
    assert len(img[:256].unique()) == 3 and not bool((img == 3).any()) and not bool((img == 7).any())
    assert int((img == 5).sum()) == 1 and int(img[356]) == 5 and 256 < 356 < 511
    for P in (1, 255, 256, 257):
        assert torch.equal(S.image_list(P), img[:P])
    assert torch.equal(S.image_list(300, B=1), torch.zeros(300, dtype=torch.int64))
    pix = S.pix_of(img, 960)
    assert torch.equal(pix // 960, img)


@pytest.mark.parametrize("shared", [False, True])
def test_reduction_bound_catches_one_dropped_point(shared):
    """The comparison of the per-image sums, applied to the float64 sum with ONE point of median magnitude removed, must fail at every
    image (the twin's float32 per-point rows stand in for the kernel's)."""
    P, B = 1000, 10
    inputs, w = S.make_points(P, 3), S.make_weights(P, 3)
    _, g32 = S.run(inputs, (None, None, w[2]), True, F32)
    per_point = torch.cat((g32[1].reshape(P, 9), g32[2], g32[3]), -1)
    img = S.image_list(P, B)
    ref, bound = S.reduction_reference(per_point, img, B, shared)
    assert ref.shape == ((1, 17) if shared else (B, 17)) and not bool(((ref - ref).abs() > bound).any())
    for b in ([0] if shared else [0, 1, 2, 4, 6, 8, 9]):
        members = torch.arange(P) if shared else (img == b).nonzero().reshape(-1)
        size = per_point[members].abs().amax(-1)
        drop = members[int(torch.argsort(size)[size.numel() // 2])]
        dropped = ref[b] - per_point[drop].double()
        assert bool(((dropped - ref[b]).abs() > bound[b]).any()), (b, (dropped - ref[b]).tolist(), bound[b].tolist())
    if not shared:
        assert torch.equal(ref[3], torch.zeros(17, dtype=F64)) and torch.equal(bound[7], torch.zeros(17, dtype=F64))
