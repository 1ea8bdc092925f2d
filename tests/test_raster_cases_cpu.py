"""The rasteriser's adversarial cases (tests/raster_cases.py) and its three references held against one another; no GPU involved.

  * every case forces what its ``forces`` entry claims, by a restatement of the box formula (raster_cases.boxes) and of the triangle
    launch's work-group composition (raster_cases.workgroups): boxes up to / above RS_BIG, tiles and chunks per work-group, the
    (image, triangle) pair count against the two lanes-per-triangle thresholds, the fullest big-box list;
  * in the tile-stage cases at least ``tile_share`` of the covered pixels belong to triangles whose box exceeds RS_BIG (a quarter on the
    spiky mesh, half or more elsewhere): the tile test and the row spans decide pixels that are seen;
  * the boxed oracle (oracle/raster_ref.c, a3d_ref_rasterize) equals the box-free one (a3d_ref_rasterize_whole) bit for bit on EVERY
    case -- none had to be set aside for the boxed comparison: the oracle's pixel box loses no pixel here;
  * the box-free oracle agrees with the float64 statement of the definition (tests/raster_fwd_ref.py) in coverage and winner on every
    pixel the statement does not mark ambiguous; ambiguous pixels are at most 1 % of a case's frame, and every case other than the bad
    input has covered pixels;
  * depth peeling: layer n of the oracle, boxed and box-free, is entry n of the box-free fragment list (a3d_ref_fragments), down to
    the empty layer.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_cases as RC  # noqa: E402
import raster_fwd_ref as RF  # noqa: E402

AMBIGUOUS_SHARE = 0.01  # of a case's frame (the issue's condition)


def _ids(rast):
    return rast[..., 3].numpy().astype(np.int64) - 1


def test_names_are_the_cases():
    assert sorted(RC.NAMES) == sorted(RC.all_cases()) and set(RC.PEEL_NAMES) == {n for n, c in RC.all_cases().items() if c["peel"]}


@pytest.mark.parametrize("name", RC.NAMES)
def test_case_forces_what_it_claims(name):
    c = RC.all_cases()[name]
    H, W, B, F = c["H"], c["W"], c["B"], c["tri"].shape[0]
    fo = c["forces"]
    assert c["clip"].dtype == torch.float32 and c["tri"].dtype == torch.int32 and c["clip"].shape[0] in (1, B)
    assert 1 <= H <= 256 and 1 <= W <= 256
    lpt = RC.lanes_per_triangle(B, F)
    ids = _ids(RC.reference(name)["whole"])
    for b in range(min(c["clip"].shape[0], 2)):
        box, straddle = RC.boxes(c["clip"][b].numpy(), c["tri"].numpy(), H, W)
        wgs = RC.workgroups(box, lpt)
        big = box[:, 4] > RC.RS_BIG
        if "box" in fo:
            bw, bh = fo["box"]
            assert int(((box[:, 2] == bw) & (box[:, 3] == bh)).sum()) == fo["n_box"]
            assert (bw * bh > RC.RS_BIG) == (fo["n_big"] > 0)
        if "n_big" in fo:
            assert int(big.sum()) == fo["n_big"], int(big.sum())
        if "nbig_fullest" in fo:
            assert max(w["nbig"] for w in wgs) == fo["nbig_fullest"]
        if "chunks" in fo:
            assert max(w["chunks"] for w in wgs) == fo["chunks"]
        if "slices" in fo:
            assert len(wgs) == 1 and wgs[0]["slices"] == fo["slices"]
        if "full_chunks" in fo:
            # one triangle with >= 2 chunks' worth of tiles, every one of them wholly inside it: wherever the chunk boundaries fall in
            # the work-group's tile list, at least one chunk (two when the triangle comes first) holds RS_TILE_CHUNK survivors
            tiles = ((box[:, 2] + 7) // 8) * ((box[:, 3] + 7) // 8)
            f = int(np.argmax(tiles))
            assert tiles[f] == fo["full_chunks"] * RC.RS_TILE_CHUNK and box[f, 2] == W and box[f, 3] == H
            st = RF.rasterize(c["clip"][b].numpy(), c["tri"].numpy()[f:f + 1], H, W)
            assert bool(st["inside"][0].all()) and not bool(st["amb"][0].any())
        if "straddlers" in fo:
            assert int(straddle.sum()) >= fo["straddlers"]
        if fo.get("tile_share") is not None:
            won = ids[b][ids[b] >= 0]
            share = float(big[won].mean())
            assert share >= fo["tile_share"], share
            assert max(w["nbig"] for w in wgs) > 0
    if "pairs" in fo:
        assert B * F == fo["pairs"] and lpt == fo["lpt"]
        assert {"lpt_300000": B * F == RC.LPT_PAIRS_4, "lpt_300240": RC.LPT_PAIRS_4 < B * F <= RC.LPT_PAIRS_4 + F,
                "lpt_600000": B * F == RC.LPT_PAIRS_2, "lpt_600240": RC.LPT_PAIRS_2 < B * F <= RC.LPT_PAIRS_2 + F}.get(name, True)
    else:
        assert lpt == 4
    if "F" in fo:
        assert F == fo["F"]
    if "bad_rows" in fo:
        t = c["tri"].numpy()
        assert int(np.any((t < 0) | (t >= c["clip"].shape[1]), axis=1).sum()) == fo["bad_rows"]
    present = set(np.unique(ids[ids >= 0]).tolist())
    assert set(fo.get("winners", ())) <= present and set(fo.get("kept", ())) <= present
    assert not (set(fo.get("losers", ())) | set(fo.get("clipped", ()))) & present
    if name == "signed_zero_pair":
        assert present == fo["winners"]  # the oracle's rule: -0 == +0, the lower id owns the pixel
    if "frame" in fo:
        assert (H, W) == fo["frame"]
    if fo.get("nonfinite"):
        assert not bool(torch.isfinite(c["clip"]).all())
    else:
        assert bool(torch.isfinite(c["clip"]).all())
    assert name != "frame_8x32" or H * W == 256
    assert name not in ("frame_5x3", "frame_50x70", "frame_24x40") or (H * W) % 256 != 0


@pytest.mark.parametrize("name", RC.NAMES)
def test_boxed_oracle_equals_box_free_oracle(name):
    ref = RC.reference(name)
    assert np.array_equal(_ids(ref["boxed"]), _ids(ref["whole"]))
    assert np.array_equal(ref["boxed"].numpy(), ref["whole"].numpy())
    assert np.array_equal(np.signbit(ref["boxed"].numpy()), np.signbit(ref["whole"].numpy()))


@pytest.mark.parametrize("name", RC.NAMES)
def test_box_free_oracle_agrees_with_the_float64_statement(name):
    c = RC.all_cases()[name]
    H, W = c["H"], c["W"]
    whole = RC.reference(name)["whole"]
    for b in range(min(c["clip"].shape[0], 2)):  # (the per-image-clip case: its first two images)
        st = RF.rasterize(c["clip"][b].numpy(), c["tri"].numpy(), H, W)
        ids = _ids(whole[b])
        sure = ~st["pixel_amb"]
        n_amb = int(st["pixel_amb"].sum())
        print(f"{name}[{b}]: covered {int((ids >= 0).sum())} of {H * W}, ambiguous {n_amb}")
        assert n_amb <= AMBIGUOUS_SHARE * H * W, (n_amb, H * W)
        assert np.array_equal((ids >= 0)[sure], (st["winner"] >= 0)[sure])  # coverage
        assert np.array_equal(ids[sure], st["winner"][sure])  # winner
        # a pair the statement is sure of is inside for the oracle too: the winner's own pair is never 'surely outside'
        won = ids >= 0
        pair_in = st["inside"][np.clip(ids, 0, None), np.arange(H)[:, None], np.arange(W)[None, :]]
        pair_amb = st["amb"][np.clip(ids, 0, None), np.arange(H)[:, None], np.arange(W)[None, :]]
        assert bool((pair_in | pair_amb)[won].all())
        zw = whole[b][..., 2].numpy().astype(np.float64)
        assert float(np.abs(zw - st["zw"])[sure & won].max(initial=0.0)) < 1e-4 or c["group"] == "bad"
        if c["group"] != "bad":
            assert int(won.sum()) > 0


@pytest.mark.parametrize("name", RC.PEEL_NAMES)
def test_peeled_layers_are_the_fragment_list(name):
    from oracle import raster_ref

    c = RC.all_cases()[name]
    H, W = c["H"], c["W"]
    count, zw, ids = RC.peel_reference(name)
    depth = int(count.max())
    assert depth >= 1
    prev_w = prev_b = None
    for n in range(depth + 1):
        lw = raster_ref.rasterize(c["clip"], c["tri"], (H, W), prev=prev_w, whole_frame=True)
        lb = raster_ref.rasterize(c["clip"], c["tri"], (H, W), prev=prev_b)
        assert np.array_equal(lw.numpy(), lb.numpy()), n
        assert np.array_equal(_ids(lw), np.where(count.numpy() > n, ids[..., n].numpy(), -1)), n
        assert np.array_equal(lw[..., 2].numpy(), np.where(count.numpy() > n, zw[..., n].numpy(), 0.0)), n
        prev_w, prev_b = lw, lb
    assert not bool((lw[..., 3] > 0).any())  # the empty layer
    assert bool((count == 0).any()) or name in ("frame_256_full", "slivers_far", "box_529_23x23")  # (a previous layer with empty pixels)


def test_float64_statement_on_a_frame_worked_by_hand():
    """4 x 4 pixels, centres at (k + 0.5) / 2 - 1.  Triangle 0: the lower-left half below x + y = 4.2 px (z/w = 0.25); triangle 1: the whole
    frame behind it (z/w = 0.5) and triangle 2 coplanar with it (the tie goes to 1); triangle 3 in front but beyond the near plane."""
    px = lambda x, y, z, w=1.0: ((2 * x / 4 - 1) * w, (2 * y / 4 - 1) * w, z * w, w)
    clip = np.asarray([px(-1, -1, 0.25), px(5.2, -1, 0.25), px(-1, 5.2, 0.25), px(-9, -9, 0.5, 2.0), px(20, -9, 0.5, 0.5), px(-9, 20, 0.5), px(-9, -9, -1.5),
                       px(20, -9, -1.5), px(-9, 20, -1.5)], dtype=np.float32)
    tri = np.asarray([[0, 1, 2], [3, 4, 5], [3, 5, 4], [6, 7, 8]])
    st = RF.rasterize(clip, tri, 4, 4)
    expect = np.asarray([[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 1], [0, 1, 1, 1]])  # centre (x + 0.5) + (y + 0.5) < 4.2  <=>  x + y <= 3
    assert np.array_equal(st["winner"], expect) and not bool(st["pixel_amb"].any())
    assert bool(st["inside"][1].all()) and bool(st["inside"][2].all()) and not bool(st["inside"][3].any())
    # ... and the mask bites: move the hypotenuse onto the centres of the anti-diagonal
    clip[1], clip[2] = px(5.0, -1, 0.25), px(-1, 5.0, 0.25)
    st = RF.rasterize(clip, tri, 4, 4)
    assert np.array_equal(st["amb"][0], np.eye(4, dtype=bool)[::-1]) and np.array_equal(st["pixel_amb"], np.eye(4, dtype=bool)[::-1])
    # two depths closer than their bounds: the winner is ambiguous wherever both cover
    clip[3:6, 2] = clip[0, 2] * clip[3:6, 3] * np.float32(1 + 2.0 ** -22)
    clip[1], clip[2] = px(5.2, -1, 0.25), px(-1, 5.2, 0.25)
    st = RF.rasterize(clip, tri[:2], 4, 4)
    assert np.array_equal(st["winner_amb"], expect == 0)
