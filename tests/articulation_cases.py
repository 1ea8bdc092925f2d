"""The cases of the articulation tests (tests/test_articulation_cpu.py, tests/test_articulation_gpu.py, the golden generator): seeded
inputs as float32 CPU tensors, rebuilt identically wherever they are needed.  A case's seed is its rank among the sorted names.

Descriptor cases: the smallest shapes at which each mechanism of csrc/articulation.hip can go wrong -- C and D one below, at and one
above the kernel's column chunk (read from the package) and 1, K in {1, 5, 20, 64}, N in {1, 3}, bones shared and per image, 1x1, 3x5
and 32x32 patches, the three layouts, the three modes and feat=None, and hand-made coordinates through an identity-like mvp.
Limits cases: K in {1, 8, 20}, N in {1, 3, 1201}, special values of x.
"""
import importlib

import numpy as np
import torch

CHUNK = importlib.import_module("3danimals_amd._lib").ARTICULATION_CHUNK
Z_OFFSET, SPATIAL_SCALE = 10.0, 7.0  # cfg_render.cam_pos_z_offset / spatial_scale of the reference's model configs
LAYOUTS = ("nchw", "nhwc", "slice")


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _d(N, shared, K, C, D, h, w, layout, mode, feat=True, coords="random"):
    return dict(N=N, shared=shared, K=K, C=C, D=D, h=h, w=w, layout=layout, mode=mode, feat=feat, coords=coords)


DESC_CASES = {
    "n1_k1_c1_d1_1x1_nchw": _d(1, False, 1, 1, 1, 1, 1, "nchw", "sample+global"),
    "n3_k5_cbelow_dabove_3x5_nhwc_shared": _d(3, True, 5, CHUNK - 1, CHUNK + 1, 3, 5, "nhwc", "sample+global"),
    "n3_k20_cat_dbelow_32x32_nchw": _d(3, False, 20, CHUNK, CHUNK - 1, 32, 32, "nchw", "sample+global"),
    "n3_k64_cabove_dat_3x5_slice": _d(3, False, 64, CHUNK + 1, CHUNK, 3, 5, "slice", "sample+global"),
    "n1_k20_cabove_d1_32x32_nhwc": _d(1, False, 20, CHUNK + 1, 1, 32, 32, "nhwc", "sample+global"),
    "n3_k5_c1_dabove_1x1_slice_shared": _d(3, True, 5, 1, 2 * CHUNK + 1, 1, 1, "slice", "sample+global"),
    "n3_k5_sample_cat_3x5_nchw_shared": _d(3, True, 5, CHUNK, 4, 3, 5, "nchw", "sample"),
    "n3_k64_sample_c2above_32x32_nhwc": _d(3, False, 64, 2 * CHUNK + 1, 3, 32, 32, "nhwc", "sample"),
    "n3_k20_global_dabove_3x5_nchw": _d(3, False, 20, 7, CHUNK + 1, 3, 5, "nchw", "global"),
    "n3_k20_nofeat_shared": _d(3, True, 20, 0, 0, 1, 1, "nchw", "sample+global", feat=False),
    "hand_k20_c5_d3_4x8_nchw": _d(2, False, 20, 5, 3, 4, 8, "nchw", "sample+global", coords="hand"),
    "hand_k20_cabove_d3_4x8_nhwc": _d(2, False, 20, CHUNK + 1, 3, 4, 8, "nhwc", "sample+global", coords="hand"),
    "hand_k20_c5_d3_4x8_slice": _d(2, False, 20, 5, 3, 4, 8, "slice", "sample", coords="hand"),
}
# the cases whose inputs hold a NaN or an infinity on purpose, and the bones of their image 0 whose projected coordinate is not finite
NON_FINITE = tuple(n for n, s in DESC_CASES.items() if s["coords"] == "hand")
NON_FINITE_BONES = (11, 12, 13)


def layout_of(patch, layout):
    """``patch`` [N,C,h,w] (contiguous) in one of the three layouts, the same values: nchw as it is, nhwc a permuted view of an NHWC
    tensor (dense, channels innermost), slice channels 1..C of a [N,C+3,h,w] tensor (not dense)."""
    if layout == "nchw":
        return patch.clone()
    if layout == "nhwc":
        return patch.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert layout == "slice", layout
    wide = torch.full((patch.shape[0], patch.shape[1] + 3, *patch.shape[2:]), 7.0, dtype=patch.dtype, device=patch.device)
    wide[:, 1:1 + patch.shape[1]] = patch
    return wide[:, 1:1 + patch.shape[1]]


def camera(N, rng):
    """mvp with clip.w around 2.5 (the midpoints of bones in [-0.6, 0.6]^3 project into and around the image), w2c a rigid motion."""
    mvp = rng.normal(0.0, 1.0, (N, 4, 4))
    mvp[:, :2, :3] *= 2.0
    mvp[:, :2, 3] = rng.uniform(-0.5, 0.5, (N, 2))
    mvp[:, 3] = np.concatenate([rng.uniform(-0.3, 0.3, (N, 3)), rng.uniform(2.2, 2.8, (N, 1))], -1)
    q, _ = np.linalg.qr(rng.normal(size=(N, 3, 3)))
    w2c = np.zeros((N, 4, 4))
    w2c[:, :3, :3] = q
    w2c[:, :3, 3] = rng.uniform(-1.0, 1.0, (N, 3))
    w2c[:, 3, 3] = 1.0
    return _f32(mvp), _f32(w2c)


def hand_points(h, w, rng):
    """(x, y, z) of 2 x 20 midpoints under the hand camera (clip = (x, y, ., z): the coordinate is (x / z, y / z)).  Image 0: exact pixel
    centres, exactly -1 and +1, three quarters of and a whole pixel outside (some taps dropped), 1e6 and +-1e30, w < 0, a NaN, an
    infinity (z = 0) and 0 / 0; image 1: all twenty bones on one point."""
    cx = lambda i: (i + 0.5) * 2.0 / w - 1.0
    cy = lambda j: (j + 0.5) * 2.0 / h - 1.0
    pts = [(cx(0), cy(0), 1.0), (cx(w - 1), cy(h - 1), 1.0), (-1.0, -1.0, 1.0), (1.0, 1.0, 1.0), (-1.0 - 0.5 / w, cy(1), 1.0),
           (cx(2), 1.0 + 0.5 / h, 1.0), (-1.0 - 1.0 / w, -1.0 - 1.0 / h, 1.0), (1e6, 0.25, 1.0), (0.25, 1e30, 1.0), (-1e30, -1e30, 1.0),
           (0.5, -0.25, -2.0), (float("nan"), 0.0, 1.0), (0.3, 0.3, 0.0), (0.0, 0.0, 0.0), (cx(1), cy(2), 1.0), (1.0, -1.0, 1.0)]
    while len(pts) < 20:
        pts.append((rng.uniform(-1.2, 1.2), rng.uniform(-1.2, 1.2), 1.0))
    one = (rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), 1.0)
    return np.array([pts, [one] * 20], dtype=np.float64)


def build_desc(name):
    """dict(bones, mvp, w2c, feat | None, patch | None (contiguous values: ``layout_of(patch, layout)`` puts them into the case's layout
    on whichever device the test runs), mode, g (the upstream gradient of bones_feat) | None)."""
    s = DESC_CASES[name]
    rng = np.random.default_rng(9000 + sorted(DESC_CASES).index(name))
    N, K = s["N"], s["K"]
    if s["coords"] == "hand":
        pts = hand_points(s["h"], s["w"], rng)
        bones = _f32(np.stack([pts, pts], 2))  # a = b: the midpoint is the point itself
        mvp = torch.zeros(N, 4, 4)
        mvp[:, 0, 0] = mvp[:, 1, 1] = mvp[:, 2, 3] = mvp[:, 3, 2] = 1.0  # clip = (x, y, 1, z)
        _, w2c = camera(N, rng)
    else:
        bones = _f32(rng.uniform(-0.6, 0.6, (1 if s["shared"] else N, K, 2, 3)))
        mvp, w2c = camera(N, rng)
    c = dict(s, name=name, bones=bones, mvp=mvp, w2c=w2c, feat=None, patch=None, g=None)
    if s["feat"]:
        c["feat"] = _f32(rng.normal(size=(N, s["D"])))
        c["patch"] = _f32(rng.normal(size=(N, s["C"], s["h"], s["w"])))
        width = {"global": s["D"], "sample": s["C"], "sample+global": s["D"] + s["C"]}[s["mode"]]
        c["g"] = _f32(rng.normal(size=(N, K, width)))
    return c


def finite_twin(c):
    """A hand case with the three bones of non-finite coordinate moved to (5, 5), far outside the image: the same defined result there
    (no sample, no scatter) from finite numbers.  torch's CPU grid_sample returns NaN at a non-finite coordinate, so the torch
    statement's figures for the hand cases are measured on this twin; every element that has a magnitude is the same in both."""
    bones = c["bones"].clone()
    bones[0, list(NON_FINITE_BONES)] = torch.tensor([5.0, 5.0, 1.0])
    return dict(c, bones=bones)


# ---------------------------------------------------------------------------------------------------------------- limits
def _l(N, K, kind, **cfg):
    return dict(N=N, K=K, kind=kind, cfg=cfg)


_PONY = dict(num_body_bones=8, num_legs=4, num_leg_bones=3, output_multiplier=0.1, max_arti_angle=60)
_FAUNA = dict(_PONY, static_root_bones=False, iter_leg_rotation_start=300000, reg_body_rotate_mult=0.1)
LIMIT_CASES = {
    "k1_n1_plain": _l(1, 1, "base", num_body_bones=1, num_legs=0, num_leg_bones=0, output_multiplier=1.0, max_arti_angle=60),
    "k8_n3_bird": _l(3, 8, "base", num_body_bones=8, num_legs=0, num_leg_bones=0, output_multiplier=0.1, max_arti_angle=45, static_root_bones=True),
    "k20_n3_magicpony": _l(3, 20, "base", **_PONY, constrain_legs=True),
    "k20_n1_ponymation": _l(1, 20, "base", **_PONY, constrain_legs=True, extra_constraints=True),
    "k20_n3_fauna_constraints": _l(3, 20, "base", **dict(_PONY, output_multiplier=1.0), constrain_legs=True, use_fauna_constraints=True, static_root_bones=True),
    "k20_n1201_fauna_late": _l(1201, 20, "fauna", **_FAUNA, total_iter=300001, forbid_leg_rotate=True, small_leg_angle=True),
    "k20_n3_fauna_early": _l(3, 20, "fauna", **dict(_FAUNA, static_root_bones=True, output_multiplier=1.0), total_iter=10, forbid_leg_rotate=True, small_leg_angle=False),
}
SPECIAL_X = (0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 200.0, -200.0)


def build_limits(name):
    """dict(x [N,K,3], g_angles [N,K,3], g_reg 0-dim, kind, cfg).  x: normal(0, 3) with the special values 0, +-1e-30, +-20 and +-200
    (a saturated tanh) strewn in; no infinity (x = +-inf at a zero factor is the one documented difference: tested on its own)."""
    s = LIMIT_CASES[name]
    rng = np.random.default_rng(9500 + sorted(LIMIT_CASES).index(name))
    x = rng.normal(0.0, 3.0, (s["N"], s["K"], 3)) / s["cfg"]["output_multiplier"]
    flat = x.reshape(-1)
    where = rng.permutation(flat.size)[: max(flat.size // 3, 1)]
    flat[where] = np.array(SPECIAL_X)[np.arange(where.size) % len(SPECIAL_X)] / s["cfg"]["output_multiplier"]
    return dict(s, name=name, x=_f32(x), g_angles=_f32(rng.normal(size=x.shape)), g_reg=_f32(rng.normal(size=())))


# ---------------------------------------------------------------------------------------------------------------- golden rows
GOLDEN_LIMITS = {
    "magicpony": ("base", dict(_PONY, constrain_legs=True)),
    "ponymation": ("base", dict(_PONY, constrain_legs=True, extra_constraints=True)),
    "bird": ("base", dict(num_body_bones=8, num_legs=0, num_leg_bones=0, output_multiplier=0.1, max_arti_angle=45, static_root_bones=True)),
    "fauna_constraints": ("base", dict(_PONY, constrain_legs=True, use_fauna_constraints=True)),
}
for _it, _tag in ((100, "early"), (300001, "late")):
    for _forbid in (False, True):
        for _small in (False, True):
            GOLDEN_LIMITS[f"fauna_{_tag}_forbid{int(_forbid)}_small{int(_small)}"] = (
                "fauna", dict(_FAUNA, total_iter=_it, forbid_leg_rotate=_forbid, small_leg_angle=_small))


def golden_limits_x(name):
    """[2,2,K,3] float32: the network's raw output of a golden limits row."""
    kind, cfg = GOLDEN_LIMITS[name]
    K = cfg["num_body_bones"] + cfg["num_legs"] * cfg["num_leg_bones"]
    rng = np.random.default_rng(9700 + sorted(GOLDEN_LIMITS).index(name))
    return _f32(rng.normal(0.0, 12.0, (2, 2, K, 3)))


GOLDEN_BONES = {f"{pred}_{mode}_{'shared' if shared else 'batched'}": dict(pred=pred, mode=mode, shared=shared)
                for pred, mode, shared in (("base", "global", True), ("base", "sample", False), ("base", "sample+global", True),
                                           ("base", "sample+global", False), ("fauna", "sample+global", False), ("fauna", "sample", True),
                                           ("refine", "sample+global", False))}
GOLDEN_N, GOLDEN_K, GOLDEN_C, GOLDEN_D, GOLDEN_HW = 3, 5, 7, 4, (3, 5)


def golden_bones_inputs(name):
    """dict(bones [1|3,5,2,3], mvp, w2c, feat [3,4], patch [3,7,3,5], mode) of a golden descriptor row."""
    s = GOLDEN_BONES[name]
    rng = np.random.default_rng(9800 + sorted(GOLDEN_BONES).index(name))
    bones = _f32(rng.uniform(-0.6, 0.6, (1 if s["shared"] else GOLDEN_N, GOLDEN_K, 2, 3)))
    mvp, w2c = camera(GOLDEN_N, rng)
    return dict(s, bones=bones, mvp=mvp, w2c=w2c, feat=_f32(rng.normal(size=(GOLDEN_N, GOLDEN_D))),
                patch=_f32(rng.normal(size=(GOLDEN_N, GOLDEN_C, *GOLDEN_HW))))
