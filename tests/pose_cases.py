"""Seeded inputs of the camera-pose glue (3danimals_amd/pose.py): the smallest shapes at which each mechanism can go wrong, shared by
tests/golden/make_golden_pose.py, tests/test_pose_cpu.py and tests/test_pose_gpu.py.

A condition, not a tolerance: outside the exact-tie cases (total_iter <= naive_probs_iter, where every blended probability is exactly
1 / H and the pick is hypothesis 0) this module asserts, in float64 and on import, that the best blended probability of every row leads
the second best by at least 1e-3 of itself, so a float32 evaluation cannot pick another hypothesis."""
import zlib

import numpy as np
import torch

Z_OFFSET, FOV = 10.0, 25.0
NAIVE_ITER, BEST_ITER = 2000, 6000
MAX_TRANS = (0.44, 0.44, 1.1)
MARGIN = 1e-3
FLOAT_OUTPUTS = ("poses_raw", "pose_raw", "pose", "mvp", "w2c", "campos", "rot_prob", "rot_logit", "rots_probs")
HAND_VALUES = (-200.0, -60.0, 0.0, 14.4, 14.5, 80.0)  # softplus switches to the identity between 14.4 and 14.5 (beta x = 20)


def orthant_signs(H):
    """The reference's tables (InstancePredictorBase.py:171, 175): the four xz quadrants, or the eight octants in meshgrid order (an
    INTEGER tensor there)."""
    if H == 4:
        return torch.tensor([[1, 1, 1], [-1, 1, 1], [-1, 1, -1], [1, 1, -1]], dtype=torch.float32)
    assert H == 8
    return torch.tensor([[x, y, z] for x in (1, -1) for y in (1, -1) for z in (1, -1)], dtype=torch.int64)


def _case(N, H, total_iter, random_sample=True, oct=False, zeroy=False, temp_clip_max=100.0, offset_extra=None, grads=FLOAT_OUTPUTS, hand=False):
    return dict(N=N, H=H, total_iter=total_iter, random_sample=random_sample, oct=oct, zeroy=zeroy, temp_clip_max=temp_clip_max,
                offset_extra=offset_extra, grads=tuple(grads), hand=hand)


# name -> spec.  total_iter 0: the uniform blend, exact ties; 2500: blend weight 0.75; 7000: p = 0.5; 200000: temperature 1/100 (1/10 with
# Fauna's clip), p = 0.8.  N = 5 with p = 0.8 is the boundary case: the value 4 of the permutation sits on 4 / 5 < 0.8 in float32.
FUSED_CASES = {
    "n1_h4_it0_rand": _case(1, 4, 0),
    "n3_h4_it0_norand_only_probs": _case(3, 4, 0, random_sample=False, grads=("rot_prob", "rots_probs")),
    "n3_h4_it2500_rand": _case(3, 4, 2500),
    "n3_h4_it7000_rand": _case(3, 4, 7000),
    "n3_h4_zeroy_it7000_rand_only_campos": _case(3, 4, 7000, zeroy=True, grads=("campos",)),
    "n3_h4_it200000_norand": _case(3, 4, 200000, random_sample=False),
    "n5_h4_it200000_rand_boundary": _case(5, 4, 200000),
    "n5_h4_zeroy_it200000_rand_fauna": _case(5, 4, 200000, zeroy=True, temp_clip_max=10.0),
    "n5_h8_oct_it7000_rand": _case(5, 8, 7000, oct=True),
    "n5_h8_oct_zeroy_it200000_rand": _case(5, 8, 200000, oct=True, zeroy=True),
    "n5_h8_oct_it2500_norand_only_poses_raw": _case(5, 8, 2500, oct=True, random_sample=False, grads=("poses_raw",)),
    "n65_h4_it2500_rand": _case(65, 4, 2500),
    "n257_h4_it7000_rand_extra": _case(257, 4, 7000, offset_extra=1.5),
    "n65_h8_oct_it200000_rand_only_mvp_logit": _case(65, 8, 200000, oct=True, grads=("mvp", "rot_logit")),
    "hand_h4_it200000_norand": _case(8, 4, 200000, random_sample=False, hand=True),
    "hand_h4_it7000_rand": _case(8, 4, 7000, hand=True),
}
NON_FINITE = "non_finite_h4_it7000_rand"  # forward only, against the torch statement's places
TIE_CASES = tuple(n for n, c in FUSED_CASES.items() if c["total_iter"] <= NAIVE_ITER)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _hand_raw(rng, N, H):
    """Every vector entry out of HAND_VALUES; rows 0 and 1 hold the all-underflow vector (-200, 0, -200) in EVERY hypothesis, so the
    picked one normalises to 0 whatever is picked; logits with one clear minimum per row, +-3e4 among them."""
    raw = np.zeros((N, 4 * H + 3))
    vec = rng.choice(HAND_VALUES, size=(N, H, 3))
    vec[0:2] = (-200.0, 0.0, -200.0)
    vec[2, :, :] = (14.4, 14.5, 80.0)
    vec[3, :, :] = (14.5, -60.0, 14.4)
    vec[4, :, :] = (-60.0, 0.0, -60.0)
    logits = rng.permutation(np.array([-3e4, 3e4, 0.0, 1.0]))[None].repeat(N, 0)
    for n in range(N):
        logits[n] = np.roll(logits[n], n)
    logits[5] = (0.5, -0.25, 2.0, 1.0)
    raw[:, :4 * H] = np.concatenate([logits[..., None], vec], -1).reshape(N, 4 * H)
    raw[:, -3:] = rng.choice(HAND_VALUES, size=(N, 3)) / 40.0
    raw[6, -3:] = (80.0, -200.0, 0.0)  # a saturated tanh
    return raw


def blended(raw, H, total_iter, temp_clip_max, rot_temp_scalar=1.0):
    """rots_probs in float64 (numpy), as the reference's lines state it."""
    logits = np.asarray(raw, dtype=np.float64)[:, :4 * H].reshape(-1, H, 4)[..., 0]
    temp = 1 / np.clip(total_iter / 1000 / rot_temp_scalar, 1., temp_clip_max)
    z = -logits / temp
    e = np.exp(z - z.max(1, keepdims=True))
    w = np.clip(1 - (total_iter - NAIVE_ITER) / 2000, 0, 1)
    return (1.0 / H) * w + e / e.sum(1, keepdims=True) * (1 - w)


def build_fused(name):
    """raw, the two permutations (None without random sampling), one upstream gradient per float output, and the keyword arguments."""
    c = dict(FUSED_CASES[name]) if name != NON_FINITE else _case(6, 4, 7000)
    rng = _rng(name)
    N, H = c["N"], c["H"]
    if c["hand"]:
        raw = _hand_raw(rng, N, H)
    else:
        raw = rng.normal(0.0, 1.0, (N, 4 * H + 3))
        raw[:, 0:4 * H:4] = rng.uniform(0.0, 3.0, (N, H))  # the logits (a reconstruction loss per hypothesis: positive)
    if name == NON_FINITE:
        raw[0, 1:4 * H:4] = np.inf  # x of every hypothesis: inf / inf in the normalisation of whichever is picked
        raw[1, 4] = np.nan  # one logit: the whole softmax row
        raw[2, 4 * H] = np.nan  # the translation
        raw[3, 2:4 * H:4] = np.nan  # y of every hypothesis
        raw[4, 3:4 * H:4], raw[4, 0], raw[4, 4 * H + 1] = -np.inf, np.inf, -np.inf  # softplus, exp and tanh of an infinity are finite
    c["raw"] = _f32(raw)
    c["signs"], c["max_trans"] = orthant_signs(H), torch.tensor(MAX_TRANS, dtype=torch.float32)
    if c["random_sample"]:
        c["rand_perm"], c["best_perm"] = torch.from_numpy(rng.permutation(N)), torch.from_numpy(rng.permutation(N))
        if N == 5:  # the boundary: the image whose best_perm is 4 is hypothesis-picked at random only if 4 / 5 < 0.8 is False
            assert 4 in c["best_perm"].tolist()
    else:
        c["rand_perm"] = c["best_perm"] = None
    shapes = dict(poses_raw=(N, 4 * H + 3), pose_raw=(N, 6), pose=(N, 12), mvp=(N, 4, 4), w2c=(N, 4, 4), campos=(N, 3), rot_prob=(N,),
                  rot_logit=(N,), rots_probs=(N, H))
    c["g"] = {k: _f32(rng.normal(0.0, 1.0, shapes[k])) for k in FLOAT_OUTPUTS}
    c["name"] = name
    return c


def fused_kwargs(c):
    return dict(orthant_signs=c["signs"], max_trans_xyz_range=c["max_trans"], cam_pos_z_offset=Z_OFFSET, fov=FOV, oct=c["oct"],
                lookat_zeroy=c["zeroy"], rot_temp_scalar=1.0, num_hypos=c["H"], naive_probs_iter=NAIVE_ITER, best_pose_start_iter=BEST_ITER,
                random_sample=c["random_sample"], temp_clip_max=c["temp_clip_max"], rand_perm=c["rand_perm"], best_perm=c["best_perm"],
                offset_extra=c["offset_extra"])


# cameras_from_pose alone: rotations that are NOT orthonormal (any 3x3), with and without offset_extra
CAMERA_CASES = {"n1": dict(N=1, offset_extra=None), "n3_extra": dict(N=3, offset_extra=0.75), "n257": dict(N=257, offset_extra=None)}


def build_cameras(name):
    c = dict(CAMERA_CASES[name])
    rng = _rng("cameras/" + name)
    c["pose"] = _f32(np.concatenate([rng.normal(0.0, 1.0, (c["N"], 9)), rng.uniform(-0.5, 0.5, (c["N"], 3))], -1))
    c["g"] = dict(mvp=_f32(rng.normal(size=(c["N"], 4, 4))), w2c=_f32(rng.normal(size=(c["N"], 4, 4))), campos=_f32(rng.normal(size=(c["N"], 3))))
    return c


# random views: rand_degree 0, 90, 359 and a repeated value; bins = 360 and bins = 7; w2c_pred has more images than rand_degree
RANDOM_VIEW_CASES = {"bins360": dict(bins=360, degree=(0, 90, 359, 90, 1)), "bins7": dict(bins=7, degree=(0, 6, 3, 3, 90, 359)),
                     "bins360_n257": dict(bins=360, degree=tuple(int(v) for v in np.random.default_rng(7).integers(0, 360, 257)))}


def build_random_view(name):
    c = dict(RANDOM_VIEW_CASES[name])
    rng = _rng("random_view/" + name)
    b = len(c["degree"])
    w2c = rng.normal(0.0, 1.0, (b + 2, 4, 4))
    w2c[:, :3, 3] = rng.uniform(-1.0, 1.0, (b + 2, 3)) + (0, 0, -Z_OFFSET)
    c["w2c_pred"], c["rand_degree"] = _f32(w2c), torch.tensor(c["degree"], dtype=torch.int64)
    return c


def _assert_margins():
    for name, spec in FUSED_CASES.items():
        if name in TIE_CASES:
            continue
        c = build_fused(name)
        q = np.sort(blended(c["raw"].numpy(), c["H"], c["total_iter"], c["temp_clip_max"]), 1)
        lead = (q[:, -1] - q[:, -2]) / q[:, -1]
        assert (lead >= MARGIN).all(), (name, float(lead.min()))


_assert_margins()
