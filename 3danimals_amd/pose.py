"""The camera-pose glue of the predictors: what the reference computes between its pose network and the first mesh operation (DESIGN.md
section 37).

``pose_heads``: forward_pose after ``self.netPose(...)`` for the quadlookat / octlookat representations
(model/predictors/InstancePredictorBase.py:257-304).  ``pick_hypothesis``: sample_pose_hypothesis_from_quad_predictions (:623-663; the
Fauna twin InstancePredictorFauna.py:37-77 is ``temp_clip_max=10.``) with lookat_forward_to_rot_matrix (:706-714).
``cameras_from_pose``: get_camera_extrinsics_from_pose (:606-620).  ``random_view_cameras``: the cameras of Fauna's get_random_view_mask
(model/models/Fauna.py:112-142).  ``predict_cameras``: the first three back to back, as InstancePredictorBase.forward (:671-678) and
InstancePredictorMotionVAE.generate (:178-185) run them.

CUDA tensors take the HIP kernels (csrc/pose.hip through ops.predict_cameras / ops.cameras_from_pose / ops.random_view_cameras: one
launch forward, at most one backward, no memset, no atomics, the same bits on every run) while ``DEVICE`` is True; CPU tensors,
``DEVICE = False`` and the sizes the kernels refuse take the torch statements, which restate the reference operation by operation.
``pose_heads`` and ``pick_hypothesis`` on their own are torch statements on every device: ``predict_cameras`` is their HIP route.
Every public function is functional: it never writes into an argument.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .model.render import util

__all__ = ["pose_heads", "pick_hypothesis", "cameras_from_pose", "random_view_cameras", "predict_cameras", "lookat_forward_to_rot_matrix",
           "best_below", "DEVICE"]

DEVICE = True  # CUDA tensors take the HIP kernels (False: the torch statements everywhere)
AUX_KEYS = ("rot_idx", "rot_prob", "rot_logit", "rots_probs", "rand_pose_flag")


def _ops():
    from . import ops

    return ops


# ---------------------------------------------------------------------------------------------------------------- torch statements
def _pose_heads_torch(pose, orthant_signs, max_trans_xyz_range, oct=False, lookat_zeroy=False):
    """InstancePredictorBase.py:257-304 statement by statement (branch quadlookat / octlookat) on the network's output ``pose``."""
    num_pose_hypos = orthant_signs.shape[0]
    trans_pred = pose[..., -3:].tanh() * max_trans_xyz_range.to(pose.device)

    rots_pred = pose[..., :num_pose_hypos * 4].view(-1, num_pose_hypos, 4)
    rots_logits = rots_pred[..., :1]
    vec_forward = rots_pred[..., 1:4]

    def softplus_with_init(x, init=0.5):
        beta = np.log(2) / init
        return F.softplus(x, beta=beta)

    xs, ys, zs = vec_forward.unbind(-1)
    xs = softplus_with_init(xs, init=0.5)
    if oct:
        ys = softplus_with_init(ys, init=0.5)
    if lookat_zeroy:
        ys = ys * 0
    zs = softplus_with_init(zs, init=0.5)
    vec_forward = torch.stack([xs, ys, zs], -1)
    vec_forward = vec_forward * orthant_signs.to(pose.device)
    vec_forward = F.normalize(vec_forward, p=2, dim=-1)
    rot_pred = torch.cat([rots_logits, vec_forward], -1).view(-1, num_pose_hypos * 4)
    return torch.cat([rot_pred, trans_pred], -1)


def lookat_forward_to_rot_matrix(vec_forward, up=(0, 1, 0)):
    """InstancePredictorBase.py:706-714: rows right, up, forward; two cross products and two normalisations."""
    up = torch.tensor(list(up), dtype=torch.float32).to(vec_forward.device).to(vec_forward.dtype)
    vec_right = up.expand_as(vec_forward).cross(vec_forward, dim=-1)
    vec_right = F.normalize(vec_right, p=2, dim=-1)
    vec_up = vec_forward.cross(vec_right, dim=-1)
    vec_up = F.normalize(vec_up, p=2, dim=-1)
    return torch.stack([vec_right, vec_up, vec_forward], -2)


def _schedule(total_iter, rot_temp_scalar, naive_probs_iter, best_pose_start_iter, temp_clip_max):
    """The three host scalars of the pick, as the reference evaluates them (:632, :637, :643): temp, naive_probs_weight, p.  Its
    ``np.clip(x, lo, hi)`` of a finite Python scalar is ``min(max(x, lo), hi)``: the same double, without numpy's scalar dispatch."""
    clip = lambda x, lo, hi: min(max(x, lo), hi)
    temp = 1 / clip(total_iter / 1000 / rot_temp_scalar, 1., temp_clip_max)
    naive_probs_weight = clip(1 - (total_iter - naive_probs_iter) / 2000, 0, 1)
    p = clip((total_iter - best_pose_start_iter) / 2000, 0, 0.8)
    return float(temp), float(naive_probs_weight), float(p)


@functools.lru_cache(maxsize=64)
def best_below(N, p):
    """How many of the values 0..N-1 satisfy ``value / N < p`` as torch evaluates it: a float32 quotient against p rounded to float32.
    The quotient is monotone in the value, so ``perm / N < p`` is ``perm < best_below(N, p)``."""
    q = np.arange(N, dtype=np.int64).astype(np.float32) / np.float32(N)
    return int(np.count_nonzero(q < np.float32(p)))


def _pick_hypothesis_torch(poses_raw, total_iter, rot_temp_scalar, num_hypos, naive_probs_iter, best_pose_start_iter, random_sample,
                           temp_clip_max, rand_perm, best_perm):
    """InstancePredictorBase.py:627-663 statement by statement; the two permutations are inputs."""
    rots_pred = poses_raw[..., :num_hypos * 4].view(-1, num_hypos, 4)
    N = len(rots_pred)
    rots_logits = rots_pred[..., 0]
    rots_pred = rots_pred[..., 1:4]
    trans_pred = poses_raw[..., -3:]
    temp, naive_probs_weight, p = _schedule(total_iter, rot_temp_scalar, naive_probs_iter, best_pose_start_iter, temp_clip_max)

    rots_probs = F.softmax(-rots_logits / temp, dim=1)
    naive_probs = torch.ones(num_hypos).to(rots_logits.device)
    naive_probs = naive_probs / naive_probs.sum()
    rots_probs = naive_probs.view(1, num_hypos) * naive_probs_weight + rots_probs * (1 - naive_probs_weight)
    best_rot_idx = torch.argmax(rots_probs, dim=1)

    if random_sample:
        rand_rot_idx = rand_perm % num_hypos
        best_flag = (best_perm / N < p).long()
        rand_flag = 1 - best_flag
        rot_idx = best_rot_idx * best_flag + rand_rot_idx * (1 - best_flag)
    else:
        rand_flag = torch.zeros_like(best_rot_idx)
        rot_idx = best_rot_idx
    rot_pred = torch.gather(rots_pred, 1, rot_idx[:, None, None].expand(-1, 1, 3))[:, 0]
    pose_raw = torch.cat([rot_pred, trans_pred], -1)
    rot_prob = torch.gather(rots_probs, 1, rot_idx[:, None].expand(-1, 1))[:, 0]
    rot_logit = torch.gather(rots_logits, 1, rot_idx[:, None].expand(-1, 1))[:, 0]

    rot_mat = lookat_forward_to_rot_matrix(rot_pred, up=[0, 1, 0])
    pose = torch.cat([rot_mat.view(N, -1), pose_raw[:, 3:]], -1)
    pose_aux = {"rot_idx": rot_idx, "rot_prob": rot_prob, "rot_logit": rot_logit, "rots_probs": rots_probs, "rand_pose_flag": rand_flag}
    return pose_raw, pose, pose_aux


def _offset_z(cam_pos_z_offset, offset_extra):
    return -cam_pos_z_offset - offset_extra if offset_extra is not None else -cam_pos_z_offset


def _cameras_from_pose_torch(pose, cam_pos_z_offset, fov, znear=0.1, zfar=1000., offset_extra=None):
    """InstancePredictorBase.py:607-620 statement by statement."""
    N = len(pose)
    pose_R = pose[:, :9].view(N, 3, 3).transpose(2, 1)
    cam_pos_offset = torch.tensor([0, 0, _offset_z(cam_pos_z_offset, offset_extra)], dtype=torch.float32).to(pose.device).to(pose.dtype)
    pose_T = pose[:, -3:] + cam_pos_offset[None, None, :]
    pose_T = pose_T.view(N, 3, 1)
    pose_RT = torch.cat([pose_R, pose_T], axis=2)
    w2c = torch.cat([pose_RT, torch.tensor([0, 0, 0, 1], dtype=torch.float32).repeat(N, 1, 1).to(pose.device).to(pose.dtype)], axis=1)
    proj = util.perspective(fov / 180 * np.pi, 1, znear, zfar)[None].to(pose.device).to(pose.dtype)
    mvp = torch.matmul(proj, w2c)
    campos = -torch.matmul(pose_R.transpose(2, 1), pose_T).view(N, 3)
    return mvp, w2c, campos


def _random_view_cameras_torch(w2c_pred, rand_degree, fov, bins=360):
    """Fauna.py:112-142 statement by statement: the loop over the batch with its ``.item()`` and its 4x4 host tensor per image."""
    device = w2c_pred.device
    delta_angle = 2 * np.pi / bins
    b = len(rand_degree)
    delta_angle = delta_angle * rand_degree.cpu()
    delta_rot_matrix = []
    for i in range(b):
        angle = delta_angle[i].item()
        angle_matrix = torch.FloatTensor([
            [np.cos(angle), 0, np.sin(angle), 0],
            [0, 1, 0, 0],
            [-np.sin(angle), 0, np.cos(angle), 0],
            [0, 0, 0, 1],
        ]).to(device)
        delta_rot_matrix.append(angle_matrix)
    delta_rot_matrix = torch.stack(delta_rot_matrix, dim=0)

    w2c = torch.FloatTensor(np.diag([1., 1., 1., 1]))
    w2c = w2c.repeat(b, 1, 1).to(device)  # (its 1.4 * cam_pos_z_offset translation is overwritten by the next statement)
    w2c_pred = w2c_pred.detach()
    w2c[:, :3, 3] = w2c_pred[:b][:, :3, 3]

    proj = util.perspective(fov / 180 * np.pi, 1, n=0.1, f=1000.0).repeat(b, 1, 1).to(device)
    mvp = torch.bmm(proj, w2c)
    campos = -w2c[:, :3, 3]
    mvp = torch.matmul(mvp, delta_rot_matrix)
    campos = torch.matmul(delta_rot_matrix[:, :3, :3].transpose(2, 1), campos[:, :, None])[:, :, 0]
    return mvp, w2c, campos


# ---------------------------------------------------------------------------------------------------------------- arguments
def _shape(t):
    return list(getattr(t, "shape", [type(t).__name__]))


def _is_float(t, dims):
    return torch.is_tensor(t) and t.is_floating_point() and t.dim() == dims


def _finite(*values):
    try:
        return all(math.isfinite(float(v)) for v in values)
    except (TypeError, ValueError):
        return False


def _as_table(v, shape_tail, device, who, name):
    """orthant_signs / max_trans_xyz_range: a tensor on any device or a nested sequence -> a float tensor where it is (not moved)."""
    try:
        t = v if torch.is_tensor(v) else torch.tensor(np.asarray(v, dtype=np.float32))
    except (TypeError, ValueError):
        t = None
    if t is not None and not t.is_floating_point() and not t.is_complex() and t.dtype != torch.bool:
        t = t.float()  # (the reference's octant table is an integer tensor)
    if t is None or not t.is_floating_point() or t.dim() != len(shape_tail) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape_tail)):
        raise ValueError(f"{who}: expected a float {name} {[s if s is not None else 'H' for s in shape_tail]}, got {_shape(v)}")
    return t


def _check_heads(raw, orthant_signs, max_trans_xyz_range, who):
    if not _is_float(raw, 2) or raw.shape[0] < 1:
        raise ValueError(f"{who}: expected a float raw [N,4H+3] with N >= 1, got {getattr(raw, 'dtype', '')} {_shape(raw)}")
    signs = _as_table(orthant_signs, (None, 3), raw.device, who, "orthant_signs")
    trans = _as_table(max_trans_xyz_range, (3,), raw.device, who, "max_trans_xyz_range")
    H = int(signs.shape[0])
    if H < 1 or raw.shape[1] != 4 * H + 3:
        raise ValueError(f"{who}: raw {_shape(raw)} does not hold the 4 * {H} + 3 columns of {H} hypotheses")
    return signs, trans, H


def _check_pick(N, width, total_iter, rot_temp_scalar, num_hypos, naive_probs_iter, best_pose_start_iter, temp_clip_max, random_sample, rand_perm,
                best_perm, who):
    if not isinstance(num_hypos, (int, np.integer)) or num_hypos < 1 or width != 4 * num_hypos + 3:
        raise ValueError(f"{who}: {width} columns are not the 4 * num_hypos + 3 of num_hypos = {num_hypos}")
    if not _finite(total_iter, rot_temp_scalar, naive_probs_iter, best_pose_start_iter, temp_clip_max) or float(rot_temp_scalar) <= 0 \
            or float(temp_clip_max) < 1 or float(total_iter) < 0:
        raise ValueError(f"{who}: total_iter {total_iter}, rot_temp_scalar {rot_temp_scalar}, naive_probs_iter {naive_probs_iter}, "
                         f"best_pose_start_iter {best_pose_start_iter}, temp_clip_max {temp_clip_max}: expected finite numbers, "
                         "total_iter >= 0, rot_temp_scalar > 0, temp_clip_max >= 1")
    for name, perm in (("rand_perm", rand_perm), ("best_perm", best_perm)):
        if perm is None:
            continue
        if not random_sample:
            raise ValueError(f"{who}: {name} given without random_sample")
        if not torch.is_tensor(perm) or perm.dtype != torch.int64 or tuple(perm.shape) != (N,):
            raise ValueError(f"{who}: expected an int64 {name} [{N}], got {getattr(perm, 'dtype', '')} {_shape(perm)}")


def _draw(N, device, random_sample, rand_perm, best_perm):
    """The reference's two draws in its order (:642 then :643) where a permutation is not given."""
    if not random_sample:
        return None, None
    if rand_perm is None:
        rand_perm = torch.randperm(N, device=device)
    if best_perm is None:
        best_perm = torch.randperm(N, device=device)
    return rand_perm.to(device), best_perm.to(device)


def _check_cameras(cam_pos_z_offset, fov, znear, zfar, offset_extra, who):
    extra = 0.0 if offset_extra is None else offset_extra
    if not _finite(cam_pos_z_offset, fov, znear, zfar, extra) or not 0 < float(fov) < 180 or float(znear) == float(zfar):
        raise ValueError(f"{who}: cam_pos_z_offset {cam_pos_z_offset}, fov {fov}, znear {znear}, zfar {zfar}, offset_extra {offset_extra}: "
                         "expected finite numbers, 0 < fov < 180, znear != zfar")


@functools.lru_cache(maxsize=16)
def _proj16(fov, znear, zfar):
    return tuple(float(v) for v in util.perspective(fov / 180 * np.pi, 1, znear, zfar).reshape(-1).tolist())


# ---------------------------------------------------------------------------------------------------------------- public functions
def pose_heads(raw, orthant_signs, max_trans_xyz_range, oct=False, lookat_zeroy=False):
    """The heads of the pose network's output raw [N,4H+3] -> ``poses_raw`` [N,4H+3]: per hypothesis (logit, forward vector), then the
    translation.  The logit passes through; the forward vector is ``F.normalize((softplus(x), y, softplus(z)) * orthant_signs[h])`` with
    y = softplus(y) when ``oct`` and y * 0 when ``lookat_zeroy``, softplus of beta = ln 2 / 0.5 (it returns x itself where
    beta * x > 20; F.normalize divides by max(norm, 1e-12)); the translation is ``tanh(t) * max_trans_xyz_range``.
    orthant_signs [H,3] and max_trans_xyz_range [3] are tensors on any device or sequences.

    A torch statement on every device (InstancePredictorBase.py:257-304 operation by operation); its HIP route is ``predict_cameras``.
    Malformed arguments raise ValueError."""
    signs, trans, _ = _check_heads(raw, orthant_signs, max_trans_xyz_range, "pose_heads")
    return _pose_heads_torch(raw, signs.to(raw.dtype), trans.to(raw.dtype), bool(oct), bool(lookat_zeroy))


def pick_hypothesis(poses_raw, total_iter, rot_temp_scalar=1., num_hypos=4, naive_probs_iter=2000, best_pose_start_iter=6000, random_sample=True,
                    temp_clip_max=100., rand_perm=None, best_perm=None):
    """One hypothesis per image out of poses_raw [N,4H+3] -> ``(pose_raw [N,6], pose [N,12], aux)``: the picked forward vector and the
    translation; the look-at rotation (rows right, up, forward; up = (0,1,0)) flattened, and the translation; aux with the reference's
    five entries rot_idx [N] int64, rot_prob [N], rot_logit [N], rots_probs [N,H], rand_pose_flag [N] int64.

    rots_probs = (1 / H) * w + softmax(-logit / temp) * (1 - w), temp = 1 / clip(total_iter / 1000 / rot_temp_scalar, 1,
    temp_clip_max) (``temp_clip_max=10.`` is the Fauna twin), w = clip(1 - (total_iter - naive_probs_iter) / 2000, 0, 1).  The best
    hypothesis is the argmax (the first NaN if there is one, else the lowest index among equal maxima).  With ``random_sample`` image n
    keeps its best one where ``best_perm[n] / N < clip((total_iter - best_pose_start_iter) / 2000, 0, 0.8)`` and takes
    ``rand_perm[n] % H`` elsewhere.  Permutations that are not given are drawn by ``torch.randperm(N, device=...)`` in the reference's
    order (rand_perm first), so a seeded run picks what the reference picks.

    A torch statement on every device (InstancePredictorBase.py:623-663 operation by operation); its HIP route is ``predict_cameras``.
    Malformed arguments raise ValueError."""
    if not _is_float(poses_raw, 2) or poses_raw.shape[0] < 1:
        raise ValueError(f"pick_hypothesis: expected a float poses_raw [N,4H+3] with N >= 1, got {getattr(poses_raw, 'dtype', '')} {_shape(poses_raw)}")
    N = int(poses_raw.shape[0])
    _check_pick(N, int(poses_raw.shape[1]), total_iter, rot_temp_scalar, num_hypos, naive_probs_iter, best_pose_start_iter, temp_clip_max,
                random_sample, rand_perm, best_perm, "pick_hypothesis")
    rand_perm, best_perm = _draw(N, poses_raw.device, random_sample, rand_perm, best_perm)
    return _pick_hypothesis_torch(poses_raw, total_iter, rot_temp_scalar, int(num_hypos), naive_probs_iter, best_pose_start_iter, bool(random_sample),
                                  temp_clip_max, rand_perm, best_perm)


def cameras_from_pose(pose, cam_pos_z_offset, fov, znear=0.1, zfar=1000., offset_extra=None):
    """pose [N,12] (a flattened 3x3 rotation R, rows right / up / forward, then a translation t) -> ``(mvp [N,4,4], w2c [N,4,4], campos
    [N,3])``: w2c = [[R^T, t + (0, 0, -cam_pos_z_offset - offset_extra)], [0, 0, 0, 1]], mvp = perspective(fov degrees, 1, znear, zfar)
    @ w2c, campos = -R (t + offset).  R need not be orthonormal (Ponymation's canonical pose, the visualisation scripts).

    CUDA tensors take csrc/pose.hip (one launch forward, one backward; the gradient goes to ``pose``).  Malformed arguments raise
    ValueError; more than 65535 images take the torch statement (InstancePredictorBase.py:606-620 operation by operation)."""
    if not _is_float(pose, 2) or pose.shape[0] < 1 or pose.shape[1] != 12:
        raise ValueError(f"cameras_from_pose: expected a float pose [N,12] with N >= 1, got {getattr(pose, 'dtype', '')} {_shape(pose)}")
    _check_cameras(cam_pos_z_offset, fov, znear, zfar, offset_extra, "cameras_from_pose")
    if DEVICE and pose.is_cuda and pose.shape[0] <= _lib.POSE_MAX_IMAGES:
        return _ops().cameras_from_pose(pose, _offset_z(cam_pos_z_offset, offset_extra), _proj16(fov, znear, zfar))
    return _cameras_from_pose_torch(pose, cam_pos_z_offset, fov, znear, zfar, offset_extra)


def random_view_cameras(w2c_pred, rand_degree, fov, bins=360):
    """The random-view cameras of Fauna's get_random_view_mask for the first b = len(rand_degree) images of w2c_pred [>= b,4,4] ->
    ``(mvp [b,4,4], w2c [b,4,4], campos [b,3])``: w2c is the identity with w2c_pred's translation, mvp = perspective(fov) @ w2c @ Ry,
    campos = Ry^T (-translation), Ry the rotation about y by the float32 product (2 pi / bins) * rand_degree, its cosine and sine taken
    in double and rounded to float32.  rand_degree is an integer tensor on any device; nothing carries a gradient.

    CUDA w2c_pred takes csrc/pose.hip (one launch, rand_degree read on the device: no ``.item()``, no host matrices).  Malformed
    arguments raise ValueError; more than 65535 images take the torch statement (Fauna.py:112-142 operation by operation)."""
    if not _is_float(w2c_pred, 3) or tuple(w2c_pred.shape[1:]) != (4, 4):
        raise ValueError(f"random_view_cameras: expected a float w2c_pred [N,4,4], got {getattr(w2c_pred, 'dtype', '')} {_shape(w2c_pred)}")
    if not torch.is_tensor(rand_degree) or rand_degree.is_floating_point() or rand_degree.is_complex() or rand_degree.dtype == torch.bool \
            or rand_degree.dim() != 1 or not 1 <= rand_degree.shape[0] <= w2c_pred.shape[0]:
        raise ValueError(f"random_view_cameras: expected an integer rand_degree [b] with 1 <= b <= {_shape(w2c_pred)[0]}, got "
                         f"{getattr(rand_degree, 'dtype', '')} {_shape(rand_degree)}")
    if not isinstance(bins, (int, np.integer)) or bins < 1 or not _finite(fov) or not 0 < float(fov) < 180:
        raise ValueError(f"random_view_cameras: bins {bins} / fov {fov}: expected an integer >= 1 and 0 < fov < 180")
    if DEVICE and w2c_pred.is_cuda and rand_degree.shape[0] <= _lib.POSE_MAX_IMAGES:
        return _ops().random_view_cameras(w2c_pred, rand_degree, float(np.float32(2 * np.pi / bins)), _proj16(fov, 0.1, 1000.0))
    return _random_view_cameras_torch(w2c_pred, rand_degree, fov, int(bins))


def predict_cameras(raw, total_iter, *, orthant_signs, max_trans_xyz_range, cam_pos_z_offset, fov, oct=False, lookat_zeroy=False, rot_temp_scalar=1.,
                    num_hypos=4, naive_probs_iter=2000, best_pose_start_iter=6000, random_sample=True, temp_clip_max=100., rand_perm=None,
                    best_perm=None, znear=0.1, zfar=1000., offset_extra=None):
    """``pose_heads``, ``pick_hypothesis`` and ``cameras_from_pose`` back to back on the pose network's output raw [N,4H+3] ->
    ``(poses_raw, pose_raw, pose, mvp, w2c, campos, aux)``; every keyword is that of the function it belongs to.

    CUDA tensors take ONE launch of csrc/pose.hip forward and one backward: the backward takes the gradients arriving through
    poses_raw, pose_raw, pose, mvp, w2c, campos, rot_prob, rot_logit and rots_probs and returns the gradient of raw, recomputed from
    raw and the two permutations.  The forward columns of a hypothesis that was not picked receive gradient only through poses_raw; an
    element nothing feeds is exactly 0.  H above 8 or more than 65535 images take the three torch statements chained.
    Malformed arguments raise ValueError."""
    signs, trans, H = _check_heads(raw, orthant_signs, max_trans_xyz_range, "predict_cameras")
    N = int(raw.shape[0])
    _check_pick(N, int(raw.shape[1]), total_iter, rot_temp_scalar, num_hypos, naive_probs_iter, best_pose_start_iter, temp_clip_max, random_sample,
                rand_perm, best_perm, "predict_cameras")
    if int(num_hypos) != H:
        raise ValueError(f"predict_cameras: num_hypos = {num_hypos} while orthant_signs has {H} rows")
    _check_cameras(cam_pos_z_offset, fov, znear, zfar, offset_extra, "predict_cameras")
    rand_perm, best_perm = _draw(N, raw.device, random_sample, rand_perm, best_perm)
    if DEVICE and raw.is_cuda and H <= _lib.POSE_MAX_HYPOS and N <= _lib.POSE_MAX_IMAGES:
        temp, weight, p = _schedule(total_iter, rot_temp_scalar, naive_probs_iter, best_pose_start_iter, temp_clip_max)
        out = _ops().predict_cameras(raw, _ops().pose_table(signs, raw.device), _ops().pose_table(trans, raw.device), rand_perm, best_perm,
                                     bool(oct), bool(lookat_zeroy), temp, weight, best_below(N, p) if random_sample else N,
                                     _offset_z(cam_pos_z_offset, offset_extra), _proj16(fov, znear, zfar))
        return out[:6] + (dict(zip(AUX_KEYS, out[6:])),)
    poses_raw = _pose_heads_torch(raw, signs.to(raw.dtype), trans.to(raw.dtype), bool(oct), bool(lookat_zeroy))
    pose_raw, pose, aux = _pick_hypothesis_torch(poses_raw, total_iter, rot_temp_scalar, H, naive_probs_iter, best_pose_start_iter,
                                                 bool(random_sample), temp_clip_max, rand_perm, best_perm)
    mvp, w2c, campos = _cameras_from_pose_torch(pose, cam_pos_z_offset, fov, znear, zfar, offset_extra)
    return poses_raw, pose_raw, pose, mvp, w2c, campos, aux
