"""The articulation glue of the posing path: what the reference's predictors compute between ``estimate_bones`` and ``skinning`` besides
the articulation network itself.

``bone_inputs``: the per-bone descriptors -- InstancePredictorBase.get_bones / get_bones_from_articulation
(model/predictors/InstancePredictorBase.py:337-382, 391-432) and the Fauna twin (InstancePredictorFauna.py:102-147) from the bones on.
``constrain_angles``: the angle limits -- apply_articulation_constraints (InstancePredictorBase.py:435-511; Fauna :149-213 with the tanh at
:229-230) and, with ``return_reg``, arti_reg_loss = mean(angles^2) (AnimalModel.py:313-314).  ``limits_base`` / ``limits_fauna`` restate
the reference's rules from its own argument names as an ``ArticulationLimits``: one multiplier and one [K,3] table.

CUDA tensors take the HIP kernels (csrc/articulation.hip through ops.bone_inputs / ops.constrain_angles: one launch forward, one
backward, no memset, no atomics, the same bits on every run) while ``DEVICE`` is True; CPU tensors, ``DEVICE = False`` and the sizes the
kernels refuse take the torch statements ``_bone_inputs_torch`` / ``_constrain_angles_torch``, which restate the reference operation by
operation (its in-place ``*=`` taken as a plain multiply).  Both public functions are functional: they never write into an argument.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

__all__ = ["bone_inputs", "constrain_angles", "ArticulationLimits", "limits_base", "limits_fauna", "FEATURE_MODES", "CHUNK", "DEVICE"]

DEVICE = True  # CUDA tensors take the HIP kernels (False: the torch statements everywhere)
CHUNK = _lib.ARTICULATION_CHUNK  # feature columns per work-group of the descriptor kernels (A3D_ARTICULATION_CHUNK of csrc/articulation.h)
FEATURE_MODES = ("global", "sample", "sample+global")


def _ops():
    from . import ops

    return ops


# ---------------------------------------------------------------------------------------------------------------- descriptors
def _bone_inputs_torch(bones, mvp, w2c, cam_pos_z_offset, spatial_scale, feat=None, patch_feat=None, feature_mode="sample+global"):
    """InstancePredictorBase.py:338-382 statement by statement, for bones [N|1,K,2,3] and N = len(mvp) images."""
    n_images = mvp.shape[0]
    bones_pos = bones
    if n_images > bones_pos.shape[0]:
        bones_pos = bones_pos.repeat(n_images, 1, 1, 1)
    num_bones = bones_pos.shape[1]
    bones_mid_pos = bones_pos.mean(2)
    bones_mid_pos_world4 = torch.cat([bones_mid_pos, torch.ones_like(bones_mid_pos[..., :1])], -1)
    bones_mid_pos_clip4 = bones_mid_pos_world4 @ mvp.transpose(-1, -2)
    bones_mid_pos_2d = bones_mid_pos_clip4[..., :2] / bones_mid_pos_clip4[..., 3:4]
    bones_mid_pos_2d = bones_mid_pos_2d.detach()

    bones_pos_world4 = torch.cat([bones_pos, torch.ones_like(bones_pos[..., :1])], -1)
    bones_pos_cam4 = bones_pos_world4 @ w2c[:, None].transpose(-1, -2)
    bones_pos_cam3 = bones_pos_cam4[..., :3] / bones_pos_cam4[..., 3:4]
    bones_pos_cam3 = bones_pos_cam3 + torch.tensor([0, 0, cam_pos_z_offset], dtype=torch.float32).to(bones_pos_cam3.device).view(1, 1, 1, 3)
    bones_pos_3d = bones_pos_cam3.view(n_images, num_bones, 2 * 3) / spatial_scale * 2

    bones_idx = torch.arange(num_bones).to(bones_pos.device)
    bones_idx_in = ((bones_idx[None, :, None] + 0.5) / num_bones * 2 - 1).repeat(n_images, 1, 1)
    bones_pos_in = torch.cat([bones_mid_pos_2d, bones_pos_3d, bones_idx_in], -1)
    bones_pos_in = bones_pos_in.detach()

    if feat is not None and patch_feat is not None:
        global_feat = feat[:, None].repeat(1, num_bones, 1)
        local_feat = F.grid_sample(patch_feat, bones_mid_pos_2d.view(n_images, 1, -1, 2).to(patch_feat.dtype), mode="bilinear", padding_mode="zeros",
                                   align_corners=False).squeeze(dim=-2).permute(0, 2, 1)
        if feature_mode == "global":
            bones_feat = global_feat
        elif feature_mode == "sample":
            bones_feat = local_feat
        elif feature_mode == "sample+global":
            bones_feat = torch.cat([global_feat, local_feat], -1)
        else:
            raise NotImplementedError
    else:
        bones_feat = None
    return bones_feat, bones_pos_in


def _is_float(t, dims, last):
    return torch.is_tensor(t) and t.is_floating_point() and t.dim() == dims and tuple(t.shape[dims - len(last):]) == tuple(last)


def bone_inputs(bones, mvp, w2c, cam_pos_z_offset, spatial_scale, feat=None, patch_feat=None, feature_mode="sample+global"):
    """The inputs of the articulation network -> ``(bones_feat | None, bones_pos_in)``.

    bones [N,K,2,3], or [1,K,2,3]: the canonical skeleton, shared by the N images without being repeated; a leading [B,F] pair
    ([B,F,K,2,3], ``aux["posed_bones"]`` of ``skinning``) is flattened.  mvp, w2c [N,4,4].

    ``bones_pos_in`` [N,K,9] float32, never requires grad (the reference detaches it): columns 0-1 ``clip.xy / clip.w`` of the bone's
    midpoint ``(a + b) / 2`` under mvp; 2-7, per end point, ``(cam.xyz / cam.w + (0, 0, cam_pos_z_offset)) / spatial_scale * 2`` under
    w2c; 8 ``(k + 0.5) / K * 2 - 1``.

    ``bones_feat``: None when ``feat`` [N,D] or ``patch_feat`` [N,C,h,w] is None (as in the reference); else [N,K,D] ("global"),
    [N,K,C] ("sample") or [N,K,D+C] ("sample+global"): ``feat[n]`` first, then ``F.grid_sample(patch_feat, xy, mode="bilinear",
    padding_mode="zeros", align_corners=False)`` at columns 0-1 of bones_pos_in -- pixel coordinate ``((x + 1) * w - 1) / 2``, a tap
    outside the image contributes nothing.  ``patch_feat`` may have any strides (the encoder's permuted NHWC patch_out, its NCHW
    patch_key): it is never copied to be made contiguous.

    Gradients: to feat the sum over k of the global columns, to patch_feat the bilinear weights scattered back (with patch_feat's
    strides when it is dense in some order, else contiguous); to bones, mvp, w2c None.

    Edge behaviour: a midpoint whose projected coordinate is not finite (a NaN, an infinity, w = 0) samples 0 and scatters nothing,
    while bones_pos_in carries the non-finite value as torch would; a finite coordinate of any size is classified inside or outside
    the image in floating point before any conversion to an integer, so 1e30 is "outside", not undefined behaviour.

    Malformed arguments raise ValueError; sizes the kernels refuse (K > 64, h or w > 4096, more than 65535 images, a count of 2^31) take
    the torch statement."""
    if feature_mode not in FEATURE_MODES:
        raise ValueError(f"bone_inputs: feature_mode {feature_mode!r} is none of {FEATURE_MODES}")
    if torch.is_tensor(bones) and bones.dim() == 5:
        bones = bones.reshape(-1, *bones.shape[2:])
    if not _is_float(bones, 4, (2, 3)) or not _is_float(mvp, 3, (4, 4)) or not _is_float(w2c, 3, (4, 4)):
        raise ValueError("bone_inputs: expected float bones [N|1,K,2,3] (or [B,F,K,2,3]), mvp [N,4,4] and w2c [N,4,4], got "
                         + ", ".join(str(list(getattr(t, "shape", [type(t).__name__]))) for t in (bones, mvp, w2c)))
    N, K = int(mvp.shape[0]), int(bones.shape[1])
    if N < 1 or K < 1 or w2c.shape[0] != N or bones.shape[0] not in (1, N):
        raise ValueError(f"bone_inputs: bones {list(bones.shape)}, mvp {list(mvp.shape)} and w2c {list(w2c.shape)} do not belong together")
    if feat is not None and (not _is_float(feat, 2, ()) or feat.shape[0] != N or feat.shape[1] < 1):
        raise ValueError(f"bone_inputs: expected a float feat [{N},D], got {list(getattr(feat, 'shape', [type(feat).__name__]))}")
    if patch_feat is not None and (not _is_float(patch_feat, 4, ()) or patch_feat.shape[0] != N or min(patch_feat.shape[1:]) < 1):
        raise ValueError(f"bone_inputs: expected a float patch_feat [{N},C,h,w], got {list(getattr(patch_feat, 'shape', [type(patch_feat).__name__]))}")
    if not (math.isfinite(float(cam_pos_z_offset)) and math.isfinite(float(spatial_scale)) and float(spatial_scale) != 0.0):
        raise ValueError(f"bone_inputs: cam_pos_z_offset {cam_pos_z_offset} / spatial_scale {spatial_scale} must be finite, the scale not 0")
    if feat is None or patch_feat is None:
        use_feat = use_patch = None
    else:
        use_feat = feat if "global" in feature_mode else None
        use_patch = patch_feat if "sample" in feature_mode else None
    if DEVICE and mvp.is_cuda:
        D = 0 if use_feat is None else int(use_feat.shape[1])
        C, h, w = (0, 1, 1) if use_patch is None else (int(v) for v in use_patch.shape[1:])
        if _ops().bone_inputs_limits_ok(N, K, D, C, h, w):
            return _ops().bone_inputs(bones, mvp, w2c, cam_pos_z_offset, spatial_scale, use_feat, use_patch)
    return _bone_inputs_torch(bones, mvp, w2c, cam_pos_z_offset, spatial_scale, feat, patch_feat, feature_mode)


# ---------------------------------------------------------------------------------------------------------------- limits
# A limits program is the reference's statements after ``articulation_angles *= output_multiplier`` as data, in its order:
#   ("tanh",)                        a = a.tanh()
#   ("mul", c) / ("div", c)          a = a * c / a = a / c (the trailing ``* max_arti_angle / 180 * np.pi``)
#   ("mask", fill, sets, c)          tmp_mask = full_like(a, fill); tmp_mask[:, bones, axis] = value for (bones, axis, value) in sets (axis
#                                    None: every axis); then a = a * tmp_mask when c is None, else tmp_mask * (a * c) + (1 - tmp_mask) * a
def _mask(fill, sets, c=None):
    return ("mask", float(fill), tuple((tuple(int(b) for b in bones), axis, float(v)) for bones, axis, v in sets), c)


def _mask_table(step, K, like=None):
    """The step's tmp_mask: numpy float64 [K,3] (``like`` None), or a tensor like ``like`` [...,K,3] written through fancy indexing as
    the reference writes it.  An index past K raises IndexError."""
    _, fill, sets, _ = step
    table = np.full((K, 3), fill, dtype=np.float64) if like is None else torch.full_like(like, fill)
    for bones, axis, value in sets:
        if len(bones) == 0:
            continue
        if axis is None:
            table[..., list(bones), :] = value
        else:
            table[..., list(bones), axis] = value
    return table


def _fold(program, K):
    """The program as one factor per (bone, axis), in float64.  Exact in exact arithmetic: mask * (a * c) + (1 - mask) * a is a * c or a
    for a 0/1 mask, a mask-multiply before the tanh is 0/1 and tanh(0) = 0, and the trailing scalars multiply."""
    S = np.ones((K, 3), dtype=np.float64)
    seen_tanh = False
    for step in program:
        if step[0] == "tanh":
            seen_tanh = True
        elif step[0] == "mul":
            S = S * step[1]
        elif step[0] == "div":
            S = S / step[1]
        else:
            mask, c = _mask_table(step, K), step[3]
            assert seen_tanh or (c is None and np.isin(mask, (0.0, 1.0)).all()), "only a 0/1 mask commutes with the tanh"
            S = S * mask if c is None else mask * (S * c) + (1.0 - mask) * S
    assert seen_tanh
    return S


class ArticulationLimits:
    """``angles = scale[k,c] * tanh(multiplier * x)``: a multiplier and a [K,3] table.  ``scale`` is taken in float64, rounded to float32
    ONCE and cached per device.  ``program`` (the builders set it) is the reference's pass-by-pass form of the same limits, which the
    torch statement executes; without one the torch statement is the formula above."""

    def __init__(self, multiplier, scale, program=None):
        s = np.array(scale, dtype=np.float64)
        if s.ndim != 2 or s.shape[1] != 3 or s.shape[0] < 1 or not np.isfinite(s).all() or not math.isfinite(float(multiplier)):
            raise ValueError(f"ArticulationLimits: expected a finite multiplier and a finite scale [K,3], got {multiplier} and {list(s.shape)}")
        self.multiplier = float(multiplier)
        self.scale64 = s
        self.scale = torch.from_numpy(s.astype(np.float32))
        self.program = program
        self._on = {}

    @property
    def num_bones(self):
        return int(self.scale.shape[0])

    def scale_on(self, device):
        device = torch.device(device)
        if device.type == "cpu":
            return self.scale
        if device not in self._on:
            self._on[device] = self.scale.to(device)
        return self._on[device]


def _limits(program, K, multiplier, who):
    if K < 1:
        raise ValueError(f"{who}: the skeleton has no bones")
    try:
        return ArticulationLimits(multiplier, _fold(program, K), tuple(program))
    except IndexError as e:
        raise ValueError(f"{who}: the reference's bone lists index past the K = {K} bones of this skeleton ({e})") from None


def _leg_passes(num_body_bones, num_legs, num_leg_bones):
    legs = list(range(num_body_bones, num_body_bones + num_leg_bones * num_legs))
    return [_mask(0, [(legs, 2, 1)], 0.3), _mask(0, [(legs, 1, 1)], 0.3)]  # twist (z), then side bending (y)


def limits_base(num_body_bones, num_legs, num_leg_bones, output_multiplier, max_arti_angle, static_root_bones=False, constrain_legs=False,
                use_fauna_constraints=False, extra_constraints=False):
    """InstancePredictorBase.apply_articulation_constraints (:435-511) for a skeleton of num_body_bones + num_legs * num_leg_bones bones.
    Raises ValueError where the reference's hard-coded bone lists ([10,13,16,19], [8,9,11,...], [0..7], [8,11,14,17], [9,10,12,...])
    would index past K."""
    nb, K = int(num_body_bones), int(num_body_bones) + int(num_legs) * int(num_leg_bones)
    program = []
    if static_root_bones:
        program.append(_mask(1, [([nb // 2 - 1, nb - 1], None, 0)]))
    program.append(("tanh",))
    if constrain_legs:
        program += _leg_passes(nb, int(num_legs), int(num_leg_bones))
        if use_fauna_constraints:
            top, bottom = [10, 13, 16, 19], [8, 9, 11, 12, 14, 15, 17, 18]
            program.append(_mask(0, [(top, 1, 1), (top, 2, 1)], 0.05))
            program.append(_mask(0, [(top, 0, 1)], 0.75))
            program.append(_mask(1, [(bottom, 1, 0), (bottom, 2, 0), (bottom, 0, 0.3)]))
            program.append(_mask(0, [(list(range(8)), 2, 1)], 0.1))
    if extra_constraints:
        half = int(num_leg_bones) * int(num_legs) // 2
        legs = [nb + i for i in range(half)] + [nb + half + i for i in range(half)]
        top, bottom = [8, 11, 14, 17], [9, 10, 12, 13, 15, 16, 18, 19]
        program.append(_mask(0, [(legs, 2, 1)], 0.3))
        program.append(_mask(0, [(legs, 1, 1)], 0.3))
        program.append(_mask(0, [(top, 1, 1), (top, 2, 1)], 0.05))
        program.append(_mask(1, [(bottom, 1, 0), (bottom, 2, 0)]))
    program += [("mul", float(max_arti_angle)), ("div", 180), ("mul", np.pi)]
    return _limits(program, K, output_multiplier, "limits_base")


def limits_fauna(num_body_bones, num_legs, num_leg_bones, output_multiplier, max_arti_angle, static_root_bones, total_iter,
                 iter_leg_rotation_start, forbid_leg_rotate, small_leg_angle, reg_body_rotate_mult):
    """The Fauna predictor at iteration ``total_iter``: the tanh of forward_articulation (InstancePredictorFauna.py:229-230), then
    apply_articulation_constraints (:187-213) and apply_fauna_articulation_regularizer (:149-185).  The table changes when total_iter
    passes iter_leg_rotation_start: build one ArticulationLimits for either side and keep both.  Raises ValueError where the
    reference's bone lists ([0..7] always, [8,11,14,17] and [9,10,12,...] after the switch) would index past K."""
    nb, K = int(num_body_bones), int(num_body_bones) + int(num_legs) * int(num_leg_bones)
    program = [("tanh",)]
    if static_root_bones:
        program.append(_mask(1, [([nb // 2 - 1, nb - 1], None, 0)]))
    if total_iter <= iter_leg_rotation_start:
        program += _leg_passes(nb, int(num_legs), int(num_leg_bones))
    if iter_leg_rotation_start > 0 and total_iter > iter_leg_rotation_start and forbid_leg_rotate:
        if small_leg_angle:
            top = [8, 11, 14, 17]
            program.append(_mask(0, [(top, 1, 1), (top, 2, 1)], 0.05))
        bottom = [9, 10, 12, 13, 15, 16, 18, 19]
        program.append(_mask(1, [(bottom, 1, 0), (bottom, 2, 0)]))
    program += [("mul", float(max_arti_angle)), ("div", 180), ("mul", np.pi)]
    body_rotate_mult = reg_body_rotate_mult * 180 * 1.0 / (max_arti_angle * np.pi)
    program.append(_mask(0, [(list(range(8)), 2, 1)], body_rotate_mult))
    return _limits(program, K, output_multiplier, "limits_fauna")


def _constrain_angles_torch(x, limits, return_reg=False):
    """The reference's passes one by one on x [...,K,3] (each allocates its mask and writes it through fancy indexing, as there)."""
    a = x * limits.multiplier
    if limits.program is None:
        a = a.tanh() * limits.scale_on(x.device).to(x.dtype)
    else:
        for step in limits.program:
            if step[0] == "tanh":
                a = a.tanh()
            elif step[0] == "mul":
                a = a * step[1]
            elif step[0] == "div":
                a = a / step[1]
            else:
                tmp_mask, c = _mask_table(step, limits.num_bones, like=a), step[3]
                a = a * tmp_mask if c is None else tmp_mask * (a * c) + (1 - tmp_mask) * a
    return (a, (a ** 2).mean()) if return_reg else a


def constrain_angles(x, limits, return_reg=False):
    """``angles = S[k,c] * tanh(m * x)`` for the network's raw output x [N,K,3] (or [B,F,K,3]: the same shape comes back) and an
    ``ArticulationLimits(multiplier=m, scale=S)``; with ``return_reg`` also ``reg = mean(angles ** 2)``, a 0-dim float32 tensor
    (arti_reg_loss), differentiable through the same backward kernel.

    Every pass of the reference is a multiplication by a constant per (bone, axis), so its up to nine mask passes, static_root_bones and
    the trailing ``* max_arti_angle / 180 * pi`` fold into S (``limits_base`` / ``limits_fauna``).  One documented difference:
    ``x = +-inf`` at a bone whose factor is 0 gives 0 here and NaN in the reference (0 * inf before its tanh, or inf * 0 in a blend).

    Malformed arguments raise ValueError; N * K * 3 > 2^20 or K > 64 take the torch statement."""
    if not isinstance(limits, ArticulationLimits):
        raise ValueError(f"constrain_angles: expected an ArticulationLimits, got {type(limits).__name__}")
    if not torch.is_tensor(x) or not x.is_floating_point() or x.dim() not in (3, 4) or x.shape[-1] != 3 or x.shape[-2] != limits.num_bones:
        raise ValueError(f"constrain_angles: expected a float x [N,{limits.num_bones},3] or [B,F,{limits.num_bones},3], got "
                         f"{getattr(x, 'dtype', type(x).__name__)} {list(getattr(x, 'shape', []))}")
    K = limits.num_bones
    if DEVICE and x.is_cuda and x.numel() >= 1 and K <= _lib.ARTICULATION_MAX_BONES and x.numel() <= _lib.ARTICULATION_MAX_ANGLES:
        out = _ops().constrain_angles(x.reshape(-1, K, 3), limits.scale_on(x.device), limits.multiplier, return_reg)
        return (out[0].reshape(x.shape), out[1]) if return_reg else out.reshape(x.shape)
    return _constrain_angles_torch(x, limits, return_reg)
