/* liba3d_hip: the camera-pose glue of the predictors -- the heads of the pose network's output, the pick of one hypothesis with its
 * look-at rotation, the cameras of a pose, and Fauna's random-view cameras (the reference's forward_pose,
 * sample_pose_hypothesis_from_quad_predictions, get_camera_extrinsics_from_pose and get_random_view_mask arithmetic); DESIGN.md section
 * 37.  An INTERNAL header: these entry points serve the package's own pose.py / ops.py, are registered in _lib.INTERNAL_SURFACES and are no
 * part of the public surface under include/ (126 entry points, a3d_version() 405: both unchanged).  Same conventions as include/a3d.h:
 * flat C, device pointers + sizes + a3d_stream_t, int status with the message in a3d_last_error(), arguments validated before anything
 * is launched, no allocation and no synchronisation inside a call.  Every call is ONE launch of one thread per image, without memset
 * and without atomics: the same bits on every run.  ``proj`` is always a HOST pointer to the 16 floats of the row-major projection: it
 * is read during the call and travels in the kernel's arguments. */
#ifndef A3D_POSE_H
#define A3D_POSE_H

#include "../../include/a3d.h"

#define A3D_POSE_MAX_HYPOS 8
#define A3D_POSE_MAX_IMAGES 65535

#ifdef __cplusplus
extern "C" {
#endif

/* raw [N,4H+3] (per hypothesis: logit, forward x y z; then the translation), orthant_signs [H,3], max_trans [3], all contiguous float32
 * on the device; rand_perm, best_perm [N] int64 on the device, both NULL for "no random sampling".
 *   poses_raw [N,4H+3]  logit; normalize((softplus(x), y', softplus(z)) * signs[h]) with y' = softplus(y) when oct, y' * 0 when zeroy,
 *                       softplus of beta = ln 2 / 0.5 returning x itself where beta * x > 20, normalize dividing by max(norm, 1e-12);
 *                       tanh(t) * max_trans.
 *   rots_probs [N,H]    (1 / H) * naive_weight + softmax(-logit / temp) * one_minus_weight, the softmax minus its row maximum.
 *   rot_idx [N] int64   best = argmax of rots_probs (the first NaN, else the lowest index among equal maxima); with permutations
 *                       best where best_perm[n] < best_below, else rand_perm[n] % H.  rand_flag [N] int64: 1 where the latter.
 *   rot_prob, rot_logit [N]: rots_probs and the logit at rot_idx.  pose_raw [N,6]: the picked forward vector, the translation.
 *   pose [N,12]         rows right = normalize((0,1,0) x f), up = normalize(f x right), f; then the translation.
 *   mvp, w2c [N,4,4], campos [N,3]: as a3d_cameras_from_pose_fwd of pose.
 * Limits: 1 <= H <= 8, 1 <= N <= 65535. */
int a3d_pose_cameras_fwd(const float* raw, const float* orthant_signs, const float* max_trans, const int64_t* rand_perm, const int64_t* best_perm,
                         int N, int H, int oct, int zeroy, float temp, float naive_weight, float one_minus_weight, int64_t best_below,
                         float offset_z, const float* proj, float* poses_raw, float* pose_raw, float* pose, float* mvp, float* w2c, float* campos,
                         int64_t* rot_idx, float* rot_prob, float* rot_logit, float* rots_probs, int64_t* rand_flag, a3d_stream_t stream);

/* The adjoint: the gradients arriving through every differentiable output (each may be NULL: absent) -> g_raw [N,4H+3], EVERY element
 * written; everything else is recomputed from raw and the two permutations.  The forward columns of a hypothesis that was not picked
 * receive gradient through g_poses_raw only; an element nothing feeds is exactly 0. */
int a3d_pose_cameras_bwd(const float* raw, const float* orthant_signs, const float* max_trans, const int64_t* rand_perm, const int64_t* best_perm,
                         int N, int H, int oct, int zeroy, float temp, float naive_weight, float one_minus_weight, int64_t best_below,
                         float offset_z, const float* proj, const float* g_poses_raw, const float* g_pose_raw, const float* g_pose,
                         const float* g_mvp, const float* g_w2c, const float* g_campos, const float* g_rot_prob, const float* g_rot_logit,
                         const float* g_rots_probs, float* g_raw, a3d_stream_t stream);

/* pose [N,12] (a row-major 3x3 R, then t) -> w2c = [[R^T, t + (0, 0, offset_z)], [0, 0, 0, 1]], mvp = proj @ w2c (all four terms of
 * every dot product, so a non-finite element spreads as in a matrix product), campos = -R (t + (0, 0, offset_z)).  1 <= N <= 65535. */
int a3d_cameras_from_pose_fwd(const float* pose, int N, float offset_z, const float* proj, float* mvp, float* w2c, float* campos,
                              a3d_stream_t stream);

/* g_mvp, g_w2c [N,4,4], g_campos [N,3] (each may be NULL, not all) -> g_pose [N,12], every element written. */
int a3d_cameras_from_pose_bwd(const float* pose, int N, float offset_z, const float* proj, const float* g_mvp, const float* g_w2c,
                              const float* g_campos, float* g_pose, a3d_stream_t stream);

/* Fauna's random-view cameras for b images: w2c_pred [>= b,4,4] float32 and rand_degree [b] int64 on the device.  angle = delta_angle *
 * (float)rand_degree, its cosine and sine taken in double and rounded to float32; Ry = [[c,0,s,0],[0,1,0,0],[-s,0,c,0],[0,0,0,1]];
 * w2c = the identity with w2c_pred's translation, mvp = (proj @ w2c) @ Ry, campos = Ry[:3,:3]^T (-translation).  1 <= b <= 65535. */
int a3d_random_view_cameras(const float* w2c_pred, const int64_t* rand_degree, int b, float delta_angle, const float* proj, float* mvp, float* w2c,
                            float* campos, a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
