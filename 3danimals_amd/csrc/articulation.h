/* liba3d_hip: the articulation glue of the posing path -- per-bone descriptors (the reference's get_bones / get_bones_from_articulation
 * arithmetic) and the angle limits (apply_articulation_constraints with arti_reg_loss); DESIGN.md section 36.  An INTERNAL header: these
 * entry points serve the package's own articulation.py / ops.py, are registered in _lib.INTERNAL_SURFACES and are no part of the public
 * surface under include/ (126 entry points, a3d_version() 405: both unchanged).  Same conventions as include/a3d.h: flat C, device
 * pointers + sizes + a3d_stream_t, int status with the message in a3d_last_error(), arguments validated before anything is launched, no
 * allocation and no synchronisation inside a call.  Every call is ONE launch, without memset and without atomics: the same bits on every
 * run. */
#ifndef A3D_ARTICULATION_H
#define A3D_ARTICULATION_H

#include "../../include/a3d.h"

/* feature columns one work-group of the descriptor kernels owns (mirrored as _lib.ARTICULATION_CHUNK); a power of two up to 256.
 * Whole calls were timed at 16, 32 and 64: a library built with another -DA3D_ARTICULATION_CHUNK
 * is for that measurement only. */
#ifndef A3D_ARTICULATION_CHUNK
#define A3D_ARTICULATION_CHUNK 32
#endif
#define A3D_ARTICULATION_MAX_BONES 64
#define A3D_ARTICULATION_MAX_SIDE 4096
/* most elements (N * K * 3) the one work-group of the limits kernels strides over */
#define A3D_ARTICULATION_MAX_ANGLES 1048576
/* most images of one call: the descriptor kernels take the image from the grid's y */
#define A3D_ARTICULATION_MAX_IMAGES 65535

#ifdef __cplusplus
extern "C" {
#endif

/* bones [N,K,2,3] (bones_shared != 0: [1,K,2,3], read by every image), mvp and w2c [N,4,4], all contiguous float32.
 *   pos_in [N,K,9]:  0-1  clip.xy / clip.w of the midpoint (a + b) / 2 under mvp;  2-7  per end point (cam.xyz / cam.w + (0, 0, z_offset))
 *                    / spatial_scale * 2 under w2c;  8  (k + 0.5) / K * 2 - 1.
 *   bones_feat [N,K,D+C]: feat[n] [D] in the first D columns of every bone, then the bilinear sample (zero padding, align_corners false:
 *                    pixel = ((x + 1) * w - 1) / 2) of patch [N,C,h,w] with the element strides sn, sc, sh, sw at columns 0-1 of pos_in.
 * D == 0: no global columns (feat may be NULL); C == 0: no sampled columns (patch may be NULL); both 0: bones_feat may be NULL.
 * A coordinate that is not finite samples 0; a finite one of any size is classified inside / outside in floating point.
 * Limits: 1 <= K <= 64, 1 <= h, w <= 4096 when C > 0, strides >= 0, N <= 65535, N * K * (D + C), N * K * 9 and N * max(D, C) below 2^31.
 * N == 0 is no work. */
int a3d_bone_inputs_fwd(const float* bones, int bones_shared, const float* mvp, const float* w2c, float cam_pos_z_offset, float spatial_scale,
                        const float* feat, const float* patch, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int N, int K, int D, int C,
                        int h, int w, float* bones_feat, float* pos_in, a3d_stream_t stream);

/* The adjoint of the feature columns: g_bones_feat [N,K,D+C] and the pos_in the forward returned ->
 *   g_feat  [N,D]      sum over k of the global columns, k ascending (NULL: not wanted);
 *   g_patch [N,C,h,w]  with the element strides gn, gc, gh, gw (>= 1, non-overlapping), EVERY element written: the work-group of (image,
 *                      chunk of channels) zero-fills its slab and then adds the taps bone by bone, k ascending, taps in the order
 *                      (y0,x0) (y0,x1) (y1,x0) (y1,x1) (NULL: not wanted).
 * Same limits as the forward, and N * C * h * w below 2^31. */
int a3d_bone_inputs_bwd(const float* g_bones_feat, const float* pos_in, int N, int K, int D, int C, int h, int w, float* g_feat, float* g_patch,
                        int64_t gn, int64_t gc, int64_t gh, int64_t gw, a3d_stream_t stream);

/* angles [N,K,3] = S[k,c] * tanh(multiplier * x), and unless reg is NULL reg[0] = mean(angles^2).  S [K,3] float32.  One work-group.
 * Limits: 1 <= K <= 64, N * K * 3 <= 2^20.  N == 0 is no work. */
int a3d_constrain_angles_fwd(const float* x, const float* S, float multiplier, int N, int K, float* angles, float* reg, a3d_stream_t stream);

/* g_x = (g_angles + g_reg[0] * 2 angles / (N K 3)) * S * multiplier * (1 - tanh^2), tanh recomputed from x (S may be 0); g_angles or g_reg
 * may be NULL (that gradient is absent), not both. */
int a3d_constrain_angles_bwd(const float* g_angles, const float* g_reg, const float* x, const float* S, float multiplier, int N, int K,
                             float* g_x, a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
