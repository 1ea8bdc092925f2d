/* liba3d_hip: the output stage of the coordinate fields' MLPs (the ninth public header of the library; the core surface is a3d.h, the
 * BSDFs are a3d_bsdf.h, the image-space derivatives a3d_deriv.h, the tangent frame a3d_tangent.h, the mesh regularisers a3d_reg.h, the
 * environment-lit shade a3d_envshade.h, the SDF regulariser a3d_sdfreg.h, the distance transform a3d_edt.h).
 *
 * Same conventions as a3d.h: flat C, device pointers + sizes + a3d_stream_t, int status (A3D_OK / A3D_EINVAL / A3D_EHIP) with the
 * message in a3d_last_error(), arguments validated before anything is launched, no allocation and no synchronisation inside a call.
 * The entry points live in the same liba3d_hip.so; they do not change a3d_version().
 *
 * What the reference's MLP / CoordMLP (model/networks/MLPs.py:9-32, 73-98) run after the last hidden ReLU of a field over a long point
 * list, as one pass over the hidden vectors h [M,256] each way (fp32 throughout, v_mfma_f32_16x16x4_f32, fp32 accumulate):
 *     forward    s   = act(h . W^T)            W [C,256] is the Linear's [out,in] weight as stored, act: none or the sigmoid
 *                out = s * scale + lo          the min_max map with lo = min, scale = max - min (both NULL: no map)
 *     backward   ga       = g_out * scale * act'(s)                 the sigmoid's adjoint from its saved output, s (1 - s)
 *                g_h[m,k] = (sum_c ga[m,c] W[c,k]) * (h[m,k] > 0)   strictly positive, as threshold_backward(g, h, 0): a denormal is positive
 *                g_W[c,k] = sum_m ga[m,c] h[m,k]
 * h is the ReLU output of the last hidden layer, so the mask IS that layer's ReLU adjoint.  No float atomics: every work-group leaves
 * the sum over its own A3D_FIELD_HEAD_WG_ROWS rows in scratch and a second launch adds these partial sums in a fixed order -- the
 * same bits on every run.
 */
#ifndef A3D_FIELDS_H
#define A3D_FIELDS_H

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define A3D_FIELD_HEAD_WIDTH 256   /* columns of h */
#define A3D_FIELD_HEAD_MAX_C 16    /* most output channels */
#define A3D_FIELD_HEAD_WG_ROWS 512 /* rows of h one work-group of either kernel walks */
#define A3D_FIELD_HEAD_ACT_NONE 0
#define A3D_FIELD_HEAD_ACT_SIGMOID 1

/* bytes of scratch a3d_field_head_bwd needs: ceil(M / A3D_FIELD_HEAD_WG_ROWS) partial sums of [C,256] floats.  0 when the sizes are
 * outside the limits below. */
size_t a3d_field_head_scratch_bytes(int64_t M, int C);

/* One launch.  s [M,C] and out [M,C]; with neither an activation nor the map only out is written (s may be NULL).
 * Limits: 1 <= M < 2^31, 1 <= C <= A3D_FIELD_HEAD_MAX_C, act one of A3D_FIELD_HEAD_ACT_*; lo and scale both given or both NULL;
 * h and W 16-byte aligned. */
int a3d_field_head_fwd(const float* h, const float* W, const float* lo, const float* scale, int act, int64_t M, int C, float* s, float* out,
                       a3d_stream_t stream);

/* Two launches.  g_out [M,C], s [M,C] as the forward left it (read only when act is the sigmoid, NULL otherwise allowed), scale [C] or
 * NULL; g_h [M,256], g_W [C,256].  Same limits; h, W, g_h and scratch (a3d_field_head_scratch_bytes(M, C) bytes) 16-byte aligned. */
int a3d_field_head_bwd(const float* g_out, const float* s, const float* h, const float* W, const float* scale, int act, int64_t M, int C,
                       void* scratch, float* g_h, float* g_W, a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
