/* liba3d_hip: shading BSDFs and the HDR image loss (the second public header of the library; the core surface is a3d.h).
 *
 * Same conventions as a3d.h: flat C, device pointers + sizes + a3d_stream_t, int status (A3D_OK / A3D_EINVAL / A3D_EHIP) with the
 * message in a3d_last_error(), arguments validated before anything is launched, no allocation and no synchronisation inside a call.
 * The entry points live in the same liba3d_hip.so; they do not change a3d_version().
 *
 * Element-wise work over the "pixels" of a broadcast result.  The result has `ndim` leading dimensions shape[0 .. ndim) (outermost
 * first; the caller merges neighbouring dimensions where every input allows it) and, per pixel, 1 or 3 channels.  Every input is a base
 * pointer plus one ELEMENT stride per leading dimension -- 0 where the input is broadcast along it -- plus a channel stride; nothing
 * is expanded in memory.  Outputs and gradients are written contiguously.
 *
 * Gradients of an input (g_mode):
 *   A3D_BSDF_GRAD_NONE    not wanted.
 *   A3D_BSDF_GRAD_DIRECT  g_in[i] is [pixels, channels]: one row per pixel of the result.
 *   A3D_BSDF_GRAD_REDUCE  the input is constant over runs of seg * seg_div[i] consecutive pixels (e.g. a [B,1,1,3] camera position:
 *                         seg * seg_div = H W); its gradient is the sum over each run: g_final[i] is [pixels / (seg * seg_div[i]),
 *                         channels].  The pixels are cut into segments of `seg` (which divides the pixel count), every work-group
 *                         covers A3D_BSDF_TILE pixels of one segment, sums its lanes' contributions in registers, in the wave and
 *                         across the work-group in LDS, and stores ONE partial row to g_in[i], which the caller provides as
 *                         [a3d_bsdf_rows(desc), channels] DOUBLES (8-byte aligned; the sums are carried in double up to the
 *                         final float); a finishing launch of the same call adds the rows of each run in a
 *                         fixed order.  No float atomics: two calls on the same inputs give the same bits.
 */
#ifndef A3D_BSDF_H
#define A3D_BSDF_H

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define A3D_BSDF_MAX_INPUTS 6
#define A3D_BSDF_MAX_DIMS 4
#define A3D_BSDF_TILE 1024 /* pixels per work-group */

/* op codes; inputs in the reference's argument order; channels per input / of the result */
#define A3D_BSDF_LAMBERT 0      /* nrm, wi                               3 3         -> 1  (renderutils/ops.py:244-264, bsdf.py:57-58)   */
#define A3D_BSDF_FROSTBITE 1    /* nrm, wi, wo, linearRoughness          3 3 3 1     -> 1  (ops.py:278-300, bsdf.py:64-79)               */
#define A3D_BSDF_PBR_SPECULAR 2 /* col, nrm, wo, wi, alpha               3 3 3 3 1   -> 3  (ops.py:315-339, bsdf.py:117-134)             */
#define A3D_BSDF_PBR 3          /* kd, arm, pos, nrm, view_pos, light_pos 3 x 6      -> 3  (ops.py:355-386, bsdf.py:136-151)             */
#define A3D_BSDF_IMAGE_LOSS 4   /* img, target                           1 1         -> scalar (ops.py:476-498, loss.py:16-41)           */

#define A3D_BSDF_GRAD_NONE 0
#define A3D_BSDF_GRAD_DIRECT 1
#define A3D_BSDF_GRAD_REDUCE 2

/* image loss codes (variant of A3D_BSDF_IMAGE_LOSS is loss + 4 * tonemap) */
#define A3D_LOSS_L1 0
#define A3D_LOSS_MSE 1
#define A3D_LOSS_SMAPE 2
#define A3D_LOSS_RELMSE 3
#define A3D_TONEMAP_NONE 0
#define A3D_TONEMAP_LOG_SRGB 1

typedef struct a3d_bsdf_desc {
    uint32_t size;          /* sizeof(a3d_bsdf_desc) of the caller's header: a shorter struct is refused */
    int32_t op;             /* A3D_BSDF_* */
    int32_t variant;        /* A3D_BSDF_PBR: diffuse lobe, 0 lambert / 1 frostbite; A3D_BSDF_IMAGE_LOSS: loss + 4 * tonemap; else 0 */
    float min_roughness;    /* A3D_BSDF_PBR_SPECULAR, A3D_BSDF_PBR: alpha is clamped to [min_roughness^2, 1] */
    int32_t ndim;           /* 1 .. A3D_BSDF_MAX_DIMS */
    int32_t reserved;       /* 0 */
    int64_t shape[4];       /* leading shape of the result; pixels = their product */
    int64_t seg;            /* pixels per segment, divides pixels (pixels itself when no gradient is reduced) */
    const float* in[6];     /* inputs (unused slots NULL) */
    int64_t stride[24];     /* stride[4 * i + d]: element stride of input i along leading dimension d, 0 = broadcast */
    int64_t cstride[6];     /* element stride between the channels of input i */
    float* out;             /* forward: [pixels, channels]; image loss forward: the scalar (the mean) */
    float* scratch;         /* image loss forward: [a3d_bsdf_rows(desc)] DOUBLES of partial sums (8-byte aligned) */
    const float* g_out;     /* backward: [pixels, channels], contiguous; image loss backward: the scalar's gradient (one float) */
    int32_t g_mode[6];      /* A3D_BSDF_GRAD_* per input */
    int64_t seg_div[6];     /* A3D_BSDF_GRAD_REDUCE: segments per run of input i (>= 1) */
    float* g_in[6];         /* DIRECT: the gradient; REDUCE: the partial rows (doubles) */
    float* g_final[6];      /* REDUCE: the gradient */
} a3d_bsdf_desc;

/* Work-groups of a launch over this descriptor = partial rows of a reduced gradient / floats of the image loss scratch:
 * (pixels / seg) * ceil(seg / A3D_BSDF_TILE); -1 for an invalid descriptor.  Touches no pointer. */
int64_t a3d_bsdf_rows(const a3d_bsdf_desc* desc);

/* lambert, frostbite_diffuse, pbr_specular, pbr_bsdf (reference renderutils/ops.py:244-386): one launch each way.
 * fwd reads in[], writes out.  bwd reads in[] and g_out, recomputes the forward's intermediates and writes every wanted gradient from
 * the same launch (plus one finishing launch when any gradient is reduced).  A backward that reduces a gradient carries its per-pixel
 * arithmetic in double (the few numbers of such a gradient then carry the rounding of the float32 inputs only); otherwise float. */
int a3d_bsdf_fwd(const a3d_bsdf_desc* desc, a3d_stream_t stream);
int a3d_bsdf_bwd(const a3d_bsdf_desc* desc, a3d_stream_t stream);

/* image_loss (reference renderutils/ops.py:476-498): op = A3D_BSDF_IMAGE_LOSS, one channel, every element a pixel.
 * fwd: partial sums (double) to scratch, then out[0] = (sum in a fixed order) / pixels.  bwd: element-wise, g_in = g_out[0] / pixels * d loss. */
int a3d_image_loss_fwd(const a3d_bsdf_desc* desc, a3d_stream_t stream);
int a3d_image_loss_bwd(const a3d_bsdf_desc* desc, a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
