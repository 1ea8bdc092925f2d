/* liba3d_hip: the exact Euclidean distance transform of batched binary images (the eighth public header of the library; the core
 * surface is a3d.h, the BSDFs are a3d_bsdf.h, the image-space derivatives a3d_deriv.h, the tangent frame a3d_tangent.h, the mesh
 * regularisers a3d_reg.h, the environment-lit shade a3d_envshade.h, the SDF regulariser a3d_sdfreg.h).
 *
 * Same conventions as a3d.h: flat C, device pointers + sizes + a3d_stream_t, int status (A3D_OK / A3D_EINVAL / A3D_EHIP) with the
 * message in a3d_last_error(), arguments validated before anything is launched, no allocation and no synchronisation inside a call.
 * The entry points live in the same liba3d_hip.so; they do not change a3d_version().
 *
 * What the reference's compute_distance_transform (model/dataset/util.py:12-18) gets from two cv2.distanceTransform(..., DIST_L2,
 * DIST_MASK_PRECISE) calls per sample on the host, and what a3d_recon_losses_fwd reads as mask_dt.  The semantics are this library's
 * own specification (OpenCV documents DIST_MASK_PRECISE as the exact transform; this is that):
 *     an input is M images [M,H,W], each pixel either ZERO or NON-ZERO
 *     d2[p]   = min over the zero pixels q of p's image of (py - qy)^2 + (px - qx)^2, an integer; 0 where p itself is zero
 *     dist[p] = (float)(sqrt((double)d2[p]) / scale): one float64 root, one float64 divide, one rounding to float32
 *     idx[p]  = qy * W + qx of a nearest zero pixel; among equally near ones the smallest flat index (candidates ordered by
 *               (d2, qy, qx)); p's own flat index where p is zero
 *     an image WITHOUT a zero pixel: d2 = H * H + W * W everywhere (strictly above any attainable value), dist from that, idx = -1.
 *               Finite on purpose: an infinity times a zero weight would put a NaN into a loss.  (scipy's distance_transform_edt
 *               returns arbitrary values for such an image.)
 * All arithmetic is integer until the final store and there are no atomics: the same bits on every run.  No backward: the reference
 * never differentiates mask_dt.
 */
#ifndef A3D_EDT_H
#define A3D_EDT_H

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* largest side of an image: d2 < 2^26 then, and (d2, qy, qx) packs into 26 + 12 + 12 bits of a 64-bit key */
#define A3D_EDT_MAX_SIDE 4096

/* how the source is read (src_kind):
 *   A3D_EDT_SRC_U8   uint8 [M,H,W]; non-zero is != 0; one channel per image.
 *   A3D_EDT_SRC_F32  float32 mask [N,H,W] with M = 2 N; BOTH channels of the reference come out of one read of the mask, laid out
 *                    [N,2,H,W]: channel 0 is non-zero where m >= t_in (the distance INSIDE the mask to the background), channel 1 is
 *                    non-zero where m <= t_out (the distance OUTSIDE to the mask).  A NaN is zero in both channels.  The reference's
 *                    np.uint8(m) / np.uint8(1 - m) on a mask in [0,1] is t_in = 1, t_out = 0; with fractional values the two
 *                    channels are not complements, hence two thresholds.  t_in and t_out are ignored for A3D_EDT_SRC_U8. */
#define A3D_EDT_SRC_U8 0
#define A3D_EDT_SRC_F32 1

/* bytes of scratch a3d_edt_fwd needs for M image-channels of H x W: one 16-bit column offset per pixel, rounded up to 16 bytes.
 * 0 when the sizes are outside the limits below. */
size_t a3d_edt_scratch_bytes(int M, int H, int W);

/* Two launches.  The first walks the columns (lanes are neighbouring columns, the rows are split over the waves of a work-group,
 * which exchange their first and last zero rows through LDS) and leaves in scratch, per pixel and channel, the signed row offset to
 * the nearest zero pixel of its column (the row above on a tie), or a sentinel.  The second gives a work-group one row of one
 * image-channel: its offsets sit in LDS and lane x minimises (x - x')^2 + offset[x']^2 over x', walking outward from x and stopping
 * as soon as (x - x')^2 alone rules out an improvement.
 * Outputs, each [M,H,W] and each optional, at least one required: dist float32, d2 int32, idx int32.
 * Limits: M >= 1 (even for A3D_EDT_SRC_F32), 1 <= H, W <= A3D_EDT_MAX_SIDE, M * H * W < 2^31, scale > 0; scratch of
 * a3d_edt_scratch_bytes(M, H, W) bytes, 2-byte aligned. */
int a3d_edt_fwd(const void* src, int src_kind, float t_in, float t_out, int M, int H, int W, double scale, void* scratch, float* dist,
                int32_t* d2, int32_t* idx, a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
