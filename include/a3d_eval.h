/* liba3d_hip: keypoint-transfer evaluation -- per-vertex visibility from a raster buffer, and the nearest visible vertex of every
 * keypoint (the tenth public header of the library; the core surface is a3d.h, the BSDFs are a3d_bsdf.h, the image-space derivatives
 * a3d_deriv.h, the tangent frame a3d_tangent.h, the mesh regularisers a3d_reg.h, the environment-lit shade a3d_envshade.h, the SDF
 * regulariser a3d_sdfreg.h, the distance transform a3d_edt.h, the field heads a3d_fields.h).
 *
 * Same conventions as a3d.h: flat C, device pointers + sizes + a3d_stream_t, int status (A3D_OK / A3D_EINVAL / A3D_EHIP) with the
 * message in a3d_last_error(), arguments validated before anything is launched, no allocation and no synchronisation inside a call.
 * The entry points live in the same liba3d_hip.so; they do not change a3d_version().
 *
 * The two reductions in the middle of the reference's PCK@0.1 evaluation:
 *   visibility  (visualization/visualize_results.py:238-246, the evaluate_keypoint branch): per image, the ids > 0 of the raster
 *               buffer, the rows of the triangle list they name, the unique corners, a scatter of 1 into visibility[num_verts];
 *   nearest     (evaluation/evaluate.py:461-472, transfer_keypoints): invisible vertices overwritten with inf, a [K,V] distance
 *               matrix, argmin along V.
 * Both are forward-only, compare / integer work with a defined tie rule: the same bits on every run.
 */
#ifndef A3D_EVAL_H
#define A3D_EVAL_H

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vertices a work-group of the nearest-vertex launch streams per thread-trip, and the most trips per thread: a slab of an image's
 * vertices is A3D_NVV_THREADS * trips vertices, 1 <= trips <= A3D_NVV_MAX_TRIPS */
#define A3D_NVV_THREADS 256
#define A3D_NVV_MAX_TRIPS 32
/* keypoints a work-group carries in registers at a time; more keypoints are served by further passes over the slab */
#define A3D_NVV_KEYPOINT_TILE 16

/* vis[b, v] = 1 exactly when v is a corner of a triangle whose id is stored in at least one pixel of image b, else 0.
 *   rast [B,H,W,4] float32, channel 3 holds the triangle id + 1, 0 = empty (a3d_rast_fwd's texels); tri [F,3] int32;
 *   vis  [B,V] float32 (out; cleared by this call); ok int32 [1] (out; set to 1 by this call, then to 0 by the launch when it met data
 *   it had to skip).
 * Two launches: a clear of vis (and the arming of ok), then one thread per pixel -- a lane whose id equals that of its left neighbour
 * in the same row (read across lanes, no LDS) skips its three stores; the stores are plain stores of the constant 1.0f, so the result
 * does not depend on their order.
 * A pixel whose channel 3 is not a whole number in [0, F] (an id above F, a negative one, a NaN) and a triangle row with a corner
 * outside [0, V) never index anything: the pixel is skipped and *ok becomes 0.  The caller looks at ok when it next reads back.
 * Limits: B, H, W, F, V >= 1, B * H * W < 2^31, B * V < 2^31; rast 16-byte aligned; no pointer NULL. */
int a3d_vertex_visibility_fwd(const float* rast, const int32_t* tri, int B, int H, int W, int F, int V, float* vis, int32_t* ok,
                              a3d_stream_t stream);

/* bytes of the keys scratch of a3d_nearest_visible_vertex_fwd: one 64-bit key per (image, keypoint).  0 when N or K is < 1 or
 * N * K >= 2^31. */
size_t a3d_nearest_visible_vertex_scratch_bytes(int N, int K);

/* vertices per work-group (the slab) that a3d_nearest_visible_vertex_fwd uses for N images of V vertices: a multiple of
 * A3D_NVV_THREADS, chosen so that N * ceil(V / slab) work-groups fill the chip for one image as well as for thousands.  0 when N or V
 * is < 1. */
int a3d_nearest_visible_vertex_slab(int N, int V);

/* idx[n, k] = the visible vertex of image n nearest to keypoint k.
 *   uv [N,V,2] float32 projected vertices; vis [N,V] float32 (0 = invisible, anything else visible); kp [N,K,2] float32 keypoints in the
 *   same frame; keys [N,K] 64-bit scratch (armed by this call); idx [N,K] int32 (out).
 * The arithmetic, one float32 operation each, in this order, never contracted:
 *     (x, y) = vis[n,v] == 0 ? (+inf, +inf) : uv[n,v]          (the reference's source_verts[visibility == 0] = np.inf)
 *     dx = x - kp.x;  dy = y - kp.y;  d2 = dx * dx + dy * dy    (so an invisible vertex has d2 = +inf for every finite keypoint)
 *     idx = the index of the smallest d2, the lowest index among equals (np.argmin's rule);
 *     a NaN d2 counts as smaller than every number, the lowest such index first (np.argmin's rule again): a NaN keypoint gives 0,
 *     a NaN coordinate of a visible vertex makes the first such vertex win;
 *     no visible vertex: every d2 is +inf, idx = 0.
 * Three launches: keys armed; a work-group owns a slab of one image's vertices, reads each once per tile of A3D_NVV_KEYPOINT_TILE
 * keypoints (held in LDS), keeps a best (order(d2), v) per lane and keypoint, reduces across the work-group and publishes one
 * fire-and-forget 64-bit atomic minimum per (keypoint, work-group) of order(d2) << 32 | v, order(NaN) = 0 < order(0); a last tiny launch
 * turns keys into idx.  A minimum over (d2, v) does not depend on the order it is taken in.
 * Limits: N, V, K >= 1, V <= 2^30, N * V < 2^31, N * K < 2^31; uv and keys 8-byte aligned; no pointer NULL. */
int a3d_nearest_visible_vertex_fwd(const float* uv, const float* vis, const float* kp, int N, int V, int K, uint64_t* keys, int32_t* idx,
                                   a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
