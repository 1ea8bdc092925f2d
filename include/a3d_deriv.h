/* liba3d_hip: image-space derivatives (the third public header of the library; the core surface is a3d.h, the BSDFs are a3d_bsdf.h).
 *
 * Same conventions as a3d.h: flat C, device pointers + sizes + a3d_stream_t, int status (A3D_OK / A3D_EINVAL / A3D_EHIP) with the
 * message in a3d_last_error(), arguments validated before anything is launched, no allocation and no synchronisation inside a call.
 * The entry points live in the same liba3d_hip.so; they do not change a3d_version().
 *
 * The two operators that produce uv_da for dr.texture -- the chain of the reference's Texture2D.sample (model/render/texture.py) and
 * of visualize_results.py:87, which passes rast_db on:
 *     rast, rast_db = dr.rasterize(ctx, pos, tri, resolution)                         nvdiffrast: second output, grad_db
 *     uv, uv_da     = dr.interpolate(uv_attr, rast, tri, rast_db=rast_db, diff_attrs='all')
 *     colour        = dr.texture(tex, uv, uv_da)
 *
 * clip[clip_batch,V,4] and attr[attr_batch,V,C] with a batch of 1 (shared by every image: nvdiffrast's range mode) or B;
 * tri[F,3]; rast[B,H,W,4] = (u, v, z/w, triangle id + 1), fully resolved.  A texel whose id is 0 or beyond F is empty: zeros out,
 * nothing back.  Every [B,H,W,4] buffer is 16-byte aligned.
 */
#ifndef A3D_DERIV_H
#define A3D_DERIV_H

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define A3D_DERIV_MAX_SELECTED 64 /* S of a3d_interp_da_*; C <= 64 as for a3d_interp_* */

/* rast_db[B,H,W,4] = (du/dX, du/dY, dv/dX, dv/dY) in units of one pixel: the second output of dr.rasterize /
 * DepthPeeler.rasterize_next_layer (reference render.py:292-294, 351 receive it; visualize_results.py:87 uses it).  Per texel, with
 * f the pixel centre in NDC: q_i = p_i.xy - f p_i.w, a_i = q_j x q_k, s = a_0 + a_1 + a_2, u = a_0 / s, v = a_1 / s and
 * du/dX = (d a_0/d fx * s - a_0 * d s/d fx) / (s * s) * (2 / W), likewise the other three (2 / H for Y).  One launch. */
int a3d_rast_db_fwd(const float* clip, int clip_batch, const int32_t* tri, const float* rast, int B, int V, int F, int H, int W,
                    float* rast_db, a3d_stream_t stream);
/* g_db[B,H,W,4] -> g_clip[clip_batch,V,4] (zeroed by the callee; z receives nothing): nvdiffrast's grad_db=True.  The forward is
 * recomputed per pixel; the rows leave through the per-tile staged scatter of a3d_rast_bwd.  A shared clip sums over the images. */
int a3d_rast_db_bwd(const float* g_db, const float* clip, int clip_batch, const int32_t* tri, const float* rast, int B, int V, int F,
                    int H, int W, float* g_clip, a3d_stream_t stream);

/* out_da[B,H,W,2S] = (dA/dX, dA/dY) per selected attribute, dA/dX = du/dX (A0 - A2) + dv/dX (A1 - A2): the second output of
 * dr.interpolate(attr, rast, tri, rast_db=, diff_attrs=) (reference texture.py, Texture2D.sample; render.py:23-24 passes None).
 * sel[S] (device) lists the selected channels in output order, repeats allowed, each in [0, C); NULL = 'all' (S == C). */
int a3d_interp_da_fwd(const float* attr, int attr_batch, int C, const int32_t* sel_or_null, int S, const float* rast,
                      const float* rast_db, const int32_t* tri, int B, int V, int F, int H, int W, float* out_da, a3d_stream_t stream);
/* g_da[B,H,W,2S] -> g_attr[attr_batch,V,C] (zeroed by the callee, zero on unselected channels; may be null) through the tile scatter,
 * and g_rast_db[B,H,W,4] (fully written; may be null).  The gradient w.r.t. rast is identically zero and is not produced. */
int a3d_interp_da_bwd(const float* g_da, const float* attr, int attr_batch, int C, const int32_t* sel_or_null, int S, const float* rast,
                      const float* rast_db, const int32_t* tri, int B, int V, int F, int H, int W, float* g_attr_or_null,
                      float* g_rast_db_or_null, a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
