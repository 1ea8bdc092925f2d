/* liba3d_hip: the tangent frame (the fourth public header of the library; the core surface is a3d.h, the BSDFs are a3d_bsdf.h, the
 * image-space derivatives a3d_deriv.h).
 *
 * Same conventions as a3d.h: flat C, device pointers + sizes + a3d_stream_t, int status (A3D_OK / A3D_EINVAL / A3D_EHIP) with the
 * message in a3d_last_error(), arguments validated before anything is launched, no allocation and no synchronisation inside a call.
 * The entry points live in the same liba3d_hip.so; they do not change a3d_version().
 *
 * Two halves of normal mapping: per-vertex tangents from the uv atlas (compute_tangents) and the per-pixel shading normal with a
 * tangent-space perturbation (prepare_shading_normal).
 */
#ifndef A3D_TANGENT_H
#define A3D_TANGENT_H

#include "a3d_bsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* op code of a3d_shading_normal_* in an a3d_bsdf_desc (the descriptor of a3d_bsdf.h, unchanged; a3d_bsdf_fwd / _bwd refuse this code).
 * Inputs in the reference's argument order: pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm, 3 channels each -> 3. */
#define A3D_SHADING_NORMAL 5
#define A3D_SHADING_NORMAL_TWO_SIDED 1 /* variant bit 0: two_sided_shading */
#define A3D_SHADING_NORMAL_OPENGL 2    /* variant bit 1: opengl (the bitangent's sign is -1) */

/* Work-groups of a launch over this descriptor = partial rows of a reduced gradient: a3d_bsdf_rows' rule,
 * (pixels / seg) * ceil(seg / A3D_BSDF_TILE); -1 for an invalid descriptor.  Touches no pointer. */
int64_t a3d_shading_normal_rows(const a3d_bsdf_desc* desc);

/* prepare_shading_normal with a perturbed normal (reference renderutils/ops.py:194-227 -> bsdf.py:30-51; c_src/normal.cu
 * PrepareShadingNormalFwdKernel / BwdKernel): one launch each way, element-wise over the pixels of the broadcast result.
 *     n = normalize(smooth_nrm), view = normalize(view_pos - pos), t = normalize(smooth_tng), bt = normalize(cross(t, n))
 *     n = normalize(t p.x + sign bt p.y + n max(p.z, 0)),  sign = -1 under A3D_SHADING_NORMAL_OPENGL
 *     two sided: front = dot(geom_nrm, view) > 0 flips n and geom_nrm;  out = lerp(g, n, clamp(dot(view, n) / 0.1, 0, 1))
 * normalize is F.normalize (eps 1e-12); the subgradients at every clamp / where are autograd's.
 * fwd reads in[], writes out [pixels, 3].  bwd reads in[] and g_out, recomputes the forward and writes every wanted gradient (g_mode per
 * input: A3D_BSDF_GRAD_NONE / _DIRECT / _REDUCE, as for a3d_bsdf_bwd) from the same launch, plus one finishing launch when any gradient
 * is reduced; the partial rows are doubles and are added in a fixed order (no float atomics: two calls give the same bits).  The forward
 * is float32; the backward carries its per-pixel arithmetic in double (the adjoint of a normalize is a difference of nearly equal
 * terms) and rounds each gradient once.  min_roughness and scratch are not read. */
int a3d_shading_normal_fwd(const a3d_bsdf_desc* desc, a3d_stream_t stream);
int a3d_shading_normal_bwd(const a3d_bsdf_desc* desc, a3d_stream_t stream);

/* compute_tangents (reference model/render/mesh.py:310-350) for a mesh whose normal indices are its position indices:
 * v_pos[B,V,3], v_nrm[B,V,3], v_tex[.,Nuv,2] with tex_batch_stride ELEMENTS between the images' atlases (0: one atlas shared by every
 * image), t_pos_idx[F,3], t_tex_idx[F,3]; off / adj: the vertex -> (corner, face) lists of t_pos_idx in the format of
 * a3d_normals_adjacency (lists_stride 0) or of the DMTet emit launch (lists_stride > 0).  Indices are trusted.
 * One thread per (image, vertex) walks its list in ascending key order, recomputes every incident face's tangent
 *     (pe1 uve2.y - pe2 uve1.y) / where(denom > 0, max(denom, 1e-6), min(denom, -1e-6)),  denom = uve1.x uve2.y - uve1.y uve2.x
 * and sums; the sum / corner count is safe-normalised (x / sqrt(max(x.x, 1e-20))), made orthogonal to v_nrm and safe-normalised again
 * -> v_tng[B,V,3].  Face tangents, sums and normalisations are carried in double.  A vertex with no face gets 0 / 0 = NaN. */
int a3d_tangents_fwd(const float* v_pos, const float* v_tex, int64_t tex_batch_stride, const float* v_nrm, const int32_t* t_pos_idx,
                     const int32_t* t_tex_idx, const int32_t* off, const int32_t* adj, int lists_stride, int B, int V, int F, float* v_tng,
                     a3d_stream_t stream);
/* g_tng[B,V,3] (contiguous) -> g_v_pos[B,V,3], g_v_nrm[B,V,3] (both fully written), two launches, no atomics, bit-reproducible.
 * Pass 1 per vertex: the forward's sum again, the adjoint through both normalisations and the projection; g_v_nrm and the adjoint of the
 * sum -> g_sum_scratch[B,V,3] DOUBLES.  Pass 2 per vertex: over the same list, the three scratch rows of each incident face give that
 * face's tangent adjoint; this corner's share of g_pe1 / g_pe2 is added in ascending key order.  v_tex receives no gradient. */
int a3d_tangents_bwd(const float* g_tng, const float* v_pos, const float* v_tex, int64_t tex_batch_stride, const float* v_nrm,
                     const int32_t* t_pos_idx, const int32_t* t_tex_idx, const int32_t* off, const int32_t* adj, int lists_stride, int B, int V,
                     int F, double* g_sum_scratch, float* g_v_pos, float* g_v_nrm, a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
