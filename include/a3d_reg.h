/* liba3d_hip: the mesh regularisers (the fifth public header of the library; the core surface is a3d.h, the BSDFs are a3d_bsdf.h, the
 * image-space derivatives a3d_deriv.h, the tangent frame a3d_tangent.h).
 *
 * Same conventions as a3d.h: flat C, device pointers + sizes + a3d_stream_t, int status (A3D_OK / A3D_EINVAL / A3D_EHIP) with the
 * message in a3d_last_error(), arguments validated before anything is launched, no allocation and no synchronisation inside a call.
 * The entry points live in the same liba3d_hip.so; they do not change a3d_version().
 *
 * laplace_regularizer_const, normal_consistency and avg_edge_length of the reference's model/render/regularizer.py as atomics-free
 * gathers over the vertex -> (corner, face) lists of a3d.h (off / adj: CSR with lists_stride 0, or the fixed-stride lists of the DMTet
 * emit launch with lists_stride > 0).  Per-element terms and every sum are carried in double; sums across work-groups are per-group
 * partials added in a fixed order, so a value and a gradient have the same bits on every run.  Indices are trusted.
 *
 * A triangle list t_pos_idx[F,3] has 3F directed occurrences: occurrence s = 3f + c runs (i, j) = (tri[f][c], tri[f][(c+1)%3]).  Its
 * undirected key is (min, max); it is FORWARD if i <= j and BACKWARD otherwise.  Unique edges are the distinct keys, E their number.
 * For one unique edge, col0 is the face of its highest forward slot and col1 the face of its highest backward slot; a column without an
 * occurrence holds face 0 (compute_edge_to_face_mapping's zero initialisation, with the order torch's sequential index put leaves on
 * the CPU).
 */
#ifndef A3D_REG_H
#define A3D_REG_H

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bits of the first word of an edge-table row */
#define A3D_EDGE_REPRESENTATIVE 1 /* the highest slot of its key in either direction: one per unique edge */
#define A3D_EDGE_WINNER 2         /* the highest slot of its key in its own direction: its face is that column of the edge */
#define A3D_EDGE_STAND_IN 4       /* no occurrence runs the other way: the partner is face 0 standing in */

/* The per-occurrence edge table of one triangle list, one launch (plus a 4-byte clear of num_edges), no sort, no hash, no read-back:
 * occurrence s scans the list of the lower vertex of its key, which holds every face at that edge.
 *     edge_table[s][0] = A3D_EDGE_* bits,  edge_table[s][1] = the face of the opposite column (0 under A3D_EDGE_STAND_IN)
 *     num_edges[0]     = E (an integer count: the order of its additions does not matter)
 * edge_table is int32 [3F,2]. */
int a3d_edge_topology(const int32_t* t_pos_idx, int F, int V, const int32_t* off, const int32_t* adj, int lists_stride, int32_t* edge_table,
                      int32_t* num_edges, a3d_stream_t stream);

/* Doubles of scratch a forward below needs for (B, n) = (images, vertices) [laplace] or (images, faces) [the other two]. */
size_t a3d_reg_partials(int B, int n);

/* laplace_regularizer_const with the evident [B,F,1] index of its normaliser (the reference's statement raises for every input):
 *     term[b,v] = sum over the corner entries (c,f) of v of ((v_{c+1} - v) + (v_{c+2} - v)) / max(2 n_v, 1),  n_v = entries of v
 *     loss = mean(term^2) over B V 3          (an isolated vertex: 0; a face that lists a vertex twice counts twice)
 * Two launches: one thread per (image, vertex) gathers over its list in ascending key order, then the partials are added.
 * scaled[B,V,3] DOUBLES receives term / max(2 n_v, 1) for the backward; partials: a3d_reg_partials(B, V) doubles; loss: one float. */
int a3d_laplace_fwd(const float* v_pos, const int32_t* t_pos_idx, const int32_t* off, const int32_t* adj, int lists_stride, int B, int V, int F,
                    double* scaled, double* partials, float* loss, a3d_stream_t stream);
/* g_loss (one float on the device) -> g_v_pos[B,V,3], fully written, one launch: the transpose of the gather,
 *     g_v = k (-2 n_v s[v] + sum over (c,f) of v of (s[v_{c+1}] + s[v_{c+2}])),  s = scaled,  k = 2 g_loss / (3 B V). */
int a3d_laplace_bwd(const float* g_loss, const double* scaled, const int32_t* t_pos_idx, const int32_t* off, const int32_t* adj,
                    int lists_stride, int B, int V, int F, float* g_v_pos, a3d_stream_t stream);

/* normal_consistency: n_f = safe_normalize(cross(v1 - v0, v2 - v0)) (x / sqrt(max(x.x, 1e-20))), per unique edge
 * t = (1 - clamp(n_col0 . n_col1, -1, 1)) 0.5, loss = mean |t| over B E.  Two launches: one thread per (image, occurrence), the
 * representatives contribute; then the partials are added and divided by B num_edges[0] on the device.
 * stand_in[B,3] DOUBLES receives, per image, the sum of the normals of the winners whose partner is the face-0 stand-in, each under the
 * mask of its edge's gradient (face 0's share of those edges in the backward).  partials: a3d_reg_partials(B, F) doubles. */
int a3d_normal_consistency_fwd(const float* v_pos, const int32_t* t_pos_idx, const int32_t* edge_table, const int32_t* num_edges, int B, int V,
                               int F, double* stand_in, double* partials, float* loss, a3d_stream_t stream);
/* g_loss -> g_v_pos[B,V,3], fully written, two launches: every face's adjoint once (its winning occurrences gather the partner's normal,
 * face 0 adds stand_in; through the normalisation and the cross product -> face_scratch[B,F,9] DOUBLES), then one thread per
 * (image, vertex) adds its corners' rows in ascending key order.  The subgradients are autograd's: the clamp passes on [-1, 1]
 * inclusive, abs gives 0 at 0. */
int a3d_normal_consistency_bwd(const float* g_loss, const float* v_pos, const int32_t* t_pos_idx, const int32_t* edge_table,
                               const int32_t* num_edges, const int32_t* off, const int32_t* adj, int lists_stride, const double* stand_in, int B,
                               int V, int F, double* face_scratch, float* g_v_pos, a3d_stream_t stream);

/* avg_edge_length: the mean over B E of sqrt(max(|v_i - v_j|^2, 1e-20)).  Two launches, as a3d_normal_consistency_fwd.
 * partials: a3d_reg_partials(B, F) doubles. */
int a3d_edge_length_fwd(const float* v_pos, const int32_t* t_pos_idx, const int32_t* edge_table, const int32_t* num_edges, int B, int V, int F,
                        double* partials, float* loss, a3d_stream_t stream);
/* g_loss -> g_v_pos[B,V,3], fully written, one launch: one thread per (image, vertex) over the two occurrences at each of its corner
 * entries, each counted where it is its edge's representative. */
int a3d_edge_length_bwd(const float* g_loss, const float* v_pos, const int32_t* t_pos_idx, const int32_t* edge_table, const int32_t* num_edges,
                        const int32_t* off, const int32_t* adj, int lists_stride, int B, int V, int F, float* g_v_pos, a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
