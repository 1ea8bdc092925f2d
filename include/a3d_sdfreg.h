/* liba3d_hip: the SDF sign-agreement regulariser (the seventh public header of the library; the core surface is a3d.h, the BSDFs are
 * a3d_bsdf.h, the image-space derivatives a3d_deriv.h, the tangent frame a3d_tangent.h, the mesh regularisers a3d_reg.h, the
 * environment-lit shade a3d_envshade.h).
 *
 * Same conventions as a3d.h: flat C, device pointers + sizes + a3d_stream_t, int status (A3D_OK / A3D_EINVAL / A3D_EHIP) with the
 * message in a3d_last_error(), arguments validated before anything is launched, no allocation and no synchronisation inside a call.
 * The entry points live in the same liba3d_hip.so; they do not change a3d_version().
 *
 * sdf_bce_reg_loss of the reference's model/geometry/dmtet.py:161-169 over an edge list all_edges[Ne,2] of a tet grid, called once per
 * training iteration (AnimalModel.py:312), restated:
 *     (a, b) = (sdf[e0], sdf[e1]);  the edge CROSSES iff sign3(a) != sign3(b),  sign3(x) = (x > 0) - (x < 0)
 *                                   (-0.0 and 0.0 are 0; so is a NaN, as torch.sign has it: a NaN crosses a non-zero value only)
 *     bce(x, t) = (1 - t) x - log_sigmoid(x) = max(x, 0) - x t + log1p(exp(-|x|))             (dmtet.py:165-166)
 *     loss = sum bce(a, [b > 0]) / M + sum bce(b, [a > 0]) / M   over the M crossing edges     (M == 0: nan)
 *     g_sdf[e0] += g (sigmoid(a) - [b > 0]) / M,   g_sdf[e1] += g (sigmoid(b) - [a > 0]) / M   (M == 0: all zero)
 * Rows may come in any order, repeat (each counts), run e0 > e1 or e0 == e1.  Terms and sums are carried in double and rounded to
 * float32 once; sums across work-groups are per-group partials added in a fixed order, the gradient is a gather over a static
 * vertex -> (edge, side) list: no atomics on floats, the same bits on every run.  Indices are trusted: the caller has checked them
 * against [0, Nv).
 */
#ifndef A3D_SDFREG_H
#define A3D_SDFREG_H

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* edge rows one work-group of the forward's first launch reads; it writes one partial of three 8-byte words */
#define A3D_SDF_BCE_BLOCK_EDGES 1024
#define A3D_SDF_BCE_PARTIAL_WORDS 3

/* Two launches.  The first streams the int32 rows (16-byte loads: all_edges must be 16-byte aligned), gathers the two values, tests the
 * crossing rule and evaluates the two terms of the crossing rows in double; a work-group adds its terms in a fixed order and writes one
 * partial (sum bce(a, .), sum bce(b, .), count as int64).  The second, one work-group, adds the partials in a fixed order:
 *     loss[0]  = (float)(S_a / M + S_b / M)
 *     state[0] = M,  state[1] = 1 / M (0 when M == 0)          DOUBLES, for a3d_sdf_bce_bwd
 * partials: A3D_SDF_BCE_PARTIAL_WORDS * ceil(Ne / A3D_SDF_BCE_BLOCK_EDGES) 8-byte words of scratch.  Nv > 0, 0 < Ne < 2^30. */
int a3d_sdf_bce_fwd(const float* sdf, int Nv, const int32_t* all_edges, int Ne, double* partials, double* state, float* loss,
                    a3d_stream_t stream);

/* g_loss (one float on the device) -> g_sdf[Nv], fully written, one launch: one thread per grid vertex walks its incidence list
 * inc[inc_off[v] .. inc_off[v + 1]), entries 2 * edge + side in ascending order, recomputes the crossing test of each entry's edge
 * and adds sigmoid(mine) - [other > 0] in list order in double; one float32 store per vertex.  inc_off: int32 [Nv + 1], inc: int32
 * [2 Ne] (every (edge, side) once, under the vertex all_edges[edge][side]).  state: as a3d_sdf_bce_fwd left it. */
int a3d_sdf_bce_bwd(const float* g_loss, const float* sdf, int Nv, const int32_t* all_edges, int Ne, const int32_t* inc_off,
                    const int32_t* inc, const double* state, float* g_sdf, a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
