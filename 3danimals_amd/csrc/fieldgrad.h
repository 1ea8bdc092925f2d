/* liba3d_hip: the input gradient of a scalar coordinate field and its adjoint -- the kernels behind hostnets.USE_FIELD_GRAD (the eikonal
 * regulariser).  An INTERNAL header: these entry points serve the package's own hostnets / ops.py, are registered in
 * _lib.INTERNAL_SURFACES and are no part of the public surface under include/ (126 entry points, a3d_version() 405: both unchanged).
 * Same conventions as include/a3d.h: flat C, device pointers + sizes + a3d_stream_t, int status with the message in a3d_last_error(),
 * arguments validated before anything is launched, no allocation and no synchronisation inside a call. */
#ifndef A3D_FIELDGRAD_H
#define A3D_FIELDGRAD_H

#include "../../include/a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the input gradient of a scalar field and its adjoint (the eikonal regulariser: d sdf / d points, then the gradient of a loss on
 * that with respect to the weights).  A bias-free Linear/ReLU stack is piecewise linear, so every mask (y_l > 0) is a constant of the
 * point, and with e = embed(x), y_0 = relu(e W_in^T), y_l = relu(y_(l-1) W_l^T), out = y_L w^T:
 *     gradient  b_L = (s w) * (y_L > 0),  b_(l-1) = (b_l W_l) * (y_(l-1) > 0)  [a3d_gemm_nn_relumask],  g_x = J_e(x)^T (b_0 W_in)
 *     adjoint   dv = J_e(x) lam,  t_0 = (dv W_in^T) * (y_0 > 0),  t_l = (t_(l-1) W_l^T) * (y_l > 0),  dW_l = b_l^T t_(l-1),
 *               dW_in = b_0^T dv,  dw = sum_m s[m] t_L[m,:],  ds = t_L w
 * Every mask is strictly > 0 on the float32 given (a denormal passes; -0.0 and a NaN do not) and is applied as a select. */

/* C[M,256] = (A[M,K] . B[256,K]^T) * (X[M,256] > 0), X NULL: the plain product.  B is a Linear's [out,in] weight as stored.
 * One launch of 64 x 128 tiles for every M (made for short lists: 1e4 rows are 314 work-groups).  Limits: N == 256, K > 0 and
 * K % 4 == 0, 0 <= M < 2^31 - 256; A and B 16-byte aligned. */
int a3d_gemm_nt_relumask(const float* A, const float* B, const float* X, int64_t M, int N, int K, float* C, a3d_stream_t stream);

/* d_emb[P, 3 + 6 n + ones] = J_e(x) lam: the tangent of a3d_harmonic_embed_fwd (a3d.h) along lam [P,3], same layout and arguments;
 * d|x_0|/dx_0 is 0 at +-0 under symmetrize and the ones column's tangent is 0. */
int a3d_harmonic_embed_jvp(const float* x, const float* lam, const float* freq, int n, int symmetrize, int ones, int64_t P, float* d_emb,
                           a3d_stream_t stream);

/* b[M,256] = (s[m] w[k]) * (y[m,k] > 0): s [M], w [256] (the head's weight), y [M,256].  1 <= M < 2^31; w, y, b 16-byte aligned. */
int a3d_field_grad_head_fwd(const float* s, const float* w, const float* y, int64_t M, float* b, a3d_stream_t stream);

/* bytes of scratch a3d_field_grad_head_bwd needs (one [256] partial sum per 64 rows); 0 when M is outside 1 <= M < 2^31. */
size_t a3d_field_grad_head_scratch_bytes(int64_t M);

/* g_w[256] = sum_m s[m] t[m,:] and, unless g_s is NULL, g_s[M] = t w.  Two launches; the partial sums of the work-groups are added in a
 * fixed order (no atomics: the same bits on every run).  t and w 16-byte aligned. */
int a3d_field_grad_head_bwd(const float* s, const float* t, const float* w, int64_t M, void* scratch, float* g_w, float* g_s,
                            a3d_stream_t stream);

/* bytes of scratch a3d_gemm_tn_splitk needs (the splits' partial products); 0 when the sizes are outside its limits. */
size_t a3d_gemm_tn_splitk_scratch_bytes(int64_t M, int NQ, int batch);

/* C[b][256,NQ] = P[b]^T Q[b] for b < batch: P [batch,M,256], Q [batch,M,NQ], all contiguous -- the weight gradients of a short list, every
 * layer in one call.  Split-K over the rows, the splits' partial products added in ascending order by a second launch (no atomics: the
 * same bits on every run).  Limits: 1 <= M < 2^31 - 256, 4 <= NQ <= 256 and NQ % 4 == 0, 1 <= batch <= 64; P, Q, C and scratch 16-byte
 * aligned. */
int a3d_gemm_tn_splitk(const float* P, const float* Q, int64_t M, int NQ, int batch, void* scratch, float* C, a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
