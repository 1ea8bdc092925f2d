// The output stage of the fields' MLPs on gfx950 (include/a3d_fields.h): Linear(256 -> C <= 16) + sigmoid + min_max map after the
// last hidden ReLU, and its adjoint together with that ReLU's, one pass over the hidden vectors h [M,256] each way.
//
// Both kernels are v_mfma_f32_16x16x4_f32 (exact fp32) on tiles of 16 rows of h, one tile per wave at a time, no barrier in the
// main loops.  Lane l = (j = l & 15, q = l >> 4) supplies one A element [i = j][kk = q] and one B element [kk = q][j] per MFMA
// and owns D[4 q + r][j], r = 0..3.  Which contraction index a (kk, step) pair stands for is free, so every operand is picked such that
// a lane's 16-byte global load IS its next four operands:
//   forward   D[m][c] = sum_k h[m][k] W[c][k]: lane (j, q) loads h[m0 + j][16 g + 4 q .. + 3] (A) and holds W[j][16 g + 4 q .. + 3] (B)
//             for g = 0..15 -- all of W is 64 registers per lane, read once per wave.
//   g_h       D[k][m] = sum_c W[c][k] ga[m][c] (the transposed product): lane (j, q) owns g_h[m0 + j][16 nb + 4 q .. + 3], which is the
//             float4 it stores and the float4 of h whose signs mask it; the operand W[4 u + q][16 nb + j] is read from LDS.
//   g_W       D[c][k] = sum_m ga[m][c] h[m][k]: the contraction runs over the rows, so h is needed with the rows on (q, step): lane
//             (j, q) loads h[m0 + q + 4 step][64 blk + 4 j .. + 3] -- a quarter wave reads 256 contiguous bytes -- and component t
//             of that float4 goes to the accumulator of columns 64 blk + 4 j + t.  This second read of the tile hits the cache.
// A wave accumulates g_W over its 8 tiles, the 4 waves of a work-group are added through LDS in wave order and the work-group's
// [C,256] goes to scratch; fh_reduce_kernel adds the work-groups' partial sums in ascending order.  No atomics.
#include "../../include/a3d_fields.h"
#include "fieldgrad.h"
#include "a3d_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int FH_K = A3D_FIELD_HEAD_WIDTH;
constexpr int FH_WAVES = 4;
constexpr int FH_TILE = 16;           // rows of one MFMA tile
constexpr int FH_TILES_PER_WAVE = 8;  // consecutive tiles a wave walks
constexpr int FH_WAVE_ROWS = FH_TILE * FH_TILES_PER_WAVE;
static_assert(FH_WAVE_ROWS * FH_WAVES == A3D_FIELD_HEAD_WG_ROWS && FH_K == 256, "the header states the work-group's rows");
constexpr int FH_WPAD = FH_K + 16;  // row stride of W in LDS (fh_bwd_kernel)
constexpr int FH_RED_SEGS = 16;  // fh_reduce_kernel: the partial sums are added in this many runs, then the runs

__device__ __forceinline__ f32x4 fh_load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ float fh_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
// the adjoint of out = act(pre) * scale + lo with respect to pre, from the saved s = act(pre): autograd's own order of operations
// (scale is 1 without the map)
template <bool ACT>
__device__ __forceinline__ float fh_adjoint(float g, float s, float scale) {
    g = g * scale;
    return ACT ? g * ((1.f - s) * s) : g;
}

__global__ __launch_bounds__(64 * FH_WAVES, 2) void fh_fwd_kernel(const float* __restrict__ h, const float* __restrict__ W,
                                                                  const float* __restrict__ lo, const float* __restrict__ scale, int act,
                                                                  long long M, int C, float* __restrict__ s_out, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 w[16];  // W[j][16 g + 4 q .. + 3]; channels past C are zero columns of the product
#pragma unroll
    for (int g = 0; g < 16; ++g) w[g] = j < C ? fh_load4(W + j * FH_K + 16 * g + 4 * q) : zero4;
    const bool map = scale != nullptr;
    const float sc = map && j < C ? scale[j] : 1.f, l0 = map && j < C ? lo[j] : 0.f;
    const long long row0 = ((long long)blockIdx.x * FH_WAVES + wave) * FH_WAVE_ROWS;
    for (int t = 0; t < FH_TILES_PER_WAVE; ++t) {
        const long long m0 = row0 + FH_TILE * t;
        if (m0 >= M) break;  // (wave-uniform)
        const long long mr = m0 + j < M ? m0 + j : M - 1;  // ragged last tile: clamp the loads, skip the stores
        const float* hp = h + mr * FH_K + 4 * q;
        f32x4 a[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) a[g] = fh_load4(hp + 16 * g);
        // eight independent chains of 32 products, added pairwise at the end: the MFMAs issue back to back, and the rounding error
        // stays near that of a blocked CPU dot product
        f32x4 acc[8] = {zero4, zero4, zero4, zero4, zero4, zero4, zero4, zero4};
#pragma unroll
        for (int g = 0; g < 16; ++g)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[g & 7] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][u], w[g][u], acc[g & 7], 0, 0, 0);
        const f32x4 d = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long m = m0 + 4 * q + r;
            if (m < M && j < C) {
                float v = d[r];
                if (act == A3D_FIELD_HEAD_ACT_SIGMOID) v = fh_sigmoid(v);
                if (act != A3D_FIELD_HEAD_ACT_NONE || map) s_out[m * C + j] = v;
                if (map) v = v * sc + l0;
                out[m * C + j] = v;
            }
        }
    }
}

// One tile of 16 rows of the backward.  RAGGED: the tile crosses M -- loads are clamped to the last row and their values zeroed where they
// would add to g_W, stores are skipped; a full tile has no per-lane condition at all.  Every load is unconditional (a load under a
// per-lane condition becomes a branch of its own with a full wait behind it), the scalar g_out / s loads are issued first, and the
// float4 loads of column block blk + 1 are issued before the MFMAs of block blk.
template <int NS, bool ACT, bool RAGGED>
__device__ __forceinline__ void fh_bwd_tile(const float* __restrict__ g_out, const float* __restrict__ s, const float* __restrict__ h,
                                            long long M, int C, long long m0, int j, int q, const float* w_lane, const float (&sc_b)[NS],
                                            float sc_a, float* __restrict__ g_h, f32x4 (&accw)[4][4]) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const bool live = !RAGGED || m0 + j < M;
    const long long mb = live ? m0 + j : M - 1;
    const int cj = j < C ? j : C - 1;
    float gb[NS], sb[NS], ga[4], sa[4];  // g_out (and s) at [m0 + j][4 u + q] and at [m0 + q + 4 step][j]
    long long ma[4];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        const int c = 4 * u + q < C ? 4 * u + q : C - 1;
        gb[u] = g_out[mb * C + c];
        sb[u] = ACT ? s[mb * C + c] : 0.f;
    }
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        const long long m = m0 + q + 4 * st;
        ma[st] = !RAGGED || m < M ? m : M - 1;
        ga[st] = g_out[ma[st] * C + cj];
        sa[st] = ACT ? s[ma[st] * C + cj] : 0.f;
    }
    const float* h_mask = h + mb * FH_K + 4 * q;
    float* gh_row = g_h + mb * FH_K + 4 * q;
    f32x4 hb[2][4], hm[2][4];
#pragma unroll
    for (int st = 0; st < 4; ++st) hb[0][st] = fh_load4(h + ma[st] * FH_K + 4 * j);
#pragma unroll
    for (int i = 0; i < 4; ++i) hm[0][i] = fh_load4(h_mask + 16 * i);
    // the adjoints; channels past C and rows past M are zero operands
#pragma unroll
    for (int u = 0; u < NS; ++u) gb[u] = 4 * u + q < C ? fh_adjoint<ACT>(gb[u], sb[u], sc_b[u]) : 0.f;
#pragma unroll
    for (int st = 0; st < 4; ++st) ga[st] = j < C && (!RAGGED || m0 + q + 4 * st < M) ? fh_adjoint<ACT>(ga[st], sa[st], sc_a) : 0.f;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
        const int cur = blk & 1, nxt = cur ^ 1;
        if (blk + 1 < 4) {
#pragma unroll
            for (int st = 0; st < 4; ++st) hb[nxt][st] = fh_load4(h + ma[st] * FH_K + 64 * (blk + 1) + 4 * j);
#pragma unroll
            for (int i = 0; i < 4; ++i) hm[nxt][i] = fh_load4(h_mask + 16 * (4 * (blk + 1) + i));
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the next block's loads above this block's MFMAs
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const f32x4 hv = !RAGGED || m0 + q + 4 * st < M ? hb[cur][st] : zero4;
#pragma unroll
            for (int t = 0; t < 4; ++t) accw[blk][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[st], hv[t], accw[blk][t], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int nb = 4 * blk + i;
            f32x4 d = zero4;
#pragma unroll
            for (int u = 0; u < NS; ++u) d = __builtin_amdgcn_mfma_f32_16x16x4f32(w_lane[4 * u * FH_WPAD + 16 * nb], gb[u], d, 0, 0, 0);
            // h > 0 on the bits: every positive float, denormals included, is a positive integer (and -0.0 is a negative one)
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = __float_as_int(hm[cur][i][r]) > 0 ? d[r] : 0.f;
            if (live) *reinterpret_cast<f32x4*>(gh_row + 16 * nb) = d;
        }
    }
}

// NS = ceil(C / 4): MFMA steps of the g_h product (step u contracts the channels 4 u .. 4 u + 3); ACT: the sigmoid's adjoint (reads s)
template <int NS, bool ACT>
__global__ __launch_bounds__(64 * FH_WAVES, 2) void fh_bwd_kernel(const float* __restrict__ g_out, const float* __restrict__ s,
                                                                  const float* __restrict__ h, const float* __restrict__ W,
                                                                  const float* __restrict__ scale, long long M, int C,
                                                                  float* __restrict__ g_h, float* __restrict__ partial) {
    // 64 KB: the waves' g_W sums at the end; before that its head holds W, zero-padded to 16 rows of FH_WPAD floats (the operand read of
    // lane (j, q), row 4 u + q, column 16 nb + j, is conflict-free with the pad: q and q + 1 share a 32-lane half and sit 16 banks apart)
    __shared__ float red[FH_WAVES][A3D_FIELD_HEAD_MAX_C * FH_K];
    static_assert(A3D_FIELD_HEAD_MAX_C * FH_WPAD <= FH_WAVES * A3D_FIELD_HEAD_MAX_C * FH_K, "W fits");
    float* w_lds = &red[0][0];
    for (int f = threadIdx.x; f < A3D_FIELD_HEAD_MAX_C * (FH_K / 4); f += 64 * FH_WAVES) {
        const int c = f / (FH_K / 4), k4 = f % (FH_K / 4);
        const f32x4 v = fh_load4(W + (c < C ? c : C - 1) * FH_K + 4 * k4);
        *reinterpret_cast<f32x4*>(w_lds + c * FH_WPAD + 4 * k4) = c < C ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, q = lane >> 4;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const bool map = scale != nullptr;
    const float* w_lane = w_lds + q * FH_WPAD + j;  // W[4 u + q][16 nb + j] at + 4 u FH_WPAD + 16 nb
    float sc_b[NS];  // the scale of channel 4 u + q (1 without the map: g * 1 is g)
#pragma unroll
    for (int u = 0; u < NS; ++u) sc_b[u] = map ? scale[4 * u + q < C ? 4 * u + q : C - 1] : 1.f;
    const float sc_a = map ? scale[j < C ? j : C - 1] : 1.f;  // g_W: this lane's channel is j
    f32x4 accw[4][4];  // [blk][t]: g_W[4 q + r][64 blk + 4 j + t] in component r
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int t = 0; t < 4; ++t) accw[b][t] = zero4;

    const long long row0 = ((long long)blockIdx.x * FH_WAVES + wave) * FH_WAVE_ROWS;
    for (int tile = 0; tile < FH_TILES_PER_WAVE; ++tile) {
        const long long m0 = row0 + FH_TILE * tile;
        if (m0 >= M) break;  // (wave-uniform; every wave still reaches the barrier below)
        if (m0 + FH_TILE <= M) fh_bwd_tile<NS, ACT, false>(g_out, s, h, M, C, m0, j, q, w_lane, sc_b, sc_a, g_h, accw);
        else fh_bwd_tile<NS, ACT, true>(g_out, s, h, M, C, m0, j, q, w_lane, sc_b, sc_a, g_h, accw);
    }
    // the waves' sums -> LDS (once every wave is done with W), added in wave order -> this work-group's partial sum
    __syncthreads();
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f32x4 v = {accw[blk][0][r], accw[blk][1][r], accw[blk][2][r], accw[blk][3][r]};
            *reinterpret_cast<f32x4*>(&red[wave][(4 * q + r) * FH_K + 64 * blk + 4 * j]) = v;
        }
    __syncthreads();
    float* mine = partial + (size_t)blockIdx.x * C * FH_K;
    for (int f = threadIdx.x; f < C * (FH_K / 4); f += 64 * FH_WAVES) {
        f32x4 v = *reinterpret_cast<const f32x4*>(&red[0][4 * f]);
#pragma unroll
        for (int w = 1; w < FH_WAVES; ++w) v += *reinterpret_cast<const f32x4*>(&red[w][4 * f]);
        *reinterpret_cast<f32x4*>(mine + 4 * f) = v;
    }
}

template <int NS>
void fh_launch_bwd(bool act, dim3 grid, dim3 block, hipStream_t st, const float* g_out, const float* s, const float* h, const float* W,
                   const float* scale, long long M, int C, float* g_h, float* partial) {
    if (act) hipLaunchKernelGGL((fh_bwd_kernel<NS, true>), grid, block, 0, st, g_out, s, h, W, scale, M, C, g_h, partial);
    else hipLaunchKernelGGL((fh_bwd_kernel<NS, false>), grid, block, 0, st, g_out, s, h, W, scale, M, C, g_h, partial);
}

// g_W[e] = sum over the work-groups' partial sums, e < n = C * 256: thread (seg, i) adds run seg of the partial sums of element
// 16 blockIdx.x + i in ascending order, then the first 16 threads add the runs in ascending order.
__global__ __launch_bounds__(16 * FH_RED_SEGS) void fh_reduce_kernel(const float* __restrict__ partial, int n_wg, int n, float* __restrict__ g_W) {
    __shared__ float runs[FH_RED_SEGS][16];
    const int i = threadIdx.x & 15, seg = threadIdx.x >> 4, e = 16 * blockIdx.x + i;  // (n is a multiple of 16)
    const int per = (n_wg + FH_RED_SEGS - 1) / FH_RED_SEGS;
    const int w0 = min(seg * per, n_wg), w1 = min(w0 + per, n_wg);
    float acc = 0.f;
    const float* p = partial + e;
    int w = w0;
    for (; w + 8 <= w1; w += 8) {  // eight loads in flight, added in order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(w + u) * n];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; w < w1; ++w) acc += p[(size_t)w * n];
    runs[seg][i] = acc;
    __syncthreads();
    if (seg == 0) {
        float t = runs[0][i];
#pragma unroll
        for (int k = 1; k < FH_RED_SEGS; ++k) t += runs[k][i];
        g_W[e] = t;
    }
}

// ---- the head of the field's INPUT gradient (the SDF regulariser differentiates a Linear(256 -> 1) head with respect to the points) ----
// forward  b[m,k] = (s[m] w[k]) * (y[m,k] > 0): where the gradient chain of a scalar field starts; one thread per float4 of b.
__global__ __launch_bounds__(256) void fg_head_fwd_kernel(const float* __restrict__ s, const float* __restrict__ w, const float* __restrict__ y,
                                                          long long M, float* __restrict__ b) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // float4 index
    if (i >= M * (FH_K / 4)) return;
    const long long m = i / (FH_K / 4);
    const int k4 = (int)(i - m * (FH_K / 4));
    const float sv = s[m];
    const f32x4 wv = fh_load4(w + 4 * k4), yv = fh_load4(y + 4 * i);
    f32x4 d;
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = yv[r] > 0.f ? sv * wv[r] : 0.f;  // strictly positive: a denormal passes, -0.0 and a NaN do not
    *reinterpret_cast<f32x4*>(b + 4 * i) = d;
}

// adjoint  g_w[k] = sum_m s[m] t[m,k] and (g_s != NULL) g_s[m] = sum_k t[m,k] w[k].  A work-group takes FG_ROWS rows: thread k adds its
// column over them in ascending order and leaves the sum in partial[work-group][k] (fh_reduce_kernel adds those, in order); for g_s wave v
// takes the rows v, v + 4, ..: a lane multiplies its float4 of the row, the wave adds by butterfly -- the same tree on every run.
constexpr int FG_ROWS = 64;

__global__ __launch_bounds__(FH_K) void fg_head_bwd_kernel(const float* __restrict__ s, const float* __restrict__ t, const float* __restrict__ w,
                                                           long long M, float* __restrict__ partial, float* __restrict__ g_s) {
    const int k = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * FG_ROWS;
    const int rows = (int)(M - m0 < FG_ROWS ? M - m0 : FG_ROWS);
    float acc = 0.f;
    for (int r = 0; r < rows; ++r) acc += s[m0 + r] * t[(m0 + r) * FH_K + k];
    partial[(size_t)blockIdx.x * FH_K + k] = acc;
    if (g_s != nullptr) {
        const int lane = k & 63, wave = k >> 6;
        const f32x4 wv = fh_load4(w + 4 * lane);
        for (int r = wave; r < rows; r += FH_K / 64) {
            const f32x4 tv = fh_load4(t + (m0 + r) * FH_K + 4 * lane);
            const float v = a3d_wave_sum((tv[0] * wv[0] + tv[1] * wv[1]) + (tv[2] * wv[2] + tv[3] * wv[3]));
            if (lane == 0) g_s[m0 + r] = v;
        }
    }
}

inline bool fh_sizes_ok(int64_t M, int C) { return M >= 1 && M < (1ll << 31) && C >= 1 && C <= A3D_FIELD_HEAD_MAX_C; }
inline int fh_work_groups(int64_t M) { return (int)((M + A3D_FIELD_HEAD_WG_ROWS - 1) / A3D_FIELD_HEAD_WG_ROWS); }
inline bool fh_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t a3d_field_head_scratch_bytes(int64_t M, int C) {
    if (!fh_sizes_ok(M, C)) return 0;
    return (size_t)fh_work_groups(M) * C * FH_K * sizeof(float);
}

extern "C" int a3d_field_head_fwd(const float* h, const float* W, const float* lo, const float* scale, int act, int64_t M, int C, float* s,
                                  float* out, a3d_stream_t stream) {
    A3D_CHECK_ARG(fh_sizes_ok(M, C));
    A3D_CHECK_ARG(act == A3D_FIELD_HEAD_ACT_NONE || act == A3D_FIELD_HEAD_ACT_SIGMOID);
    A3D_CHECK_ARG((lo == nullptr) == (scale == nullptr));
    A3D_CHECK_ARG(h && W && out && fh_aligned16(h) && fh_aligned16(W));
    A3D_CHECK_ARG(s || (act == A3D_FIELD_HEAD_ACT_NONE && !scale));
    hipLaunchKernelGGL(fh_fwd_kernel, dim3(fh_work_groups(M)), dim3(64 * FH_WAVES), 0, (hipStream_t)stream, h, W, lo, scale, act, (long long)M, C, s,
                       out);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_field_head_bwd(const float* g_out, const float* s, const float* h, const float* W, const float* scale, int act, int64_t M,
                                  int C, void* scratch, float* g_h, float* g_W, a3d_stream_t stream) {
    A3D_CHECK_ARG(fh_sizes_ok(M, C));
    A3D_CHECK_ARG(act == A3D_FIELD_HEAD_ACT_NONE || act == A3D_FIELD_HEAD_ACT_SIGMOID);
    A3D_CHECK_ARG(g_out && h && W && g_h && g_W && scratch);
    A3D_CHECK_ARG(s || act == A3D_FIELD_HEAD_ACT_NONE);
    A3D_CHECK_ARG(fh_aligned16(h) && fh_aligned16(W) && fh_aligned16(g_h) && fh_aligned16(scratch));
    hipStream_t st = (hipStream_t)stream;
    const int n_wg = fh_work_groups(M);
    const dim3 grid(n_wg), block(64 * FH_WAVES);
    float* partial = (float*)scratch;
    const bool sig = act == A3D_FIELD_HEAD_ACT_SIGMOID;
    switch ((C + 3) / 4) {
        case 1: fh_launch_bwd<1>(sig, grid, block, st, g_out, s, h, W, scale, (long long)M, C, g_h, partial); break;
        case 2: fh_launch_bwd<2>(sig, grid, block, st, g_out, s, h, W, scale, (long long)M, C, g_h, partial); break;
        case 3: fh_launch_bwd<3>(sig, grid, block, st, g_out, s, h, W, scale, (long long)M, C, g_h, partial); break;
        default: fh_launch_bwd<4>(sig, grid, block, st, g_out, s, h, W, scale, (long long)M, C, g_h, partial); break;
    }
    A3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(fh_reduce_kernel, dim3(C * FH_K / 16), dim3(16 * FH_RED_SEGS), 0, st, partial, n_wg, C * FH_K, g_W);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" size_t a3d_field_grad_head_scratch_bytes(int64_t M) {
    if (M < 1 || M >= (1ll << 31)) return 0;
    return (size_t)((M + FG_ROWS - 1) / FG_ROWS) * FH_K * sizeof(float);
}

extern "C" int a3d_field_grad_head_fwd(const float* s, const float* w, const float* y, int64_t M, float* b, a3d_stream_t stream) {
    A3D_CHECK_ARG(M >= 1 && M < (1ll << 31));
    A3D_CHECK_ARG(s && w && y && b && fh_aligned16(w) && fh_aligned16(y) && fh_aligned16(b));
    hipLaunchKernelGGL(fg_head_fwd_kernel, dim3(a3d_div_up(M * (FH_K / 4), 256)), dim3(256), 0, (hipStream_t)stream, s, w, y, (long long)M, b);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_field_grad_head_bwd(const float* s, const float* t, const float* w, int64_t M, void* scratch, float* g_w, float* g_s,
                                       a3d_stream_t stream) {
    A3D_CHECK_ARG(M >= 1 && M < (1ll << 31));
    A3D_CHECK_ARG(s && t && w && scratch && g_w && fh_aligned16(t) && fh_aligned16(w));
    const int n_wg = (int)((M + FG_ROWS - 1) / FG_ROWS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fg_head_bwd_kernel, dim3(n_wg), dim3(FH_K), 0, st, s, t, w, (long long)M, (float*)scratch, g_s);
    A3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(fh_reduce_kernel, dim3(FH_K / 16), dim3(16 * FH_RED_SEGS), 0, st, (const float*)scratch, n_wg, FH_K, g_w);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
