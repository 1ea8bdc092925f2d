// The exact Euclidean distance transform of batched binary images on gfx950 (include/a3d_edt.h): what the reference's
// compute_distance_transform (model/dataset/util.py:12-18) gets from cv2.distanceTransform(..., DIST_L2, DIST_MASK_PRECISE) on the host.
//
// Separable, two launches, integers until the final store, no atomics.  Columns: lanes are neighbouring columns (every row read is
// coalesced), the rows of a column are split over the waves of a work-group; a lane keeps the zero pixels of its rows as bit masks in
// registers (both channels of a float mask from ONE read), the waves exchange their first and last zero rows through LDS, and the
// signed row offset to the nearest zero pixel of the column comes out of count-leading / count-trailing-zeros on the masks.  Rows: a
// work-group holds the offsets of one row in LDS, lane x walks outward from x and stops as soon as (x - x')^2 alone cannot improve
// its best -- exact, and a few steps for every pixel near the silhouette.
#include "../../include/a3d_edt.h"
#include "a3d_common.h"

namespace {

constexpr int EC_MAX_WAVES = 16;  // waves of a column work-group
constexpr int EC_WORDS = 4;       // 64-row masks a lane holds per channel
static_assert(EC_MAX_WAVES * EC_WORDS * 64 == A3D_EDT_MAX_SIDE, "a column work-group covers the tallest image");
constexpr int ER_THREADS = 256;
constexpr int ER_STEPS = 4;      // distances a lane of the row kernel tries between two tests of its exit (distance only)
constexpr int ER_STEPS_IDX = 1;  // the same with idx: the 64-bit candidates of a group of four cost more than the round trips they saved
constexpr int EDT_NO_ZERO = 32767;  // scratch: the column has no zero pixel (its square exceeds every attainable d2 and the no-zero value)
constexpr int EC_FAR = 1 << 20;     // a row further away than any row of an image
constexpr int EDT_MAX_BLOCKS = 1 << 20;

typedef unsigned long long u64;

// bit c: the pixel of channel c is ZERO.  (Written as negations: a NaN is zero in both channels.)
__device__ __forceinline__ int zero_bits(unsigned char v, float, float) { return v == 0 ? 1 : 0; }
__device__ __forceinline__ int zero_bits(float m, float t_in, float t_out) { return (!(m >= t_in) ? 1 : 0) | (!(m <= t_out) ? 2 : 0); }

// NC = 1: T = unsigned char [N,H,W] -> offsets [N,H,W]; NC = 2: T = float [N,H,W] -> offsets [N,2,H,W].
// blockDim.x = 64 * waves, wave w owns the rows [w * rows_per_wave, (w + 1) * rows_per_wave) of 64 columns; rows_per_wave <= 64 * EC_WORDS.
template <int NC, typename T>
__global__ __launch_bounds__(64 * EC_MAX_WAVES) void edt_columns_kernel(const T* __restrict__ src, float t_in, float t_out, int N, int H, int W,
                                                                      int rows_per_wave, short* __restrict__ g) {
    __shared__ int s_first[NC][EC_MAX_WAVES][64];
    __shared__ int s_last[NC][EC_MAX_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int tiles = (W + 63) >> 6;
    const int r0 = min(wave * rows_per_wave, H), r1 = min(r0 + rows_per_wave, H);
    for (long long item = blockIdx.x; item < (long long)N * tiles; item += gridDim.x) {
        const int n = (int)(item / tiles), x = (int)(item % tiles) * 64 + lane;
        const bool live = x < W;
        const T* col = src + (size_t)n * H * W + x;
        u64 z[NC][EC_WORDS];
#pragma unroll
        for (int k = 0; k < EC_WORDS; ++k) {
#pragma unroll
            for (int c = 0; c < NC; ++c) z[c][k] = 0;
            const int w0 = r0 + 64 * k;
            for (int j0 = 0; j0 < 64 && w0 + j0 < r1; j0 += 8) {  // eight independent loads in flight
                int bits[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int row = w0 + j0 + u;
                    bits[u] = (live && row < r1) ? zero_bits(col[(size_t)row * W], t_in, t_out) : 0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int c = 0; c < NC; ++c) z[c][k] |= (u64)((bits[u] >> c) & 1) << (j0 + u);
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            int first = EC_FAR, last = -EC_FAR;
#pragma unroll
            for (int k = 0; k < EC_WORDS; ++k)
                if (z[c][k]) {
                    first = min(first, r0 + 64 * k + (int)__builtin_ctzll(z[c][k]));
                    last = max(last, r0 + 64 * k + 63 - (int)__builtin_clzll(z[c][k]));
                }
            s_first[c][wave][lane] = first;
            s_last[c][wave][lane] = last;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            int up = -EC_FAR, dn = EC_FAR;  // the last zero row above my rows, the first one below them
            for (int w = 0; w < waves; ++w) {
                if (w < wave) up = max(up, s_last[c][w][lane]);
                if (w > wave) dn = min(dn, s_first[c][w][lane]);
            }
            int upk[EC_WORDS], dnk[EC_WORDS];  // the same per 64-row mask
#pragma unroll
            for (int k = 0; k < EC_WORDS; ++k) {
                upk[k] = up;
                if (z[c][k]) up = r0 + 64 * k + 63 - (int)__builtin_clzll(z[c][k]);
            }
#pragma unroll
            for (int k = EC_WORDS - 1; k >= 0; --k) {
                dnk[k] = dn;
                if (z[c][k]) dn = r0 + 64 * k + (int)__builtin_ctzll(z[c][k]);
            }
            short* out = g + ((size_t)n * NC + c) * H * W + x;
#pragma unroll
            for (int k = 0; k < EC_WORDS; ++k) {
                const int w0 = r0 + 64 * k;
                const u64 m = z[c][k];
                const int rows = min(64, r1 - w0);
                for (int j = 0; j < rows; ++j) {
                    const int y = w0 + j;
                    const u64 lo = m & (~0ull >> (63 - j)), hi = m >> j;  // zero rows at or above y, at or below y
                    const int a = lo ? w0 + 63 - (int)__builtin_clzll(lo) : upk[k];
                    const int b = hi ? y + (int)__builtin_ctzll(hi) : dnk[k];
                    const int da = y - a, db = b - y;
                    int off = da <= db ? -da : db;  // equally far above and below: the row above
                    if (min(da, db) >= A3D_EDT_MAX_SIDE) off = EDT_NO_ZERO;
                    if (live) out[(size_t)y * W] = (short)off;
                }
            }
        }
        __syncthreads();  // (s_first / s_last are written again by the next item)
    }
}

// one row of one image-channel per trip: its column offsets in LDS, lane x minimises (x - x')^2 + off[x']^2 over x' walking outward.
// IDX: the minimised value is the key d2 << 24 | qy << 12 | qx, whose order is (d2, qy, qx); without it the minimum stays 32-bit.
// The walk goes STEPS distances at a time -- their LDS reads are in flight together instead of one round trip per distance -- and
// tests the exit once per group: a candidate beyond the exact bound has a larger d2 and changes nothing.  s_g holds a sentinel on
// either side of the row, an x' outside the row reads it (its square exceeds every attainable d2).
template <bool IDX>
__global__ __launch_bounds__(ER_THREADS) void edt_rows_kernel(const short* __restrict__ g, long long rows_total, int H, int W, double scale,
                                                              float* __restrict__ dist, int* __restrict__ d2_out, int* __restrict__ idx_out) {
    __shared__ short s_g[A3D_EDT_MAX_SIDE + 2];
    constexpr int STEPS = IDX ? ER_STEPS_IDX : ER_STEPS;
    const int none = H * H + W * W;
    if (threadIdx.x == 0) s_g[0] = s_g[W + 1] = EDT_NO_ZERO;
    for (long long row = blockIdx.x; row < rows_total; row += gridDim.x) {
        const int y = (int)(row % H);
        const short* grow = g + (size_t)row * W;
        for (int i = threadIdx.x; i < W; i += blockDim.x) s_g[i + 1] = grow[i];
        __syncthreads();
        for (int x = threadIdx.x; x < W; x += blockDim.x) {
            const int reach = max(x, W - 1 - x);
            int best = none;
            u64 key = ((u64)none << 24) | 0xFFFFFFull;
            for (int d0 = 0; d0 <= reach; d0 += STEPS) {
                // nothing at d0 or beyond can improve: exact.  (With idx a candidate AT the best distance may still win the tie.)
                if (IDX ? d0 * d0 > best : d0 * d0 >= best) break;
                int gl[STEPS], gr[STEPS];
#pragma unroll
                for (int u = 0; u < STEPS; ++u) {
                    gl[u] = s_g[max(x - d0 - u, -1) + 1];
                    gr[u] = s_g[min(x + d0 + u, W) + 1];
                }
#pragma unroll
                for (int u = 0; u < STEPS; ++u) {
                    const int d = d0 + u, dd = d * d, cl = dd + gl[u] * gl[u], cr = dd + gr[u] * gr[u];
                    if (IDX) {  // (a sentinel's key is 2^54 or more whatever its low fields hold: above every real key, < 2^50)
                        key = min(key, ((u64)cl << 24) + ((u64)(y + gl[u]) << 12) + (u64)(x - d));
                        key = min(key, ((u64)cr << 24) + ((u64)(y + gr[u]) << 12) + (u64)(x + d));
                    } else {
                        best = min(best, min(cl, cr));
                    }
                }
                if (IDX) best = (int)(key >> 24);
            }
            const size_t p = (size_t)row * W + x;
            if (dist) dist[p] = (float)(sqrt((double)best) / scale);
            if (d2_out) d2_out[p] = best;
            if (IDX) idx_out[p] = best == none ? -1 : (int)((key >> 12) & 4095) * W + (int)(key & 4095);
        }
        __syncthreads();  // (s_g is written again by the next trip)
    }
}

inline bool edt_sizes_ok(int M, int H, int W) {
    return M >= 1 && H >= 1 && W >= 1 && H <= A3D_EDT_MAX_SIDE && W <= A3D_EDT_MAX_SIDE && (long long)M * H * W < (1ll << 31);
}

}  // namespace

extern "C" size_t a3d_edt_scratch_bytes(int M, int H, int W) {
    if (!edt_sizes_ok(M, H, W)) return 0;
    return ((size_t)M * H * W * sizeof(short) + 15) & ~(size_t)15;
}

extern "C" int a3d_edt_fwd(const void* src, int src_kind, float t_in, float t_out, int M, int H, int W, double scale, void* scratch, float* dist,
                           int32_t* d2, int32_t* idx, a3d_stream_t stream) {
    A3D_CHECK_ARG(edt_sizes_ok(M, H, W));
    A3D_CHECK_ARG(src_kind == A3D_EDT_SRC_U8 || src_kind == A3D_EDT_SRC_F32);
    A3D_CHECK_ARG(src_kind != A3D_EDT_SRC_F32 || (M % 2 == 0 && ((uintptr_t)src & 3) == 0));
    A3D_CHECK_ARG(scale > 0.0 && scale <= 1.7976931348623157e308);  // (a NaN fails the first test)
    A3D_CHECK_ARG(src && scratch && ((uintptr_t)scratch & 1) == 0);
    A3D_CHECK_ARG(dist || d2 || idx);
    hipStream_t s = (hipStream_t)stream;
    short* g = (short*)scratch;
    const int waves = min(EC_MAX_WAVES, a3d_div_up(H, 16));
    const int rows_per_wave = a3d_div_up(H, waves);
    const int tiles = a3d_div_up(W, 64);
    if (src_kind == A3D_EDT_SRC_U8) {
        const int blocks = (int)min((long long)M * tiles, (long long)EDT_MAX_BLOCKS);
        hipLaunchKernelGGL((edt_columns_kernel<1, unsigned char>), dim3(blocks), dim3(64 * waves), 0, s, (const unsigned char*)src, t_in, t_out, M, H,
                           W, rows_per_wave, g);
    } else {
        const int blocks = (int)min((long long)(M / 2) * tiles, (long long)EDT_MAX_BLOCKS);
        hipLaunchKernelGGL((edt_columns_kernel<2, float>), dim3(blocks), dim3(64 * waves), 0, s, (const float*)src, t_in, t_out, M / 2, H, W,
                           rows_per_wave, g);
    }
    A3D_LAUNCH_CHECK();
    const long long rows_total = (long long)M * H;
    const int blocks = (int)min(rows_total, (long long)EDT_MAX_BLOCKS);
    const int threads = min(ER_THREADS, 64 * a3d_div_up(W, 64));
    if (idx)
        hipLaunchKernelGGL(edt_rows_kernel<true>, dim3(blocks), dim3(threads), 0, s, g, rows_total, H, W, scale, dist, d2, idx);
    else
        hipLaunchKernelGGL(edt_rows_kernel<false>, dim3(blocks), dim3(threads), 0, s, g, rows_total, H, W, scale, dist, d2, idx);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
