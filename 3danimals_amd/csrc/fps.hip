// Farthest-point sampling on the device: the first stage of a3d_estimate_bones when the caller appends the resample tail
// (a3d_eb_fps_tail, eb_common.h; include/a3d.h describes it).  Restates geometry/util.sample_farthest_points (reference
// geometry/util.py:5-27), a Python loop of one argmax, one gather, one norm and one minimum per pick: pos[N,V,3] -> k indices per cloud
// and the k points themselves.
//   pick 0   the cloud's start index, read from a device tensor (clamped into [0, V): whatever it holds, every index written is in range)
//   pick i   the arg-max over ALL points of the running minimum of  d = sqrt(dx*dx + dy*dy + dz*dz)  in float32, evaluated in that order
//            (the file is built with -ffp-contract=off; sqrtf is correctly rounded under the build's flags).  Ties go to the LOWEST index, as torch.max on the CPU
//            and every other arg-extremum of this library.  A point already picked has distance 0: when k exceeds the number of distinct
//            points the maximum is 0 everywhere and the pick is index 0, as in the reference.
//   NaN      ordered as torch orders it: a NaN distance (a NaN coordinate, or inf - inf) is GREATER than every number, +inf included, and
//            the running minimum keeps a NaN once it has one (torch.minimum propagates).  So a point with a NaN coordinate is picked
//            first (the lowest such index); every distance to it is NaN, and from then on every pick is index 0.  A point with an
//            infinite coordinate is at distance inf from the finite ones and at NaN from itself: once picked, it is picked again every
//            time.  Nothing traps, nothing waits: the call always writes k indices in [0, V).
// One work-group per cloud, grid = N; nothing waits for another work-group and the loop over the k picks is the only sequential loop
// (the loops over a thread's own points are bounded by V).  Distances are kept as their bit patterns: for d >= +0 the unsigned pattern orders
// like the float, NaN canonicalised to FPS_NAN_KEY sorts above +inf, and  pattern << 32 | ~index  makes one 64-bit maximum the arg-max
// with the lowest index on ties.  Per pick: every thread brings its points' running minima up to date and finds its best, the wave
// takes the maximum with DPP moves (a3d_common.h's controls), one lane per wave writes it to LDS, ONE barrier (the slots alternate
// between two sets, so the next pick's writes cannot overtake this pick's reads), and every row of 16 lanes reduces the waves' entries.
// Two regimes, by V alone:
//   V <= A3D_FPS_REG_MAX_V   coordinates and running minima in registers (P = 1, 2, 3, 4, 6, 8, 12 or 16 points per thread; 256 threads up to
//                            FPS_SMALL_MAX_V points, 1024 above); the winner's coordinates travel through LDS with its key.  No global
//                            memory is touched between the prologue and the outputs.
//   above, to A3D_FPS_MAX_V  coordinates re-read through L2 every pick, running minima in the caller's workspace ([N, V] words, each
//                            word read and written by one thread only); the winner's coordinates are re-read from pos.
// Integer comparisons only between threads: two calls on the same input give the same bits.
#include "eb_common.h"

#define FPS_THREADS 1024
#define FPS_SMALL_THREADS 256
#define FPS_SMALL_MAX_V 256  // up to here one point per thread of a 256-thread work-group (a barrier of 4 waves, not 16)
#define FPS_REG_MAX_P 16     // points per thread in the register regime
#define FPS_NAN_KEY 0x7FC00000u
#define FPS_INF_KEY 0x7F800000u
static_assert(A3D_FPS_REG_MAX_V == FPS_THREADS * FPS_REG_MAX_P, "include/a3d.h states where the register regime ends");
static_assert(A3D_FPS_MAX_V >= 131072 && A3D_FPS_MAX_V <= A3D_EB_WIDE_MAX_POINTS, "the documented limit of V");
static_assert(FPS_THREADS / 64 <= 16, "a row of 16 lanes reduces the waves' entries");

typedef unsigned long long u64;

namespace {

struct FpsParams {
    const float* pos;      // [N, V, 3]
    const int64_t* start;  // [N]
    float* sampled;        // [N, k, 3]
    int64_t* idx;          // [N, k] or null
    unsigned* dist;        // beyond A3D_FPS_REG_MAX_V: [N, V] running minima (bit patterns)
    int V, k;
};

// the distance's bit pattern; NaN (any sign, any payload) -> FPS_NAN_KEY
__device__ __forceinline__ unsigned fps_key(float px, float py, float pz, float x, float y, float z) {
    const float dx = px - x, dy = py - y, dz = pz - z;
    const float d = sqrtf(dx * dx + dy * dy + dz * dz);  // (correctly rounded under the build's -fhip-fp32-correctly-rounded-divide-sqrt, as in every other file)
    return min(__float_as_uint(d), FPS_NAN_KEY);  // (d >= +0 or a quiet NaN: every NaN pattern, of either sign, is above FPS_NAN_KEY or equal to it)
}
// torch.minimum on the patterns: NaN (the greatest pattern there is) stays
__device__ __forceinline__ unsigned fps_min(unsigned m, unsigned c) { return max(m, c) == FPS_NAN_KEY ? FPS_NAN_KEY : min(m, c); }
__device__ __forceinline__ u64 fps_pack(unsigned key, int v) { return ((u64)key << 32) | (u64)(0xFFFFFFFFu - (unsigned)v); }
// the index a packed key carries (clamped: whatever was compared, what comes out addresses a point of the cloud)
__device__ __forceinline__ int fps_index(u64 k, int V) { return (int)min(0xFFFFFFFFu - (unsigned)k, (unsigned)(V - 1)); }

// max(k, k of the lane the DPP control names); the whole wave arrives together
template <int CTRL>
__device__ __forceinline__ u64 fps_dpp_max(u64 k) {
    const u64 o = ((u64)(unsigned)a3d_dpp<CTRL>((int)(k >> 32)) << 32) | (u64)(unsigned)a3d_dpp<CTRL>((int)(unsigned)k);
    return o > k ? o : k;
}
// ... of the lane a row broadcast names; the rows outside ROWS read 0, the identity of this maximum
template <int CTRL, int ROWS>
__device__ __forceinline__ u64 fps_bcast_max(u64 k) {
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(k >> 32), CTRL, ROWS, 0xf, false);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)k, CTRL, ROWS, 0xf, false);
    const u64 o = ((u64)hi << 32) | lo;
    return o > k ? o : k;
}
// maximum over the aligned row of 16 lanes, in every lane of it
__device__ __forceinline__ u64 fps_row16_max(u64 k) {
    k = fps_dpp_max<A3D_DPP_QUAD_XOR1>(k);
    k = fps_dpp_max<A3D_DPP_QUAD_XOR2>(k);
    k = fps_dpp_max<A3D_DPP_ROW_HALF_MIRROR>(k);
    return fps_dpp_max<A3D_DPP_ROW_MIRROR>(k);
}
// maximum over the wave, in lane 63 (the rows' maxima walk up as the sums of a3d_wave_incl_scan do)
__device__ __forceinline__ u64 fps_wave_max_in_lane63(u64 k) {
    k = fps_row16_max(k);
    k = fps_bcast_max<A3D_DPP_ROW_BCAST15, 0xa>(k);
    return fps_bcast_max<A3D_DPP_ROW_BCAST31, 0xc>(k);
}
// the work-group's maximum from the waves' entries, in every lane: lane r of each row of 16 reads wave r's entry
template <int WAVES>
__device__ __forceinline__ u64 fps_block_max(const uint2* s_best) {
    const int r = threadIdx.x & 15;
    const uint2 e = r < WAVES ? s_best[r] : make_uint2(0u, 0u);
    return fps_row16_max(((u64)e.x << 32) | e.y);
}

__device__ __forceinline__ int fps_start(const FpsParams& a, int n) {
    const long long s = a.start[n];
    return (int)(s < 0 ? 0 : (s >= a.V ? a.V - 1 : s));
}
__device__ __forceinline__ void fps_emit(const FpsParams& a, int n, int i, int cur, float px, float py, float pz) {
    const long long o = (long long)n * a.k + i;
    a.sampled[3 * o] = px; a.sampled[3 * o + 1] = py; a.sampled[3 * o + 2] = pz;
    if (a.idx) a.idx[o] = cur;
}

// ---- V <= THREADS * P: everything in registers.  Thread t owns the points j * THREADS + t.
template <int THREADS, int P>
__global__ __launch_bounds__(THREADS) void fps_reg_kernel(const FpsParams a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ uint2 s_best[2][16];
    __shared__ float4 s_xyz[2][16];
    const int tid = threadIdx.x, wave = tid >> 6, n = blockIdx.x, V = a.V;
    const float* __restrict__ p = a.pos + (long long)n * V * 3;
    float x[P], y[P], z[P];
    unsigned m[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {  // a slot past the cloud's end holds a copy of its LAST point: equal keys, a higher index -- it never wins
        const int v = min(j * THREADS + tid, V - 1);
        x[j] = p[3 * v]; y[j] = p[3 * v + 1]; z[j] = p[3 * v + 2];
        m[j] = FPS_INF_KEY;
    }
    int cur = fps_start(a, n), par = 0;
    float px = p[3 * cur], py = p[3 * cur + 1], pz = p[3 * cur + 2];
    for (int i = 0;; ++i) {
        if (tid == 0) fps_emit(a, n, i, cur, px, py, pz);
        if (i + 1 >= a.k) break;
        // the thread's best: its points ascend in index, so a strictly greater key keeps the lowest index among equals
        m[0] = fps_min(m[0], fps_key(px, py, pz, x[0], y[0], z[0]));
        unsigned bk = m[0];
        int bj = 0;
        float bx = x[0], by = y[0], bz = z[0];
#pragma unroll
        for (int j = 1; j < P; ++j) {
            m[j] = fps_min(m[j], fps_key(px, py, pz, x[j], y[j], z[j]));
            if (m[j] > bk) { bk = m[j]; bj = j; bx = x[j]; by = y[j]; bz = z[j]; }
        }
        const u64 best = fps_pack(bk, bj * THREADS + tid);
        const u64 w63 = fps_wave_max_in_lane63(best);
        const u64 wmax = ((u64)(unsigned)__builtin_amdgcn_readlane((int)(w63 >> 32), 63) << 32) | (u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)w63, 63);
        if (best == wmax) {  // the one lane that owns the wave's winner
            s_best[par][wave] = make_uint2((unsigned)(wmax >> 32), (unsigned)wmax);
            s_xyz[par][wave] = make_float4(bx, by, bz, 0.f);
        }
        __syncthreads();
        cur = fps_index(fps_block_max<WAVES>(s_best[par]), V);
        const float4 c = s_xyz[par][(cur & (THREADS - 1)) >> 6];  // the wave of the thread that owns point ``cur``
        px = c.x; py = c.y; pz = c.z;
        par ^= 1;
    }
}

// ---- any V: coordinates through L2, running minima in the workspace.  Thread t owns the points t, t + FPS_THREADS, ..
__global__ __launch_bounds__(FPS_THREADS) void fps_mem_kernel(const FpsParams a) {
    constexpr int WAVES = FPS_THREADS / 64;
    __shared__ uint2 s_best[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.x, V = a.V;
    const float* __restrict__ p = a.pos + (long long)n * V * 3;
    unsigned* __restrict__ m = a.dist + (long long)n * V;
    int cur = fps_start(a, n), par = 0;
    float px = p[3 * cur], py = p[3 * cur + 1], pz = p[3 * cur + 2];
    for (int i = 0;; ++i) {
        if (tid == 0) fps_emit(a, n, i, cur, px, py, pz);
        if (i + 1 >= a.k) break;
        u64 best = 0ull;
#pragma unroll 8
        for (int v = tid; v < V; v += FPS_THREADS) {
            const unsigned old = i == 0 ? FPS_INF_KEY : m[v];  // (the first pass writes every word it will ever read)
            const unsigned now = fps_min(old, fps_key(px, py, pz, p[3 * v], p[3 * v + 1], p[3 * v + 2]));
            if (i == 0 || now != old) m[v] = now;
            const u64 key = fps_pack(now, v);
            best = key > best ? key : best;
        }
        best = fps_wave_max_in_lane63(best);
        if (lane == 63) s_best[par][wave] = make_uint2((unsigned)(best >> 32), (unsigned)best);
        __syncthreads();
        cur = fps_index(fps_block_max<WAVES>(s_best[par]), V);
        px = p[3 * cur]; py = p[3 * cur + 1]; pz = p[3 * cur + 2];
        par ^= 1;
    }
}

template <int THREADS, int P>
void fps_launch_reg(const FpsParams& p, int N, hipStream_t stream) {
    hipLaunchKernelGGL((fps_reg_kernel<THREADS, P>), dim3(N), dim3(THREADS), 0, stream, p);
}

}  // namespace

// the sampler of a validated call with the resample tail (a3d_estimate_bones, bones.hip)
int eb_fps_launch(const a3d_estimate_bones_args* args, const a3d_eb_fps_tail* tail, hipStream_t stream) {
    FpsParams p;
    p.pos = args->pos; p.start = tail->start; p.sampled = tail->sampled; p.idx = tail->idx;
    p.dist = reinterpret_cast<unsigned*>(args->workspace); p.V = args->V; p.k = tail->k;
    const int N = args->N, V = args->V;
    if (V <= FPS_SMALL_MAX_V) fps_launch_reg<FPS_SMALL_THREADS, 1>(p, N, stream);
    else if (V <= FPS_THREADS) fps_launch_reg<FPS_THREADS, 1>(p, N, stream);
    else if (V <= FPS_THREADS * 2) fps_launch_reg<FPS_THREADS, 2>(p, N, stream);
    else if (V <= FPS_THREADS * 3) fps_launch_reg<FPS_THREADS, 3>(p, N, stream);
    else if (V <= FPS_THREADS * 4) fps_launch_reg<FPS_THREADS, 4>(p, N, stream);
    else if (V <= FPS_THREADS * 6) fps_launch_reg<FPS_THREADS, 6>(p, N, stream);
    else if (V <= FPS_THREADS * 8) fps_launch_reg<FPS_THREADS, 8>(p, N, stream);
    else if (V <= FPS_THREADS * 12) fps_launch_reg<FPS_THREADS, 12>(p, N, stream);
    else if (V <= A3D_FPS_REG_MAX_V) fps_launch_reg<FPS_THREADS, FPS_REG_MAX_P>(p, N, stream);
    else hipLaunchKernelGGL(fps_mem_kernel, dim3(N), dim3(FPS_THREADS), 0, stream, p);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
