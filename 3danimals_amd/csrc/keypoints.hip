// Keypoint-transfer evaluation on gfx950 (include/a3d_eval.h): which vertices an image shows (the evaluate_keypoint branch of the
// reference's visualization/visualize_results.py:238-246) and the visible vertex nearest to every keypoint (transfer_keypoints,
// evaluation/evaluate.py:461-472).
//
// Visibility: one thread per pixel, the triangle id from the raster buffer, three plain stores of 1.0f -- many writers of one value, so
// the order does not matter; a lane whose id is that of its left neighbour in the same row skips them (one DPP move, no LDS).
// Nearest vertex: a work-group streams a slab of one image's vertices, a lane keeps the best (order(d2), v) of up to 16 keypoints in
// registers, the work-group reduces them and publishes one 64-bit atomicMin per keypoint, as the rasteriser does with depth || id.
#include "../../include/a3d_eval.h"
#include "a3d_common.h"

namespace {

typedef unsigned long long u64;

constexpr int KP_THREADS = 256;
constexpr int KP_MAX_BLOCKS = 2048;    // grid-strided clears
constexpr int NVV_WAVES = A3D_NVV_THREADS / 64;
constexpr int NVV_TILE = A3D_NVV_KEYPOINT_TILE;
constexpr int NVV_TARGET_WORKGROUPS = 2048;  // 256 CUs x 8

// ---- visibility
__global__ __launch_bounds__(KP_THREADS) void vis_clear_kernel(float* __restrict__ vis, long long n, int* __restrict__ ok) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *ok = 1;
    for (long long i = (long long)blockIdx.x * KP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * KP_THREADS) vis[i] = 0.f;
}

// thread p is pixel p of [B,H,W]; blockDim.x is a multiple of 64, so lane - 1 holds pixel p - 1
__global__ __launch_bounds__(KP_THREADS) void vis_pixels_kernel(const float4* __restrict__ rast, const int* __restrict__ tri, int total, int HW, int W,
                                                                int F, int V, float* __restrict__ vis, int* __restrict__ ok) {
    const long long pl = (long long)blockIdx.x * KP_THREADS + threadIdx.x;  // (total may end less than a work-group below 2^31)
    const bool live = pl < total;
    const int p = (int)pl;
    int id = 0;  // 0: nothing to store
    bool bad = false;
    if (live) {
        const float w = rast[p].w;
        if (w >= 0.f && w < 2147483648.f && w == truncf(w))  // (a NaN fails the first test)
            id = (int)w;
        if (!(w >= 0.f) || id != w || id > F) {
            id = 0;
            bad = true;
        }
    }
    // every lane of the wave arrives here: the id of lane - 1 within the row of 16 lanes, 0 for the first lane of a row
    const int left = a3d_dpp<A3D_DPP_ROW_SHR + 1>(id);
    if (id > 0 && !(left == id && p % W != 0)) {
        const int* row = tri + (size_t)(id - 1) * 3;
        const int a = row[0], b = row[1], c = row[2];
        if ((unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V) {
            float* out = vis + (size_t)(p / HW) * V;
            out[a] = 1.f;
            out[b] = 1.f;
            out[c] = 1.f;
        } else {
            bad = true;
        }
    }
    if (bad) *ok = 0;
}

// ---- nearest visible vertex
__global__ __launch_bounds__(KP_THREADS) void nvv_arm_kernel(u64* __restrict__ keys, int n) {
    for (int i = blockIdx.x * KP_THREADS + threadIdx.x; i < n; i += gridDim.x * KP_THREADS) keys[i] = ~0ull;
}

__global__ __launch_bounds__(KP_THREADS) void nvv_finish_kernel(const u64* __restrict__ keys, int n, int* __restrict__ idx) {
    for (int i = blockIdx.x * KP_THREADS + threadIdx.x; i < n; i += gridDim.x * KP_THREADS) idx[i] = (int)(unsigned)(keys[i] & 0xFFFFFFFFull);
}

// order(d2): d2 is +0 or above, +inf or a NaN; its bits are monotone over the first three, + 1 keeps 0 for the NaN
__device__ __forceinline__ unsigned nvv_order(float d2) { return d2 != d2 ? 0u : __float_as_uint(d2) + 1u; }

template <int M>
__device__ __forceinline__ u64 nvv_min_xor(u64 k) {
    const unsigned lo = (unsigned)a3d_lane_xor<M>((int)(unsigned)k), hi = (unsigned)a3d_lane_xor<M>((int)(unsigned)(k >> 32));
    const u64 o = ((u64)hi << 32) | lo;
    return o < k ? o : k;
}

// work-group blockIdx.x = n * slabs + s owns the vertices [s * slab, min(V, (s + 1) * slab)) of image n
__global__ __launch_bounds__(A3D_NVV_THREADS) void nvv_slab_kernel(const float2* __restrict__ uv, const float* __restrict__ vis,
                                                                  const float2* __restrict__ kp, int V, int K, int slab, int slabs,
                                                                  u64* __restrict__ keys) {
    __shared__ float2 s_kp[NVV_TILE];
    __shared__ u64 s_red[NVV_WAVES][NVV_TILE];
    const int n = blockIdx.x / slabs, s = blockIdx.x % slabs;
    const int v0 = s * slab, v1 = min(V, v0 + slab);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float2* uvn = uv + (size_t)n * V;
    const float* visn = vis + (size_t)n * V;
    for (int k0 = 0; k0 < K; k0 += NVV_TILE) {
        if (threadIdx.x < NVV_TILE) s_kp[threadIdx.x] = k0 + threadIdx.x < K ? kp[(size_t)n * K + k0 + threadIdx.x] : make_float2(0.f, 0.f);
        __syncthreads();
        unsigned bo[NVV_TILE], bv[NVV_TILE];
#pragma unroll
        for (int j = 0; j < NVV_TILE; ++j) {
            bo[j] = 0xFFFFFFFFu;
            bv[j] = 0xFFFFFFFFu;
        }
#pragma unroll 2
        for (int v = v0 + threadIdx.x; v < v1; v += A3D_NVV_THREADS) {
            float2 q = uvn[v];
            if (visn[v] == 0.f) q = make_float2(INFINITY, INFINITY);
#pragma unroll
            for (int j = 0; j < NVV_TILE; ++j) {
                const float2 c = s_kp[j];
                const float dx = q.x - c.x, dy = q.y - c.y;
                const float xx = dx * dx, yy = dy * dy;
                const unsigned o = nvv_order(xx + yy);
                if (o < bo[j]) {  // a lane meets its vertices in ascending order: strictly smaller keeps the lowest index
                    bo[j] = o;
                    bv[j] = (unsigned)v;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NVV_TILE; ++j) {
            u64 key = ((u64)bo[j] << 32) | bv[j];
            key = nvv_min_xor<1>(key);
            key = nvv_min_xor<2>(key);
            key = nvv_min_xor<4>(key);
            key = nvv_min_xor<8>(key);
            key = nvv_min_xor<16>(key);
            key = nvv_min_xor<32>(key);
            if (lane == 0) s_red[wave][j] = key;
        }
        __syncthreads();
        if (threadIdx.x < NVV_TILE && k0 + threadIdx.x < K) {
            u64 key = s_red[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < NVV_WAVES; ++w) key = min(key, s_red[w][threadIdx.x]);
            atomicMin(keys + (size_t)n * K + k0 + threadIdx.x, key);  // fire and forget
        }
        // (s_kp is rewritten by threads that passed the barrier above; s_red only behind the next trip's first barrier)
    }
}

inline int nvv_slab(int N, int V) {
    long long trips = (long long)N * V / ((long long)A3D_NVV_THREADS * NVV_TARGET_WORKGROUPS);
    trips = trips < 1 ? 1 : (trips > A3D_NVV_MAX_TRIPS ? A3D_NVV_MAX_TRIPS : trips);
    return A3D_NVV_THREADS * (int)trips;
}

}  // namespace

extern "C" int a3d_vertex_visibility_fwd(const float* rast, const int32_t* tri, int B, int H, int W, int F, int V, float* vis, int32_t* ok,
                                         a3d_stream_t stream) {
    A3D_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && F >= 1 && V >= 1);
    A3D_CHECK_ARG((long long)B * H * W < (1ll << 31) && (long long)B * V < (1ll << 31));
    A3D_CHECK_ARG(rast && tri && vis && ok);
    A3D_CHECK_ARG(((uintptr_t)rast & 15) == 0 && ((uintptr_t)tri & 3) == 0 && ((uintptr_t)vis & 3) == 0 && ((uintptr_t)ok & 3) == 0);
    hipStream_t s = (hipStream_t)stream;
    const long long nv = (long long)B * V;
    hipLaunchKernelGGL(vis_clear_kernel, dim3(min(a3d_div_up(nv, KP_THREADS), KP_MAX_BLOCKS)), dim3(KP_THREADS), 0, s, vis, nv, ok);
    A3D_LAUNCH_CHECK();
    const int total = B * H * W;
    hipLaunchKernelGGL(vis_pixels_kernel, dim3(a3d_div_up(total, KP_THREADS)), dim3(KP_THREADS), 0, s, (const float4*)rast, tri, total, H * W, W, F, V, vis,
                       ok);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" size_t a3d_nearest_visible_vertex_scratch_bytes(int N, int K) {
    if (N < 1 || K < 1 || (long long)N * K >= (1ll << 31)) return 0;
    return (size_t)N * K * sizeof(u64);
}

extern "C" int a3d_nearest_visible_vertex_slab(int N, int V) { return N < 1 || V < 1 ? 0 : nvv_slab(N, V); }

extern "C" int a3d_nearest_visible_vertex_fwd(const float* uv, const float* vis, const float* kp, int N, int V, int K, uint64_t* keys, int32_t* idx,
                                              a3d_stream_t stream) {
    A3D_CHECK_ARG(N >= 1 && V >= 1 && K >= 1 && V <= (1 << 30));
    A3D_CHECK_ARG((long long)N * V < (1ll << 31) && (long long)N * K < (1ll << 31));
    A3D_CHECK_ARG(uv && vis && kp && keys && idx);
    A3D_CHECK_ARG(((uintptr_t)uv & 7) == 0 && ((uintptr_t)kp & 7) == 0 && ((uintptr_t)keys & 7) == 0 && ((uintptr_t)vis & 3) == 0 &&
                  ((uintptr_t)idx & 3) == 0);
    const int slab = nvv_slab(N, V), slabs = a3d_div_up(V, slab);
    A3D_CHECK_ARG((long long)N * slabs < (1ll << 31));
    hipStream_t s = (hipStream_t)stream;
    const int nk = N * K, small = min(a3d_div_up(nk, KP_THREADS), KP_MAX_BLOCKS);
    hipLaunchKernelGGL(nvv_arm_kernel, dim3(small), dim3(KP_THREADS), 0, s, (u64*)keys, nk);
    A3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(nvv_slab_kernel, dim3(N * slabs), dim3(A3D_NVV_THREADS), 0, s, (const float2*)uv, vis, (const float2*)kp, V, K, slab, slabs,
                       (u64*)keys);
    A3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(nvv_finish_kernel, dim3(small), dim3(KP_THREADS), 0, s, (const u64*)keys, nk, idx);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
