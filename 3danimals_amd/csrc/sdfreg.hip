// The SDF sign-agreement regulariser on gfx950 (include/a3d_sdfreg.h): sdf_bce_reg_loss of the reference's model/geometry/dmtet.py:161-169,
// which its Trainer evaluates once per iteration over EVERY edge of the tet grid (AnimalModel.py:312).
//
// Forward: a stream over the int32 edge rows (8 B per edge, 16-byte non-temporal loads, four rows per thread) with two gathers from the
// SDF array, which stays cache resident; the ~1 % of rows that cross evaluate their two terms in double.  A work-group adds its terms in a
// fixed order and writes one partial, a finishing launch of one work-group adds the partials in a fixed order, rounds once and leaves M
// and 1 / M on the device.  (Not finished inside the first launch by a last-block ticket: dmtet.hip records what publishing across XCDs
// cost there.)  Backward: a gather, one thread per grid vertex over its static (edge, side) list; no atomics on floats anywhere.
#include "../../include/a3d_sdfreg.h"
#include "a3d_common.h"

namespace {

constexpr int SB_THREADS = 256;
constexpr int SB_WAVES = SB_THREADS / A3D_WAVE;
constexpr int SB_PAIRS = A3D_SDF_BCE_BLOCK_EDGES / 2 / SB_THREADS;  // 16-byte loads (two rows each) per thread
static_assert(SB_PAIRS * 2 * SB_THREADS == A3D_SDF_BCE_BLOCK_EDGES, "a work-group reads whole 16-byte pairs");

// one partial of the first launch
struct Partial {
    double sum_a, sum_b;
    long long count;
};
static_assert(sizeof(Partial) == 8 * A3D_SDF_BCE_PARTIAL_WORDS, "a partial is A3D_SDF_BCE_PARTIAL_WORDS 8-byte words");

// torch.sign's three classes: -0.0, 0.0 and a NaN are 0
__device__ __forceinline__ int sign3(float x) { return (x > 0.0f) - (x < 0.0f); }
__device__ __forceinline__ bool crosses(float a, float b) { return sign3(a) != sign3(b); }

// binary_cross_entropy_with_logits of one element as torch evaluates it, (1 - t) x - log_sigmoid(x) with log_sigmoid(x) =
// min(x, 0) - log1p(exp(-|x|)): for a finite x this is max(x, 0) - x t + log1p(exp(-|x|)) term for term (max(x, 0) - x == max(-x, 0)
// exactly), it cannot overflow, and an infinite x lands in the class torch gives (+inf against t = 0: inf; -inf: nan)
__device__ __forceinline__ double bce(double x, bool t) {
    const double log_sigmoid = fmin(x, 0.0) - log1p(exp(-fabs(x)));
    return (t ? 0.0 : 1.0) * x - log_sigmoid;
}

__device__ __forceinline__ double stable_sigmoid(double x) {
    if (x >= 0.0) return 1.0 / (1.0 + exp(-x));
    const double e = exp(x);
    return e / (1.0 + e);  // (a NaN comes here and stays a NaN)
}

__device__ __forceinline__ void add_edge(const float* __restrict__ sdf, int e0, int e1, double& sa, double& sb, int& n) {
    const float a = sdf[e0], b = sdf[e1];
    if (crosses(a, b)) {
        sa += bce((double)a, b > 0.0f);
        sb += bce((double)b, a > 0.0f);
        ++n;
    }
}

__global__ __launch_bounds__(SB_THREADS) void sdf_bce_partials_kernel(const float* __restrict__ sdf, const int* __restrict__ edges, int Ne,
                                                                      Partial* __restrict__ partials) {
    __shared__ double red[SB_WAVES];
    __shared__ int red_n[SB_WAVES];
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef int v2i __attribute__((ext_vector_type(2)));
    const long long pair0 = (long long)blockIdx.x * (SB_PAIRS * SB_THREADS) + threadIdx.x;
    const long long n_pairs = Ne >> 1;  // whole pairs; an odd Ne leaves one row behind them
    v4i rows[SB_PAIRS];
    bool have[SB_PAIRS];
#pragma unroll
    for (int k = 0; k < SB_PAIRS; ++k) {  // every load of the thread in flight before the first gather
        const long long p = pair0 + (long long)k * SB_THREADS;
        have[k] = p < n_pairs;
        rows[k] = have[k] ? __builtin_nontemporal_load(reinterpret_cast<const v4i*>(edges) + p) : v4i{0, 0, 0, 0};
    }
    double sa = 0.0, sb = 0.0;
    int n = 0;
#pragma unroll
    for (int k = 0; k < SB_PAIRS; ++k) {
        if (have[k]) {
            add_edge(sdf, rows[k].x, rows[k].y, sa, sb, n);
            add_edge(sdf, rows[k].z, rows[k].w, sa, sb, n);
        } else if (pair0 + (long long)k * SB_THREADS == n_pairs && (Ne & 1)) {  // the one row behind the last whole pair
            const v2i r = reinterpret_cast<const v2i*>(edges)[Ne - 1];
            add_edge(sdf, r.x, r.y, sa, sb, n);
        }
    }
    const double ta = a3d_block_sum<SB_WAVES>(sa, red);
    const double tb = a3d_block_sum<SB_WAVES>(sb, red);
    const int tn = a3d_block_sum<SB_WAVES>(n, red_n);
    if (threadIdx.x == 0) partials[blockIdx.x] = Partial{ta, tb, (long long)tn};
}

// one work-group: each thread adds a strided share of the partials in ascending order, the group adds the shares in a fixed order
__global__ __launch_bounds__(SB_THREADS) void sdf_bce_finish_kernel(const Partial* __restrict__ partials, int rows, double* __restrict__ state,
                                                                    float* __restrict__ loss) {
    __shared__ double red[SB_WAVES];
    __shared__ long long red_n[SB_WAVES];
    double sa = 0.0, sb = 0.0;
    long long n = 0;
    for (int r = threadIdx.x; r < rows; r += SB_THREADS) {
        const Partial p = partials[r];
        sa += p.sum_a;
        sb += p.sum_b;
        n += p.count;
    }
    const double ta = a3d_block_sum<SB_WAVES>(sa, red);
    const double tb = a3d_block_sum<SB_WAVES>(sb, red);
    const long long tn = a3d_block_sum<SB_WAVES>(n, red_n);
    if (threadIdx.x == 0) {
        const double M = (double)tn;
        loss[0] = (float)(ta / M + tb / M);  // (M == 0: 0 / 0, the mean of nothing)
        state[0] = M;
        state[1] = tn > 0 ? 1.0 / M : 0.0;
    }
}

// one thread per grid vertex: sum over its (edge, side) entries, in list order, of sigmoid(mine) - [other > 0] where the edge crosses
__global__ __launch_bounds__(SB_THREADS) void sdf_bce_bwd_kernel(const float* __restrict__ g_loss, const float* __restrict__ sdf, int Nv,
                                                                 const int* __restrict__ edges, const int* __restrict__ inc_off,
                                                                 const int* __restrict__ inc, const double* __restrict__ state,
                                                                 float* __restrict__ g_sdf) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= Nv) return;
    const float mine = sdf[v];
    const int lo = inc_off[v], hi = inc_off[v + 1];
    double acc = 0.0, sig = 0.0;
    bool have_sig = false;
    for (int i = lo; i < hi; ++i) {
        const int entry = inc[i];
        const float other = sdf[edges[entry ^ 1]];  // (entry = 2 edge + side indexes my end of the flat row list: the other end is entry ^ 1)
        if (crosses(mine, other)) {
            if (!have_sig) {
                sig = stable_sigmoid((double)mine);
                have_sig = true;
            }
            acc += sig - (other > 0.0f ? 1.0 : 0.0);
        }
    }
    g_sdf[v] = (float)(acc * ((double)g_loss[0] * state[1]));
}

}  // namespace

#define SB_CHECK_SIZES() A3D_CHECK_ARG(Nv > 0 && Ne > 0 && Ne < (1 << 30))

extern "C" int a3d_sdf_bce_fwd(const float* sdf, int Nv, const int32_t* all_edges, int Ne, double* partials, double* state, float* loss,
                               a3d_stream_t stream) {
    SB_CHECK_SIZES();
    A3D_CHECK_ARG(sdf && all_edges && partials && state && loss);
    A3D_CHECK_ARG(((uintptr_t)all_edges & 15) == 0 && ((uintptr_t)partials & 7) == 0);
    hipStream_t s = (hipStream_t)stream;
    const int gx = a3d_div_up(Ne, A3D_SDF_BCE_BLOCK_EDGES);
    hipLaunchKernelGGL(sdf_bce_partials_kernel, dim3(gx), dim3(SB_THREADS), 0, s, sdf, all_edges, Ne, (Partial*)partials);
    A3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdf_bce_finish_kernel, dim3(1), dim3(SB_THREADS), 0, s, (const Partial*)partials, gx, state, loss);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_sdf_bce_bwd(const float* g_loss, const float* sdf, int Nv, const int32_t* all_edges, int Ne, const int32_t* inc_off,
                               const int32_t* inc, const double* state, float* g_sdf, a3d_stream_t stream) {
    SB_CHECK_SIZES();
    A3D_CHECK_ARG(g_loss && sdf && all_edges && inc_off && inc && state && g_sdf);
    hipLaunchKernelGGL(sdf_bce_bwd_kernel, dim3(a3d_div_up(Nv, SB_THREADS)), dim3(SB_THREADS), 0, (hipStream_t)stream, g_loss, sdf, Nv, all_edges,
                       inc_off, inc, state, g_sdf);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
