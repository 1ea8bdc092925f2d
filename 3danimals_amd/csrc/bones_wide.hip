// estimate_bones on the device for any number of instances: the multi-work-group path behind a3d_estimate_bones (include/a3d.h), taken by
// exactly the calls the one-group eb_kernel (bones.hip) does not take -- N > 32 instances or more than 2^22 points.  The sequence models
// estimate the bones of B x F deformed meshes per iteration (20 x 10 = 200 instances of 5,720 vertices); restated on torch that is ~245
// launches per call.  Same semantics as eb_kernel's phases A-D (reference skinning.py:50-248), cut into launches at every point where a
// work-group needs what other work-groups produce:
//   sums    work-group (instance, slab of A3D_EB_WIDE_SLAB vertices): the slab's coordinate sums in double, plain stores; arms the keys
//   spine   every work-group adds its instance's partial sums in the same fixed order (all get the same centroid bits), scans its slab for
//           the spine ends and publishes each with ONE 64-bit atomicMax / atomicMin of  order(value) << 32 | index  (the maximum carries
//           ~index: the lower index wins a tie either way, as torch.argmax / argmin)
//   radix   one launch per 8-bit pass of the radix select: a work-group first brings the targets' (prefix, remaining rank) up to date from the
//           previous pass's global histograms (redundantly in every work-group; work-group 0 stores the result for the next launch), then
//           histograms the matching values of its slab in LDS and adds the non-empty bins to the global histogram.  All ranks of a stage share
//           its four passes; the Fauna variant runs a second stage over x and z of the vertices with y < threshold, evaluated on the fly
//           (no compaction: the count of the low vertices is the total of its first histogram)
//   feet    margins / centres of the quadrants from the last histograms, then one 64-bit atomicMin per (instance, quadrant) and work-group
//   finish  one thread per bone end: the closed forms of eb_common.h; writes ``nearest`` and clears ``ok`` for an empty quadrant
// Launches: 3 without legs, 8 with legs, 12 for the Fauna variant, plus one memset of the histograms.
// Every dependency between work-groups is a launch boundary: nothing inside a launch waits for another work-group.  Integer atomics only
// (histogram adds, min / max keys) and sums in a fixed order: two calls on the same input give the same bits.
#include "eb_common.h"

#define EBW_THREADS 256
#define EBW_WAVES (EBW_THREADS / 64)
#define EBW_STAGE0_ROWS 4  // histogram rows of the first stage (x: the neighbours of the 95 % and 5 % quantiles; Fauna: y, two of them)
#define EBW_HIST_WORDS (4 * (EBW_STAGE0_ROWS + EB_MAXSEL) * 256)
#define EBW_STATE_WORDS 256  // (prefix, rank) x EB_MAXSEL targets x 4 passes x 2 stages = 192, rounded up
static_assert(EBW_HIST_WORDS + EBW_STATE_WORDS == A3D_EB_WIDE_FIXED_WORDS, "include/a3d.h states the workspace of the wide path");
static_assert(A3D_EB_WIDE_WORDS_PER_INSTANCE == 2 * 6 + 3 && A3D_EB_WIDE_WORDS_PER_SLAB == 2 * 3, "keys + centroid, partial sums");
static_assert(A3D_EB_WIDE_SLAB % EBW_THREADS == 0, "a slab is whole trips of the work-group");

typedef unsigned long long u64;

namespace {

struct EbwParams {
    const float* pos;  // [N, V, 3]
    int N, V, slabs, n_body, n_leg, yplus, fauna;
    float y_q;
    float blend[17], ramp[9];
    int attach[4];
    float* bones;
    int* nearest;
    int* ok;
    int* hist;        // stage 0: [4 passes][EBW_STAGE0_ROWS][256], then stage 1: [4 passes][EB_MAXSEL][256]
    unsigned* state;  // [2 stages][4 passes][EB_MAXSEL][2]: prefix and remaining rank of every target AFTER the pass
    u64* keys;        // [N][6]: spine maximum, spine minimum, the four feet
    double* part;     // [N][slabs][3]
    float* cent;      // [N][3]
};

__device__ __forceinline__ int* ebw_hist(const EbwParams& a, int stage, int pass) {
    return a.hist + (stage == 0 ? pass * EBW_STAGE0_ROWS * 256 : 4 * EBW_STAGE0_ROWS * 256 + pass * EB_MAXSEL * 256);
}
__device__ __forceinline__ unsigned* ebw_state(const EbwParams& a, int stage, int pass) { return a.state + (stage * 4 + pass) * EB_MAXSEL * 2; }
// targets of a stage and targets per coordinate: x -> 4 (Fauna: y -> 2), then x and z among the low vertices -> 6 each
__device__ __forceinline__ int ebw_targets(const EbwParams& a, int stage) { return stage == 0 ? (a.fauna ? 2 : 4) : 12; }
__device__ __forceinline__ int ebw_per_coordinate(const EbwParams& a, int stage) { return stage == 0 ? (a.fauna ? 2 : 4) : 6; }

__device__ __forceinline__ u64 ebw_wave_max(u64 k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 y = __shfl_xor(k, o, 64);
        k = y > k ? y : k;
    }
    return k;
}
__device__ __forceinline__ u64 ebw_wave_min(u64 k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 y = __shfl_xor(k, o, 64);
        k = y < k ? y : k;
    }
    return k;
}
// the key of a value: -0 and +0 compare equal in torch's arg-max / arg-min, so both go in as +0
__device__ __forceinline__ u64 ebw_value_key(float v) { return (u64)eb_key(v + 0.f) << 32; }

// ---- sums: work-group blockIdx.x = n * slabs + s owns the vertices [s * SLAB, min(V, (s + 1) * SLAB)) of instance n, in every launch
__global__ __launch_bounds__(EBW_THREADS) void ebw_sums_kernel(const EbwParams a) {
    __shared__ double s_red[EBW_WAVES];
    const int tid = threadIdx.x, n = blockIdx.x / a.slabs, s = blockIdx.x - n * a.slabs;
    const int v0 = s * A3D_EB_WIDE_SLAB, v1 = min(a.V, v0 + A3D_EB_WIDE_SLAB);
    const float* __restrict__ p = a.pos + (long long)n * a.V * 3;
    double sx = 0., sy = 0., sz = 0.;
    for (int v = v0 + tid; v < v1; v += EBW_THREADS) { sx += (double)p[3 * v]; sy += (double)p[3 * v + 1]; sz += (double)p[3 * v + 2]; }
    sx = a3d_block_sum<EBW_WAVES>(sx, s_red);
    sy = a3d_block_sum<EBW_WAVES>(sy, s_red);
    sz = a3d_block_sum<EBW_WAVES>(sz, s_red);
    if (tid == 0) {
        double* o = a.part + (long long)blockIdx.x * 3;
        o[0] = sx; o[1] = sy; o[2] = sz;
    }
    // the state words of the call: keys to their neutral values (the grid has at least N * 256 threads), ok = 1
    const long long gid = (long long)blockIdx.x * EBW_THREADS + tid;
    if (gid < 6ll * a.N) a.keys[gid] = gid % 6 == 0 ? 0ull : ~0ull;
    if (gid == 0) a.ok[0] = 1;
}

// ---- spine
__global__ __launch_bounds__(EBW_THREADS) void ebw_spine_kernel(const EbwParams a) {
    __shared__ double s_red[EBW_WAVES];
    __shared__ u64 s_key[EBW_WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.x / a.slabs, s = blockIdx.x - n * a.slabs;
    const int v0 = s * A3D_EB_WIDE_SLAB, v1 = min(a.V, v0 + A3D_EB_WIDE_SLAB), V = a.V;
    const float* __restrict__ p = a.pos + (long long)n * V * 3;
    // the instance's partial sums in an order that does not depend on the work-group: thread t adds slabs t, t + 256, .., then the fixed
    // tree of a3d_block_sum
    double c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double acc = 0.;
        for (int j = tid; j < a.slabs; j += EBW_THREADS) acc += a.part[((long long)n * a.slabs + j) * 3 + k];
        c[k] = a3d_block_sum<EBW_WAVES>(acc, s_red);
    }
    const float cy = (float)(c[1] / (double)V);
    if (s == 0 && tid == 0) {
        a.cent[3ll * n] = (float)(c[0] / (double)V); a.cent[3ll * n + 1] = cy; a.cent[3ll * n + 2] = (float)(c[2] / (double)V);
    }
    float hv = -INFINITY, lv = INFINITY;
    unsigned hi = 0xFFFFFFFFu, li = 0xFFFFFFFFu;
    for (int v = v0 + tid; v < v1; v += EBW_THREADS) {  // ascending per thread: strictly better keeps the lowest index
        const float z = p[3 * v + 2];
        float ka = z, kb = z;
        if (a.yplus) {  // z * upper + (-+1e6) * (1 - upper)   (skinning.py:103-107)
            const float up = p[3 * v + 1] > (cy - 0.5f) ? 1.f : 0.f;
            ka = z * up + (-1e6f) * (1.f - up);
            kb = z * up + 1e6f * (1.f - up);
        }
        if (ka > hv) { hv = ka; hi = (unsigned)v; }
        if (kb < lv) { lv = kb; li = (unsigned)v; }
    }
    u64 kmax = hi == 0xFFFFFFFFu ? 0ull : (ebw_value_key(hv) | (0xFFFFFFFFu - hi));
    u64 kmin = li == 0xFFFFFFFFu ? ~0ull : (ebw_value_key(lv) | li);
    kmax = ebw_wave_max(kmax); kmin = ebw_wave_min(kmin);
    if (lane == 0) { s_key[wave][0] = kmax; s_key[wave][1] = kmin; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < EBW_WAVES; ++w) {
            kmax = s_key[w][0] > kmax ? s_key[w][0] : kmax;
            kmin = s_key[w][1] < kmin ? s_key[w][1] : kmin;
        }
        if (kmax != 0ull) atomicMax(a.keys + 6ll * n, kmax);
        if (kmin != ~0ull) atomicMin(a.keys + 6ll * n + 1, kmin);
    }
}

// ---- the select.  Ranks a stage starts from (thread 0): ``count`` values are ranked
__device__ __forceinline__ void ebw_initial_ranks(const EbwParams& a, int stage, int count, int* s_rank) {
    if (stage == 0 && !a.fauna) {
        const EbRanks r95 = eb_ranks_of(0.95f, count), r05 = eb_ranks_of(0.05f, count);
        s_rank[0] = r95.lo; s_rank[1] = r95.hi; s_rank[2] = r05.lo; s_rank[3] = r05.hi;
    } else if (stage == 0) {
        const EbRanks r = eb_ranks_of(a.y_q, count);
        s_rank[0] = r.lo; s_rank[1] = r.hi;
    } else {  // x among the low vertices in slots 0..5, z in slots 6..11: median, 95 %, 5 %
        const EbRanks r50 = eb_ranks_of(0.5f, count), r95 = eb_ranks_of(0.95f, count), r05 = eb_ranks_of(0.05f, count);
        s_rank[0] = r50.lo; s_rank[1] = r50.hi; s_rank[2] = r95.lo; s_rank[3] = r95.hi; s_rank[4] = r05.lo; s_rank[5] = r05.hi;
        for (int k = 0; k < 6; ++k) s_rank[6 + k] = s_rank[k];
    }
}

// s_rep[t] = the first target of t's coordinate whose prefix agrees with t's: targets that agree so far (the two neighbours a quantile
// interpolates between nearly always do, to the last pass) share one histogram, the one of that target.  (thread t)
__device__ __forceinline__ int ebw_representative(const unsigned* s_prefix, int t, int mg) {
    int rep = t;
    for (int u = t - 1; u >= (t / mg) * mg; --u)
        if (s_prefix[u] == s_prefix[t]) rep = u;
    return rep;
}

// Brings s_prefix / s_rank of the stage's targets to their values AFTER pass q, from the values after pass q - 1 (work-group 0 of the
// launch before stored them; before pass 0: the initial ranks) and the global histograms of pass q (complete: an earlier launch).  Every
// work-group computes the same; work-group 0 stores the result for the launches behind.  All threads of the work-group call it.
__device__ __forceinline__ void ebw_advance(const EbwParams& a, int stage, int q, int count, int* s_rank, unsigned* s_prefix, int* s_rep) {
    const int tid = threadIdx.x, T = ebw_targets(a, stage), mg = ebw_per_coordinate(a, stage);
    __syncthreads();  // (whoever read s_prefix before is done)
    if (q == 0) {
        if (tid == 0) ebw_initial_ranks(a, stage, count, s_rank);
        if (tid < T) s_prefix[tid] = 0u;
    } else if (tid < T) {
        const unsigned* st = ebw_state(a, stage, q - 1);
        s_prefix[tid] = st[2 * tid]; s_rank[tid] = (int)st[2 * tid + 1];
    }
    __syncthreads();
    if (tid < T) s_rep[tid] = ebw_representative(s_prefix, tid, mg);
    __syncthreads();
    const int* h = ebw_hist(a, stage, q);
    for (int t = tid >> 6; t < T; t += EBW_WAVES) {  // one wave per target
        const unsigned pre = s_prefix[t];
        int b = 0, rest = 0;
        const bool found = eb_find_bin(h + s_rep[t] * 256, s_rank[t], &b, &rest);
        if (found) { s_rank[t] = rest; s_prefix[t] = (pre << 8) | (unsigned)b; }
        if (__ballot(found) == 0ull && (tid & 63) == 0) s_prefix[t] = pre << 8;  // (fewer values than the rank asks for: nothing was ranked)
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < T) {
        unsigned* st = ebw_state(a, stage, q);
        st[2 * tid] = s_prefix[tid]; st[2 * tid + 1] = (unsigned)s_rank[tid];
    }
}

// the number of vertices below the y threshold: the total of the first histogram of the second stage (in every lane)
__device__ __forceinline__ int ebw_low_count(const EbwParams& a) {
    const int4 c = reinterpret_cast<const int4*>(ebw_hist(a, 1, 0))[threadIdx.x & 63];
    return a3d_group_sum<64>(c.x + c.y + c.z + c.w);
}

__global__ __launch_bounds__(EBW_THREADS) void ebw_radix_kernel(const EbwParams a, int stage, int pass) {
    __shared__ __attribute__((aligned(16))) int s_hist[EB_MAXSEL][256];
    __shared__ int s_rank[EB_MAXSEL], s_rep[EB_MAXSEL];
    __shared__ unsigned s_prefix[EB_MAXSEL];
    __shared__ int s_nu[2], s_urep[2][EB_MAXGROUP];
    __shared__ unsigned s_upre[2][EB_MAXGROUP];
    __shared__ float s_thr;
    const int tid = threadIdx.x, n = blockIdx.x / a.slabs, s = blockIdx.x - n * a.slabs;
    const int v0 = s * A3D_EB_WIDE_SLAB, v1 = min(a.V, v0 + A3D_EB_WIDE_SLAB), total = a.N * a.V;
    const float* __restrict__ p = a.pos + (long long)n * a.V * 3;
    const int T = ebw_targets(a, stage), mg = ebw_per_coordinate(a, stage), NG = T / mg;
    for (int i = tid; i < T * 256; i += EBW_THREADS) (&s_hist[0][0])[i] = 0;
    float thr = 0.f;
    if (stage == 1) {  // the y threshold: the first stage's result (its last pass is evaluated by the first launch of this stage)
        if (pass == 0) {
            ebw_advance(a, 0, 3, total, s_rank, s_prefix, s_rep);
        } else {
            if (tid < 2) s_prefix[tid] = ebw_state(a, 0, 3)[2 * tid];
        }
        __syncthreads();
        if (tid == 0) s_thr = eb_lerp(eb_unkey(s_prefix[0]), eb_unkey(s_prefix[1]), eb_ranks_of(a.y_q, total).w);
        __syncthreads();
        thr = s_thr;
    }
    if (pass > 0) {
        ebw_advance(a, stage, pass - 1, stage == 1 ? ebw_low_count(a) : total, s_rank, s_prefix, s_rep);
    } else {
        __syncthreads();
        if (tid < T) s_prefix[tid] = 0u;
    }
    __syncthreads();
    if (tid < NG) {  // the distinct prefixes of a coordinate and the targets that own their histograms
        int nu = 0;
        for (int t = tid * mg; t < (tid + 1) * mg; ++t)
            if (ebw_representative(s_prefix, t, mg) == t) { s_upre[tid][nu] = s_prefix[t]; s_urep[tid][nu] = t; ++nu; }
        s_nu[tid] = nu;
    }
    __syncthreads();
    {
        const int shift = 24 - 8 * pass;
        unsigned upre[2][EB_MAXGROUP];
        int urep[2][EB_MAXGROUP], nu[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            nu[g] = g < NG ? s_nu[g] : 0;
#pragma unroll
            for (int u = 0; u < EB_MAXGROUP; ++u) {
                const bool have = u < nu[g];
                upre[g][u] = have ? s_upre[g][u] : 0xFFFFFFFFu;
                urep[g][u] = have ? s_urep[g][u] : 0;
            }
        }
        for (int v = v0 + tid; v < v1; v += EBW_THREADS) {
            const float x = p[3 * v], y = p[3 * v + 1], z = p[3 * v + 2];
            if (stage == 1 && !(y < thr)) continue;
            const float val[2] = {stage == 1 ? x : (a.fauna ? y : x), z};
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                if (g >= NG) break;
                const unsigned k = eb_key(val[g]), hi = pass == 0 ? 0u : k >> (shift + 8), digit = (k >> shift) & 255u;
#pragma unroll
                for (int u = 0; u < EB_MAXGROUP; ++u) {
                    if (u >= nu[g]) break;  // (uniform: usually one to three distinct prefixes)
                    if (hi == upre[g][u]) atomicAdd(&s_hist[urep[g][u]][digit], 1);
                }
            }
        }
    }
    __syncthreads();
    int* h = ebw_hist(a, stage, pass);
    for (int i = tid; i < T * 256; i += EBW_THREADS) {
        const int c = (&s_hist[0][0])[i];
        if (c) atomicAdd(h + i, c);
    }
}

// ---- feet
__global__ __launch_bounds__(EBW_THREADS) void ebw_feet_kernel(const EbwParams a) {
    __shared__ int s_rank[EB_MAXSEL], s_rep[EB_MAXSEL];
    __shared__ unsigned s_prefix[EB_MAXSEL];
    __shared__ float s_q[4];
    __shared__ u64 s_key[EBW_WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.x / a.slabs, s = blockIdx.x - n * a.slabs;
    const int v0 = s * A3D_EB_WIDE_SLAB, v1 = min(a.V, v0 + A3D_EB_WIDE_SLAB), total = a.N * a.V;
    const float* __restrict__ p = a.pos + (long long)n * a.V * 3;
    if (!a.fauna) {
        ebw_advance(a, 0, 3, total, s_rank, s_prefix, s_rep);
        if (tid == 0) {
            const float q95 = eb_lerp(eb_unkey(s_prefix[0]), eb_unkey(s_prefix[1]), eb_ranks_of(0.95f, total).w);
            const float q05 = eb_lerp(eb_unkey(s_prefix[2]), eb_unkey(s_prefix[3]), eb_ranks_of(0.05f, total).w);
            s_q[0] = (q95 - q05) * 0.2f;  // margin
        }
    } else {
        const int nlow = ebw_low_count(a);
        ebw_advance(a, 1, 3, nlow, s_rank, s_prefix, s_rep);
        if (tid == 0) {
            const float w[3] = {eb_ranks_of(0.5f, nlow).w, eb_ranks_of(0.95f, nlow).w, eb_ranks_of(0.05f, nlow).w};
            float q[2][3];
            for (int c = 0; c < 2; ++c)
                for (int k = 0; k < 3; ++k) q[c][k] = eb_lerp(eb_unkey(s_prefix[6 * c + 2 * k]), eb_unkey(s_prefix[6 * c + 2 * k + 1]), w[k]);
            s_q[0] = q[0][0]; s_q[1] = q[1][0];                                      // x0, z0 (medians)
            s_q[2] = (q[0][1] - q[0][2]) * 0.2f; s_q[3] = (q[1][1] - q[1][2]) * 0.2f;  // mx, mz
            if (nlow == 0 && blockIdx.x == 0) a.ok[0] = 0;  // (torch.quantile of an empty tensor raises in the reference)
        }
    }
    __syncthreads();
    float bv[4];
    unsigned bi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { bv[k] = INFINITY; bi[k] = 0xFFFFFFFFu; }
    for (int v = v0 + tid; v < v1; v += EBW_THREADS) {
        const float x = p[3 * v], y = p[3 * v + 1], z = p[3 * v + 2];
        bool in[4];
        if (!a.fauna) {
            const float m = s_q[0];
            in[0] = x > m && z > 0.f; in[1] = x > m && z < 0.f; in[2] = x < -m && z < 0.f; in[3] = x < -m && z > 0.f;
        } else {
            const float x0 = s_q[0], z0 = s_q[1], mx = s_q[2], mz = s_q[3];
            in[0] = (x - x0 > mx) && (z - z0 > mz); in[1] = (x - x0 > mx) && (z < z0);
            in[2] = (x - x0 < -mx) && (z < z0); in[3] = (x - x0 < -mx) && (z - z0 > mz);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (in[k] && y < bv[k]) { bv[k] = y; bi[k] = (unsigned)v; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        u64 key = bi[k] == 0xFFFFFFFFu ? ~0ull : (ebw_value_key(bv[k]) | bi[k]);
        key = ebw_wave_min(key);
        if (lane == 0) s_key[wave][k] = key;
    }
    __syncthreads();
    if (tid < 4) {
        u64 key = s_key[0][tid];
        for (int w = 1; w < EBW_WAVES; ++w) key = s_key[w][tid] < key ? s_key[w][tid] : key;
        if (key != ~0ull) atomicMin(a.keys + 6ll * n + 2 + tid, key);
    }
}

// ---- finish: one thread per bone end
__global__ __launch_bounds__(EBW_THREADS) void ebw_finish_kernel(const EbwParams a) {
    __shared__ float s_blend[17], s_ramp[9];
    __shared__ int s_attach[4];
    const int tid = threadIdx.x, N = a.N, V = a.V, K = a.n_body + 4 * a.n_leg;
    if (tid < 17) s_blend[tid] = a.blend[tid];
    if (tid < 9) s_ramp[tid] = a.ramp[tid];
    __syncthreads();
    auto index_of = [&](u64 key, bool inverted) {  // (a key nobody lowered / raised: vertex 0, like arg-min over all-inf)
        const unsigned lo = (unsigned)(key & 0xFFFFFFFFull), i = inverted ? 0xFFFFFFFFu - lo : lo;
        return i < (unsigned)V ? (int)i : -1;
    };
    auto spine_of = [&](int n) {
        EbSpine s;
        s.p = a.pos + (long long)n * V * 3;
        s.va = max(index_of(a.keys[6ll * n], true), 0); s.vb = max(index_of(a.keys[6ll * n + 1], false), 0);
        s.cy = a.cent[3ll * n + 1]; s.cz = a.cent[3ll * n + 2];
        s.n_body = a.n_body; s.n_leg = a.n_leg; s.blend = s_blend;
        return s;
    };
    if (a.n_leg > 0) {
        if (tid < 2) {  // attachment joints (instance 0): nearest body bone end in z to the foot, first index on ties
            int att = a.attach[tid];
            if (att < 0) att = eb_nearest_body_bone(spine_of(0), a.pos[3 * max(index_of(a.keys[2 + tid], false), 0) + 2]);
            s_attach[tid] = att;
        }
        __syncthreads();
        if (tid == 0) {
            s_attach[2] = a.attach[2] < 0 ? s_attach[1] : a.attach[2];
            s_attach[3] = a.attach[3] < 0 ? s_attach[0] : a.attach[3];
            if (blockIdx.x == 0) { a.nearest[0] = s_attach[0]; a.nearest[1] = s_attach[1]; }
        }
        __syncthreads();
    }
    const long long idx = (long long)blockIdx.x * EBW_THREADS + tid;
    if (idx >= 2ll * N * K) return;
    const int n = (int)(idx / (2 * K)), r = (int)(idx - (long long)n * 2 * K), bone = r >> 1, e = r & 1;
    const EbSpine s = spine_of(n);
    float o[3];
    if (bone < a.n_body) {
        eb_body_end(s, bone, e, o);
    } else {
        const int l = (bone - a.n_body) / a.n_leg, i = (bone - a.n_body) - l * a.n_leg;
        const int foot = index_of(a.keys[6ll * n + 2 + l], false);
        if (foot < 0) a.ok[0] = 0;  // an empty quadrant (the same value from every writer)
        eb_leg_end(s, s.p + 3 * max(foot, 0), s_attach[l], s_ramp, i, e, o);
    }
    float* out = a.bones + ((long long)n * K + bone) * 6 + 3 * e;
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
}

}  // namespace

// the launches of a validated wide call (a3d_estimate_bones, bones.hip)
int eb_wide_launch(const a3d_estimate_bones_args* args, hipStream_t stream) {
    EbwParams p;
    p.pos = args->pos; p.N = args->N; p.V = args->V; p.slabs = a3d_div_up(args->V, A3D_EB_WIDE_SLAB);
    p.n_body = args->n_body; p.n_leg = args->n_leg; p.yplus = args->body_mode_y_plus; p.fauna = args->use_y_threshold; p.y_q = args->y_threshold;
    for (int i = 0; i < 17; ++i) p.blend[i] = args->blend[i];
    for (int i = 0; i < 9; ++i) p.ramp[i] = args->ramp[i];
    for (int i = 0; i < 4; ++i) p.attach[i] = args->attach[i];
    p.bones = args->bones; p.nearest = args->nearest; p.ok = args->ok;
    // the workspace, A3D_EB_WIDE_WORKSPACE_WORDS(N, V) 4-byte words: histograms | state | keys | partial sums | centroids
    uint32_t* w = reinterpret_cast<uint32_t*>(args->workspace);
    p.hist = reinterpret_cast<int*>(w);
    p.state = w + EBW_HIST_WORDS;
    p.keys = reinterpret_cast<u64*>(w + A3D_EB_WIDE_FIXED_WORDS);
    p.part = reinterpret_cast<double*>(w + A3D_EB_WIDE_FIXED_WORDS + 12ll * p.N);
    p.cent = reinterpret_cast<float*>(w + A3D_EB_WIDE_FIXED_WORDS + 12ll * p.N + 6ll * p.N * p.slabs);
    const dim3 grid(p.N * p.slabs), block(EBW_THREADS);
    if (p.n_leg > 0) A3D_HIP(hipMemsetAsync(p.hist, 0, sizeof(int) * EBW_HIST_WORDS, stream));
    hipLaunchKernelGGL(ebw_sums_kernel, grid, block, 0, stream, p);
    A3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(ebw_spine_kernel, grid, block, 0, stream, p);
    A3D_LAUNCH_CHECK();
    if (p.n_leg > 0) {
        for (int stage = 0; stage < (p.fauna ? 2 : 1); ++stage)
            for (int pass = 0; pass < 4; ++pass) {
                hipLaunchKernelGGL(ebw_radix_kernel, grid, block, 0, stream, p, stage, pass);
                A3D_LAUNCH_CHECK();
            }
        hipLaunchKernelGGL(ebw_feet_kernel, grid, block, 0, stream, p);
        A3D_LAUNCH_CHECK();
    }
    const int K = p.n_body + 4 * p.n_leg;
    hipLaunchKernelGGL(ebw_finish_kernel, dim3(a3d_div_up(2ll * p.N * K, EBW_THREADS)), block, 0, stream, p);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
