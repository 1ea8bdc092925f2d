// The strided-pixel front end: the memory side of every element-wise launch over an a3d_bsdf_desc (include/a3d_bsdf.h), once.  bsdf.hip
// (the BSDFs, the image loss) and tangent.hip (the shading normal) supply a per-pixel policy and their op / variant rule; the rest is here.
//
// One lane per pixel, A3D_BSDF_TILE = 4 x 256 pixels per work-group: in round `it` lane t takes pixel tile + 256 it + t, so a wave reads 64
// consecutive pixels = 768 contiguous bytes of every contiguous 3-channel input.  The forward keeps everything in registers and stores
// the result once; the backward recomputes the forward's intermediates from the inputs (nothing is saved but the inputs) and writes
// every gradient from the same launch.
// Inputs are base pointer + per-dimension element strides (0 = broadcast), resolved per input to one of three address modes on the host:
// ROWS (contiguous [pixels, C]: offset = pixel * C, no index arithmetic), UNIFORM (constant over the work-group's segment: one offset
// per work-group) or STRIDED (the pixel index is decomposed into the leading dimensions; 32-bit divisions when the pixel count allows).
// Gradients of inputs that are constant over runs of pixels (camera / light position, a constant albedo) are reduced without atomics:
// lane registers over the 4 rounds -> wave (xor butterfly) -> work-group (LDS, fixed order) -> ONE partial row per work-group; a second
// small launch adds the rows of each run in a fixed order.  The sums are carried in DOUBLE (partial rows are doubles).  Bit-identical
// run to run.  A policy whose result is one scalar (the image loss) has it summed the same way.
#pragma once
#include <limits.h>

#include "../../include/a3d_bsdf.h"
#include "a3d_common.h"
#include "bsdf_math.h"

namespace {
namespace px {

using bsdf::V3T;

constexpr int NI = A3D_BSDF_MAX_INPUTS, ND = A3D_BSDF_MAX_DIMS, TILE = A3D_BSDF_TILE, THREADS = 256, ROUNDS = TILE / THREADS;
enum { MODE_ROWS = 0, MODE_UNIFORM = 1, MODE_STRIDED = 2 };

struct In {
    const float* p;
    long long st[ND];
    long long cs;
    float* g;
    int mode, gmode;
};

struct K {
    int variant, ndim, small, any_uniform, any_strided;
    float min_a;
    long long n, seg, bps;
    long long shape[ND];
    In in[NI];
    float* out;
    const float* g_out;
    float* scratch;
};

struct Fin {  // the finishing launch: final[e][c] = sum over rows [e R, (e + 1) R) of rows[.][c], optionally / div
    const double* rows[NI];
    float* final_[NI];
    long long R[NI], ne[NI];
    int C[NI];
    double div;
};

// offset of pixel p in an input, from its leading-dimension strides
__device__ __forceinline__ void index(const K& k, long long p, long long* idx) {
    if (k.small) {
        unsigned r = (unsigned)p;
        for (int d = k.ndim - 1; d > 0; --d) {
            const unsigned s = (unsigned)k.shape[d];
            idx[d] = r % s;
            r /= s;
        }
        idx[0] = r;
    } else {
        long long r = p;
        for (int d = k.ndim - 1; d > 0; --d) {
            idx[d] = r % k.shape[d];
            r /= k.shape[d];
        }
        idx[0] = r;
    }
}

__device__ __forceinline__ long long offset(const K& k, const In& in, const long long* idx) {
    long long o = 0;
    for (int d = 0; d < k.ndim; ++d) o += idx[d] * in.st[d];
    return o;
}

template <typename T>
__device__ __forceinline__ T comp(V3T<T> v, int c) { return c == 0 ? v.x : c == 1 ? v.y : v.z; }

// sum of v over the work-group, in a fixed order (red: 4 doubles of LDS).  Sums are carried in double from the lane to the finishing
// launch: what is left in a reduced gradient is the rounding of the per-pixel terms, not of the summation
__device__ __forceinline__ double block_sum(double v, double* red) { return a3d_block_sum<THREADS / 64>(v, red); }

// The one kernel body.  P is the operator's policy:
//   NIN, cin(i), CO    inputs, channels of input i, channels of the result
//   SUM                the result is one scalar, the mean over all pixels of o[0] (its gradient reaches pixel() as go[0] = g_out / n)
//   pixel<BWD, T>(k, x, go, o, g)    x[i][c] -> o[c] and, BWD, g[i] for the output gradient go[c]
// T: the scalar the per-pixel arithmetic is carried in; the operator's launch picks it.
template <class P, bool BWD, typename T>
__global__ __launch_bounds__(THREADS) void kernel(const K k) {
    constexpr int NIN = P::NIN, CO = P::CO;
    __shared__ double red[4];
    const unsigned bps = (unsigned)k.bps;  // (the grid fits 31 bits, so does this: 32-bit division, once per lane)
    const long long sg = blockIdx.x / bps, blk = blockIdx.x % bps;
    const long long p0 = sg * k.seg;
    long long idx[ND] = {0, 0, 0, 0};
    long long uoff[NIN];
    if (k.any_uniform) {
        index(k, p0, idx);
#pragma unroll
        for (int i = 0; i < NIN; ++i) uoff[i] = offset(k, k.in[i], idx);
    } else {
#pragma unroll
        for (int i = 0; i < NIN; ++i) uoff[i] = 0;
    }
    // (accumulators only where a gradient can be reduced: the double instantiation and the scalar sum; a float backward carries none)
    constexpr bool ACC = BWD && (sizeof(T) == 8 || P::SUM);
    double acc[ACC ? NIN : 1][3];
#pragma unroll
    for (int i = 0; i < (ACC ? NIN : 1); ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.0;
    double lsum = 0.0;
    const T g_scalar = (P::SUM && BWD) ? (T)(k.g_out[0] / (float)k.n) : T(0);

    // (the backwards keep the rounds rolled: unrolled, four rounds of live state do not fit the register file; the forwards and the
    // scalar sum have little state and want their four rounds of loads in flight together)
    constexpr int UNROLL = (P::SUM || !BWD) ? ROUNDS : 1;
#pragma unroll UNROLL
    for (int it = 0; it < ROUNDS; ++it) {
        const long long q = blk * TILE + it * THREADS + threadIdx.x;
        if (q >= k.seg) break;
        const long long p = p0 + q;
        if (k.any_strided) index(k, p, idx);
        T x[NIN][3];
#pragma unroll
        for (int i = 0; i < NIN; ++i) {
            const int C = P::cin(i);
            const In& in = k.in[i];
            if (in.mode == MODE_ROWS) {
                const float* s = in.p + p * C;
#pragma unroll
                for (int c = 0; c < C; ++c) x[i][c] = s[c];
            } else {
                const float* s = in.p + (in.mode == MODE_UNIFORM ? uoff[i] : offset(k, in, idx));
#pragma unroll
                for (int c = 0; c < C; ++c) x[i][c] = s[c * in.cs];
            }
        }
        V3T<T> g[NIN];
#pragma unroll
        for (int i = 0; i < NIN; ++i) g[i] = V3T<T>{T(0), T(0), T(0)};
        T go[3] = {g_scalar, T(0), T(0)};
        if (BWD && !P::SUM) {
#pragma unroll
            for (int c = 0; c < CO; ++c) go[c] = k.g_out[p * CO + c];
        }
        T o[3] = {T(0), T(0), T(0)};
        P::template pixel<BWD, T>(k, x, go, o, g);
        if (P::SUM) lsum += o[0];
        if (!BWD) {
            if (!P::SUM) {
#pragma unroll
                for (int c = 0; c < CO; ++c) k.out[p * CO + c] = (float)o[c];
            }
        } else {
#pragma unroll
            for (int i = 0; i < NIN; ++i) {
                const int C = P::cin(i);
                const In& in = k.in[i];
                if (in.gmode == A3D_BSDF_GRAD_DIRECT) {
#pragma unroll
                    for (int c = 0; c < C; ++c) in.g[p * C + c] = (float)comp(g[i], c);
                } else if (ACC && in.gmode == A3D_BSDF_GRAD_REDUCE) {
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[ACC ? i : 0][c] += comp(g[i], c);
                }
            }
        }
    }
    if (ACC) {
#pragma unroll
        for (int i = 0; i < NIN; ++i) {
            const int C = P::cin(i);
            if (k.in[i].gmode != A3D_BSDF_GRAD_REDUCE) continue;  // (the same in every lane)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double s = block_sum(acc[ACC ? i : 0][c], red);
                if (threadIdx.x == 0) reinterpret_cast<double*>(k.in[i].g)[(long long)blockIdx.x * C + c] = s;
            }
        }
    } else if (P::SUM) {
        const double s = block_sum(lsum, red);
        if (threadIdx.x == 0) reinterpret_cast<double*>(k.scratch)[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(THREADS) void finish_kernel(const Fin f) {
    __shared__ double red[4];
    const int i = blockIdx.y;
    const long long e = blockIdx.x;
    if (!f.rows[i] || e >= f.ne[i]) return;  // (the same in every lane of the work-group)
    const int C = f.C[i];
    const long long R = f.R[i];
    const double* rows = f.rows[i] + e * R * C;
    for (int c = 0; c < C; ++c) {
        double s = 0.0;
        for (long long r = threadIdx.x; r < R; r += THREADS) s += rows[r * C + c];
        s = block_sum(s, red);
        if (threadIdx.x == 0) f.final_[i][e * C + c] = (float)(f.div > 0.0 ? s / f.div : s);
    }
}

// ---- host side
// d >= the returned k are the dimensions inside a run of `run` consecutive pixels; -1 when no boundary between dimensions gives that run
inline int run_dim(const int64_t* shape, int ndim, long long run) {
    long long prod = 1;
    if (run == 1) return ndim;
    for (int d = ndim - 1; d >= 0; --d) {
        prod *= shape[d];
        if (prod == run) return d;
        if (prod > run) return -1;
    }
    return -1;
}

inline bool const_from(const a3d_bsdf_desc* d, int i, int from) {
    for (int j = from; j < d->ndim; ++j)
        if (d->shape[j] > 1 && d->stride[ND * i + j] != 0) return false;
    return true;
}

// the work-groups (= partial rows) of a launch over desc, -1 for a descriptor that is short or has no valid geometry: a3d_*_rows
inline int64_t rows(const a3d_bsdf_desc* desc) {
    if (!desc || desc->size < sizeof(a3d_bsdf_desc)) return -1;
    if (desc->ndim < 1 || desc->ndim > A3D_BSDF_MAX_DIMS || desc->seg < 1) return -1;
    long long n = 1;
    for (int j = 0; j < desc->ndim; ++j) {
        if (desc->shape[j] < 0 || desc->shape[j] > (1ll << 40)) return -1;
        n *= desc->shape[j];
        if (n > (1ll << 40)) return -1;
    }
    if (n % desc->seg) return -1;
    return (n / desc->seg) * ((desc->seg + TILE - 1) / TILE);
}

// the first check of every entry point, before any other field is read: a shorter struct does not have them.  The operator's own op /
// variant rule comes next, then check()
inline int check_size(const a3d_bsdf_desc* d, const char* fn) {
    if (!d) {
        a3d_set_error("%s: invalid argument: desc", fn);
        return A3D_EINVAL;
    }
    if (d->size < sizeof(a3d_bsdf_desc)) {
        a3d_set_error("%s: invalid argument: desc->size %u < sizeof(a3d_bsdf_desc) %zu (a caller built against an older header)", fn, d->size,
                      sizeof(a3d_bsdf_desc));
        return A3D_EINVAL;
    }
    return A3D_OK;
}

// validates everything that can be validated without touching a pointer, for an operator of nin inputs with cin(op, i) channels; fills k
// and *nrows (n == 0: nothing to launch)
inline int check(const a3d_bsdf_desc* d, K& k, const char* fn, int nin, int (*cin)(int op, int i), bool bwd, long long* nrows) {
#define PX_REQUIRE(cond)                                                \
    do {                                                                \
        if (!(cond)) {                                                  \
            a3d_set_error("%s: invalid argument: %s", fn, #cond);       \
            return A3D_EINVAL;                                          \
        }                                                               \
    } while (0)
    PX_REQUIRE(d->ndim >= 1 && d->ndim <= A3D_BSDF_MAX_DIMS);
    long long n = 1;
    for (int j = 0; j < d->ndim; ++j) {
        if (d->shape[j] < 0 || d->shape[j] > (1ll << 40)) {
            a3d_set_error("%s: invalid argument: shape[%d] = %lld", fn, j, (long long)d->shape[j]);
            return A3D_EINVAL;
        }
        n *= d->shape[j];
        PX_REQUIRE(n <= (1ll << 40));
    }
    k.n = n;
    *nrows = 0;
    if (n == 0) return A3D_OK;
    PX_REQUIRE(d->seg >= 1 && n % d->seg == 0);
    const int kseg = run_dim(d->shape, d->ndim, d->seg);
    PX_REQUIRE(kseg >= 0 /* seg must be the product of trailing dimensions */);
    k.seg = d->seg;
    k.bps = (d->seg + TILE - 1) / TILE;
    PX_REQUIRE((n / d->seg) <= INT_MAX / k.bps);
    *nrows = (n / d->seg) * k.bps;
    k.variant = d->variant;
    k.ndim = d->ndim;
    k.small = n < (1ll << 31);
    k.min_a = d->min_roughness * d->min_roughness;
    k.any_uniform = k.any_strided = 0;
    for (int j = 0; j < ND; ++j) k.shape[j] = j < d->ndim ? d->shape[j] : 1;
    for (int i = 0; i < nin; ++i) {
        In& in = k.in[i];
        const int C = cin(d->op, i);
        long long rowstride = C;
        bool rows_mode = d->cstride[i] == 1 || C == 1;
        for (int j = ND - 1; j >= 0; --j) {
            in.st[j] = j < d->ndim ? d->stride[ND * i + j] : 0;
            if (j < d->ndim) {
                if (in.st[j] < 0) {
                    a3d_set_error("%s: invalid argument: stride[%d][%d] = %lld is negative", fn, i, j, (long long)in.st[j]);
                    return A3D_EINVAL;
                }
                if (d->shape[j] > 1 && in.st[j] != rowstride) rows_mode = false;
                rowstride *= d->shape[j];
            }
        }
        PX_REQUIRE(d->cstride[i] >= 0);
        in.p = d->in[i];
        in.cs = d->cstride[i];
        in.mode = rows_mode ? MODE_ROWS : const_from(d, i, kseg) ? MODE_UNIFORM : MODE_STRIDED;
        k.any_uniform |= in.mode == MODE_UNIFORM;
        k.any_strided |= in.mode == MODE_STRIDED;
        in.g = nullptr;
        in.gmode = A3D_BSDF_GRAD_NONE;
        if (!in.p) {
            a3d_set_error("%s: invalid argument: in[%d] is NULL", fn, i);
            return A3D_EINVAL;
        }
        if (bwd) {
            in.gmode = d->g_mode[i];
            in.g = d->g_in[i];
            PX_REQUIRE(in.gmode >= A3D_BSDF_GRAD_NONE && in.gmode <= A3D_BSDF_GRAD_REDUCE);
            if (in.gmode != A3D_BSDF_GRAD_NONE) PX_REQUIRE(d->g_in[i] != nullptr);
            if (in.gmode == A3D_BSDF_GRAD_REDUCE) {
                PX_REQUIRE(d->g_final[i] != nullptr && d->seg_div[i] >= 1 && (n / d->seg) % d->seg_div[i] == 0);
                const int kr = run_dim(d->shape, d->ndim, d->seg * d->seg_div[i]);
                if (kr < 0 || !const_from(d, i, kr)) {
                    a3d_set_error("%s: invalid argument: in[%d] has g_mode A3D_BSDF_GRAD_REDUCE but is not constant over its runs of seg * "
                                  "seg_div[%d] = %lld pixels", fn, i, i, (long long)(d->seg * d->seg_div[i]));
                    return A3D_EINVAL;
                }
            }
        }
    }
    k.out = d->out;
    k.g_out = d->g_out;
    k.scratch = d->scratch;
    if (bwd) PX_REQUIRE(d->g_out != nullptr);
    else PX_REQUIRE(d->out != nullptr);
#undef PX_REQUIRE
    return A3D_OK;
}

// the finishing launch of a backward: every reduced input in one grid (y = input)
inline int finish_grads(const a3d_bsdf_desc* d, const K& k, int nin, int (*cin)(int op, int i), hipStream_t s) {
    Fin f = {};
    long long max_e = 0;
    for (int i = 0; i < nin; ++i) {
        if (k.in[i].gmode != A3D_BSDF_GRAD_REDUCE) continue;
        f.rows[i] = reinterpret_cast<const double*>(d->g_in[i]);
        f.final_[i] = d->g_final[i];
        f.R[i] = d->seg_div[i] * k.bps;
        f.ne[i] = (k.n / k.seg) / d->seg_div[i];
        f.C[i] = cin(d->op, i);
        if (f.ne[i] > max_e) max_e = f.ne[i];
    }
    if (max_e == 0) return A3D_OK;
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)max_e, nin), dim3(THREADS), 0, s, f);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

}  // namespace px
}  // namespace
