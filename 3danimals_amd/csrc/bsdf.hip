// Shading BSDFs and the HDR image loss on gfx950 (include/a3d_bsdf.h): lambert, frostbite_diffuse, pbr_specular, pbr_bsdf and image_loss
// of the reference's renderutils (ops.py:244-386, 476-498), one fused launch forward and one backward per call.  The per-pixel arithmetic
// and its hand-written derivatives are bsdf_math.h; this file is the memory side.
//
// One lane per pixel, A3D_BSDF_TILE = 4 x 256 pixels per work-group: in round `it` lane t takes pixel tile + 256 it + t, so a wave reads 64
// consecutive pixels = 768 contiguous bytes of every contiguous 3-channel input.  The forward keeps everything in registers and stores
// the colour once; the backward recomputes the forward's intermediates from the inputs (nothing is saved but the inputs) and writes
// every gradient from the same launch.
// Inputs are base pointer + per-dimension element strides (0 = broadcast), resolved per input to one of three address modes on the host:
// ROWS (contiguous [pixels, C]: offset = pixel * C, no index arithmetic), UNIFORM (constant over the work-group's segment: one offset
// per work-group) or STRIDED (the pixel index is decomposed into the leading dimensions; 32-bit divisions when the pixel count allows).
// Gradients of inputs that are constant over runs of pixels (camera / light position, a constant albedo) are reduced without atomics:
// lane registers over the 4 rounds -> wave (xor butterfly) -> work-group (LDS, fixed order) -> ONE partial row per work-group; a second
// small launch adds the rows of each run in a fixed order.  The sums are carried in DOUBLE (partial rows are doubles).  Bit-identical run to run.  image_loss forward sums its scalar the same way.
#include <limits.h>

#include "../../include/a3d_bsdf.h"
#include "a3d_common.h"
#include "bsdf_math.h"

namespace {

using bsdf::V3T;

constexpr int NI = A3D_BSDF_MAX_INPUTS, ND = A3D_BSDF_MAX_DIMS, TILE = A3D_BSDF_TILE, THREADS = 256, ROUNDS = TILE / THREADS;
enum { MODE_ROWS = 0, MODE_UNIFORM = 1, MODE_STRIDED = 2 };

constexpr int op_nin(int op) { return op == A3D_BSDF_LAMBERT ? 2 : op == A3D_BSDF_FROSTBITE ? 4 : op == A3D_BSDF_PBR_SPECULAR ? 5 : op == A3D_BSDF_PBR ? 6 : 2; }
constexpr int op_cin(int op, int i) {
    return op == A3D_BSDF_IMAGE_LOSS ? 1 : (op == A3D_BSDF_FROSTBITE && i == 3) ? 1 : (op == A3D_BSDF_PBR_SPECULAR && i == 4) ? 1 : 3;
}
constexpr int op_cout(int op) { return (op == A3D_BSDF_PBR_SPECULAR || op == A3D_BSDF_PBR) ? 3 : 1; }

struct BsdfIn {
    const float* p;
    long long st[ND];
    long long cs;
    float* g;
    int mode, gmode;
};

struct BsdfK {
    int variant, ndim, small, any_uniform, any_strided;
    float min_a;
    long long n, seg, bps;
    long long shape[ND];
    BsdfIn in[NI];
    float* out;
    const float* g_out;
    float* scratch;
};

struct BsdfFin {  // the finishing launch: final[e][c] = sum over rows [e R, (e + 1) R) of rows[.][c], optionally / div
    const double* rows[NI];
    float* final_[NI];
    long long R[NI], ne[NI];
    int C[NI];
    double div;
};

// offset of pixel p in an input, from its leading-dimension strides
__device__ __forceinline__ void bsdf_index(const BsdfK& k, long long p, long long* idx) {
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

__device__ __forceinline__ long long bsdf_offset(const BsdfK& k, const BsdfIn& in, const long long* idx) {
    long long o = 0;
    for (int d = 0; d < k.ndim; ++d) o += idx[d] * in.st[d];
    return o;
}

template <typename T>
__device__ __forceinline__ T comp(V3T<T> v, int c) { return c == 0 ? v.x : c == 1 ? v.y : v.z; }

// sum of v over the work-group, in a fixed order (red: 4 doubles of LDS).  Sums are carried in double from the lane to the finishing
// launch: what is left in a reduced gradient is the rounding of the per-pixel terms, not of the summation
__device__ __forceinline__ double bsdf_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// T: the scalar the per-pixel arithmetic is carried in.  float, except in the backward of a call that reduces a gradient over pixels
// (a [B,1,1,3] camera): there it is double, so that the few numbers such a gradient consists of carry the rounding of the float32
// INPUTS only -- two float32 evaluations of a sum of thousands of ill-conditioned terms otherwise differ by a factor either way.
template <int OP, bool BWD, typename T>
__global__ __launch_bounds__(THREADS) void bsdf_kernel(const BsdfK k) {
    constexpr int NIN = op_nin(OP), CO = op_cout(OP);
    __shared__ double red[4];
    const unsigned bps = (unsigned)k.bps;  // (the grid fits 31 bits, so does this: 32-bit division, once per lane)
    const long long sg = blockIdx.x / bps, blk = blockIdx.x % bps;
    const long long p0 = sg * k.seg;
    long long idx[ND] = {0, 0, 0, 0};
    long long uoff[NIN];
    if (k.any_uniform) {
        bsdf_index(k, p0, idx);
#pragma unroll
        for (int i = 0; i < NIN; ++i) uoff[i] = bsdf_offset(k, k.in[i], idx);
    } else {
#pragma unroll
        for (int i = 0; i < NIN; ++i) uoff[i] = 0;
    }
    // (accumulators only where a gradient can be reduced: the double instantiation -- bsdf_launch picks it exactly then -- and the image
    // loss; the float BSDF backward carries none)
    constexpr bool ACC = BWD && (sizeof(T) == 8 || OP == A3D_BSDF_IMAGE_LOSS);
    double acc[ACC ? NIN : 1][3];
#pragma unroll
    for (int i = 0; i < (ACC ? NIN : 1); ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.0;
    double lsum = 0.0;
    const T g_scalar = (OP == A3D_BSDF_IMAGE_LOSS && BWD) ? (T)(k.g_out[0] / (float)k.n) : T(0);

    // (the BSDF backwards keep the rounds rolled: unrolled, four rounds of live state do not fit the register file; the forwards and the
    // image loss have little state and want their four rounds of loads in flight together)
    constexpr int UNROLL = (OP == A3D_BSDF_IMAGE_LOSS || !BWD) ? ROUNDS : 1;
#pragma unroll UNROLL
    for (int it = 0; it < ROUNDS; ++it) {
        const long long q = blk * TILE + it * THREADS + threadIdx.x;
        if (q >= k.seg) break;
        const long long p = p0 + q;
        if (k.any_strided) bsdf_index(k, p, idx);
        T x[NIN][3];
#pragma unroll
        for (int i = 0; i < NIN; ++i) {
            const int C = op_cin(OP, i);
            const BsdfIn& in = k.in[i];
            if (in.mode == MODE_ROWS) {
                const float* s = in.p + p * C;
#pragma unroll
                for (int c = 0; c < C; ++c) x[i][c] = s[c];
            } else {
                const float* s = in.p + (in.mode == MODE_UNIFORM ? uoff[i] : bsdf_offset(k, in, idx));
#pragma unroll
                for (int c = 0; c < C; ++c) x[i][c] = s[c * in.cs];
            }
        }
        V3T<T> g[NIN];
#pragma unroll
        for (int i = 0; i < NIN; ++i) g[i] = V3T<T>{T(0), T(0), T(0)};
        T go[3] = {T(0), T(0), T(0)};
        if (BWD && OP != A3D_BSDF_IMAGE_LOSS) {
#pragma unroll
            for (int c = 0; c < CO; ++c) go[c] = k.g_out[p * CO + c];
        }
        T o[3] = {T(0), T(0), T(0)};
        auto V = [&](int i) { return V3T<T>{x[i][0], x[i][1], x[i][2]}; };
        const T min_a = (T)k.min_a;
        if constexpr (OP == A3D_BSDF_LAMBERT) {
            o[0] = bsdf::lambert_fwd(V(0), V(1));
            if (BWD) bsdf::lambert_bwd(V(0), V(1), go[0], g[0], g[1]);
        } else if constexpr (OP == A3D_BSDF_FROSTBITE) {
            o[0] = bsdf::frostbite<BWD>(V(0), V(1), V(2), x[3][0], go[0], g[0], g[1], g[2], g[3].x);
        } else if constexpr (OP == A3D_BSDF_PBR_SPECULAR) {
            const V3T<T> r = bsdf::pbr_specular<BWD>(V(0), V(1), V(2), V(3), x[4][0], min_a, V3T<T>{go[0], go[1], go[2]}, g[0], g[1], g[2], g[3], g[4].x);
            o[0] = r.x; o[1] = r.y; o[2] = r.z;
        } else if constexpr (OP == A3D_BSDF_PBR) {
            const V3T<T> r = bsdf::pbr_bsdf<BWD>(V(0), V(1), V(2), V(3), V(4), V(5), min_a, k.variant, V3T<T>{go[0], go[1], go[2]}, g[0], g[1], g[2],
                                             g[3], g[4], g[5]);
            o[0] = r.x; o[1] = r.y; o[2] = r.z;
        } else {
            T da, db;
            lsum += bsdf::image_loss(x[0][0], x[1][0], k.variant & 3, k.variant >> 2, da, db);
            g[0].x = g_scalar * da;
            g[1].x = g_scalar * db;
        }
        if (!BWD) {
            if (OP != A3D_BSDF_IMAGE_LOSS) {
#pragma unroll
                for (int c = 0; c < CO; ++c) k.out[p * CO + c] = (float)o[c];
            }
        } else {
#pragma unroll
            for (int i = 0; i < NIN; ++i) {
                const int C = op_cin(OP, i);
                const BsdfIn& in = k.in[i];
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
            const int C = op_cin(OP, i);
            if (k.in[i].gmode != A3D_BSDF_GRAD_REDUCE) continue;  // (the same in every lane)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double s = bsdf_block_sum(acc[ACC ? i : 0][c], red);
                if (threadIdx.x == 0) reinterpret_cast<double*>(k.in[i].g)[(long long)blockIdx.x * C + c] = s;
            }
        }
    } else if (OP == A3D_BSDF_IMAGE_LOSS) {
        const double s = bsdf_block_sum(lsum, red);
        if (threadIdx.x == 0) reinterpret_cast<double*>(k.scratch)[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(THREADS) void bsdf_finish_kernel(const BsdfFin f) {
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
        s = bsdf_block_sum(s, red);
        if (threadIdx.x == 0) f.final_[i][e * C + c] = (float)(f.div > 0.0 ? s / f.div : s);
    }
}

// ---- host side
// d >= the returned k are the dimensions inside a run of `run` consecutive pixels; -1 when no boundary between dimensions gives that run
int bsdf_run_dim(const int64_t* shape, int ndim, long long run) {
    long long prod = 1;
    if (run == 1) return ndim;
    for (int d = ndim - 1; d >= 0; --d) {
        prod *= shape[d];
        if (prod == run) return d;
        if (prod > run) return -1;
    }
    return -1;
}

bool bsdf_const_from(const a3d_bsdf_desc* d, int i, int from) {
    for (int j = from; j < d->ndim; ++j)
        if (d->shape[j] > 1 && d->stride[ND * i + j] != 0) return false;
    return true;
}

// image_loss over two contiguous, 16-byte aligned images of n = 4 m elements, no gradient reduced: 16 bytes per lane and load, four
// loads per input in flight (the generic kernel's one float per lane and load reaches a quarter of the probe's bandwidth; the torch
// twin of plain l1 / mse is two or three streaming launches and was faster).  Work-group b covers elements [4 TILE b, 4 TILE (b + 1)).
template <bool BWD>
__global__ __launch_bounds__(THREADS) void loss_rows_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n4, int variant,
                                                            const float* g_out, double n, float* ga, float* gb, double* scratch) {
    __shared__ double red[4];
    const float gs = BWD ? g_out[0] / (float)n : 0.f;
    double lsum = 0.0;
#pragma unroll
    for (int it = 0; it < ROUNDS; ++it) {
        const long long q = ((long long)blockIdx.x * ROUNDS + it) * THREADS + threadIdx.x;
        if (q >= n4) break;
        const float4 va = reinterpret_cast<const float4*>(a)[q], vb = reinterpret_cast<const float4*>(b)[q];
        const float xa[4] = {va.x, va.y, va.z, va.w}, xb[4] = {vb.x, vb.y, vb.z, vb.w};
        float da[4], db[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) lsum += bsdf::image_loss(xa[c], xb[c], variant & 3, variant >> 2, da[c], db[c]);
        if (BWD) {
            if (ga) reinterpret_cast<float4*>(ga)[q] = make_float4(gs * da[0], gs * da[1], gs * da[2], gs * da[3]);
            if (gb) reinterpret_cast<float4*>(gb)[q] = make_float4(gs * db[0], gs * db[1], gs * db[2], gs * db[3]);
        }
    }
    if (!BWD) {
        const double s = bsdf_block_sum(lsum, red);
        if (threadIdx.x == 0) scratch[blockIdx.x] = s;
    }
}

// the fast form applies: both inputs ROWS, everything 16-byte aligned, n a multiple of 4, no reduced gradient
bool loss_rows_ok(const a3d_bsdf_desc* d, const BsdfK& k, bool bwd) {
    if (k.n % 4 || k.in[0].mode != MODE_ROWS || k.in[1].mode != MODE_ROWS) return false;
    uintptr_t bits = (uintptr_t)d->in[0] | (uintptr_t)d->in[1];
    if (bwd)
        for (int i = 0; i < 2; ++i) {
            if (k.in[i].gmode == A3D_BSDF_GRAD_REDUCE) return false;
            if (k.in[i].gmode == A3D_BSDF_GRAD_DIRECT) bits |= (uintptr_t)d->g_in[i];
        }
    return (bits & 15) == 0;
}

// validates everything that can be validated without touching a pointer; fills k (n == 0: nothing to launch)
int bsdf_check(const a3d_bsdf_desc* d, BsdfK& k, const char* fn, bool loss, bool bwd, long long* rows) {
    if (!d) {
        a3d_set_error("%s: invalid argument: desc", fn);
        return A3D_EINVAL;
    }
    if (d->size < sizeof(a3d_bsdf_desc)) {  // (before any other field is read: a shorter struct does not have them)
        a3d_set_error("%s: invalid argument: desc->size %u < sizeof(a3d_bsdf_desc) %zu (a caller built against an older header)", fn, d->size,
                      sizeof(a3d_bsdf_desc));
        return A3D_EINVAL;
    }
#define BSDF_REQUIRE(cond)                                              \
    do {                                                                \
        if (!(cond)) {                                                  \
            a3d_set_error("%s: invalid argument: %s", fn, #cond);       \
            return A3D_EINVAL;                                          \
        }                                                               \
    } while (0)
    if (loss) {
        if (d->op != A3D_BSDF_IMAGE_LOSS || d->variant < 0 || d->variant > 7) {
            a3d_set_error("%s: invalid argument: op %d / variant %d: op must be A3D_BSDF_IMAGE_LOSS, variant loss + 4 * tonemap in 0 .. 7", fn,
                          d->op, d->variant);
            return A3D_EINVAL;
        }
    } else if (d->op < A3D_BSDF_LAMBERT || d->op > A3D_BSDF_PBR || (d->op == A3D_BSDF_PBR && (d->variant < 0 || d->variant > 1))) {
        a3d_set_error("%s: invalid argument: unknown op %d / variant %d", fn, d->op, d->variant);
        return A3D_EINVAL;
    }
    BSDF_REQUIRE(d->ndim >= 1 && d->ndim <= A3D_BSDF_MAX_DIMS);
    long long n = 1;
    for (int j = 0; j < d->ndim; ++j) {
        if (d->shape[j] < 0 || d->shape[j] > (1ll << 40)) {
            a3d_set_error("%s: invalid argument: shape[%d] = %lld", fn, j, (long long)d->shape[j]);
            return A3D_EINVAL;
        }
        n *= d->shape[j];
        BSDF_REQUIRE(n <= (1ll << 40));
    }
    k.n = n;
    *rows = 0;
    if (n == 0) return A3D_OK;
    BSDF_REQUIRE(d->seg >= 1 && n % d->seg == 0);
    const int kseg = bsdf_run_dim(d->shape, d->ndim, d->seg);
    BSDF_REQUIRE(kseg >= 0 /* seg must be the product of trailing dimensions */);
    k.seg = d->seg;
    k.bps = (d->seg + TILE - 1) / TILE;
    BSDF_REQUIRE((n / d->seg) <= INT_MAX / k.bps);
    *rows = (n / d->seg) * k.bps;
    k.variant = d->variant;
    k.ndim = d->ndim;
    k.small = n < (1ll << 31);
    k.min_a = d->min_roughness * d->min_roughness;
    k.any_uniform = k.any_strided = 0;
    for (int j = 0; j < ND; ++j) k.shape[j] = j < d->ndim ? d->shape[j] : 1;
    const int nin = op_nin(d->op);
    for (int i = 0; i < nin; ++i) {
        BsdfIn& in = k.in[i];
        const int C = d->op == A3D_BSDF_IMAGE_LOSS ? 1 : op_cin(d->op, i);
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
        BSDF_REQUIRE(d->cstride[i] >= 0);
        in.p = d->in[i];
        in.cs = d->cstride[i];
        in.mode = rows_mode ? MODE_ROWS : bsdf_const_from(d, i, kseg) ? MODE_UNIFORM : MODE_STRIDED;
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
            BSDF_REQUIRE(in.gmode >= A3D_BSDF_GRAD_NONE && in.gmode <= A3D_BSDF_GRAD_REDUCE);
            if (in.gmode != A3D_BSDF_GRAD_NONE) BSDF_REQUIRE(d->g_in[i] != nullptr);
            if (in.gmode == A3D_BSDF_GRAD_REDUCE) {
                BSDF_REQUIRE(d->g_final[i] != nullptr && d->seg_div[i] >= 1 && (n / d->seg) % d->seg_div[i] == 0);
                const int kr = bsdf_run_dim(d->shape, d->ndim, d->seg * d->seg_div[i]);
                BSDF_REQUIRE(kr >= 0 && bsdf_const_from(d, i, kr) /* a reduced input must be constant over its runs */);
            }
        }
    }
    k.out = d->out;
    k.g_out = d->g_out;
    k.scratch = d->scratch;
    if (bwd) BSDF_REQUIRE(d->g_out != nullptr);
    else BSDF_REQUIRE(d->out != nullptr);
    if (loss && !bwd) BSDF_REQUIRE(d->scratch != nullptr);
#undef BSDF_REQUIRE
    return A3D_OK;
}

template <int OP, bool BWD>
void bsdf_launch(const BsdfK& k, long long rows, hipStream_t stream) {
    bool reduce = false;
    for (int i = 0; i < op_nin(OP); ++i) reduce |= k.in[i].gmode == A3D_BSDF_GRAD_REDUCE;
    if (BWD && OP != A3D_BSDF_IMAGE_LOSS && reduce) {
        hipLaunchKernelGGL((bsdf_kernel<OP, BWD, double>), dim3((unsigned)rows), dim3(THREADS), 0, stream, k);
        return;
    }
    hipLaunchKernelGGL((bsdf_kernel<OP, BWD, float>), dim3((unsigned)rows), dim3(THREADS), 0, stream, k);
}

template <bool BWD>
int bsdf_run(const a3d_bsdf_desc* d, a3d_stream_t stream, const char* fn, BsdfK& k) {
    long long rows;
    const int rc = bsdf_check(d, k, fn, false, BWD, &rows);
    if (rc || k.n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (d->op) {
        case A3D_BSDF_LAMBERT: bsdf_launch<A3D_BSDF_LAMBERT, BWD>(k, rows, s); break;
        case A3D_BSDF_FROSTBITE: bsdf_launch<A3D_BSDF_FROSTBITE, BWD>(k, rows, s); break;
        case A3D_BSDF_PBR_SPECULAR: bsdf_launch<A3D_BSDF_PBR_SPECULAR, BWD>(k, rows, s); break;
        default: bsdf_launch<A3D_BSDF_PBR, BWD>(k, rows, s); break;
    }
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

// the finishing launch of a backward: every reduced input in one grid (y = input)
int bsdf_finish_grads(const a3d_bsdf_desc* d, const BsdfK& k, hipStream_t s) {
    BsdfFin f = {};
    long long max_e = 0;
    const int nin = op_nin(d->op);
    for (int i = 0; i < nin; ++i) {
        if (k.in[i].gmode != A3D_BSDF_GRAD_REDUCE) continue;
        f.rows[i] = reinterpret_cast<const double*>(d->g_in[i]);
        f.final_[i] = d->g_final[i];
        f.R[i] = d->seg_div[i] * k.bps;
        f.ne[i] = (k.n / k.seg) / d->seg_div[i];
        f.C[i] = d->op == A3D_BSDF_IMAGE_LOSS ? 1 : op_cin(d->op, i);
        if (f.ne[i] > max_e) max_e = f.ne[i];
    }
    if (max_e == 0) return A3D_OK;
    hipLaunchKernelGGL(bsdf_finish_kernel, dim3((unsigned)max_e, nin), dim3(THREADS), 0, s, f);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

}  // namespace

extern "C" int64_t a3d_bsdf_rows(const a3d_bsdf_desc* desc) {
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

extern "C" int a3d_bsdf_fwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    BsdfK k;
    return bsdf_run<false>(desc, stream, __func__, k);
}

extern "C" int a3d_bsdf_bwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    BsdfK k;
    const int rc = bsdf_run<true>(desc, stream, __func__, k);
    if (rc || k.n == 0) return rc;
    return bsdf_finish_grads(desc, k, (hipStream_t)stream);
}

extern "C" int a3d_image_loss_fwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    BsdfK k;
    long long rows;
    const int rc = bsdf_check(desc, k, __func__, true, false, &rows);
    if (rc || k.n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (loss_rows_ok(desc, k, false)) {  // (fewer work-groups than `rows`: the scratch is large enough, the finishing launch reads these)
        rows = (k.n / 4 + TILE - 1) / TILE;
        hipLaunchKernelGGL(loss_rows_kernel<false>, dim3((unsigned)rows), dim3(THREADS), 0, s, desc->in[0], desc->in[1], k.n / 4, k.variant,
                           (const float*)nullptr, (double)k.n, (float*)nullptr, (float*)nullptr, reinterpret_cast<double*>(desc->scratch));
    } else {
        bsdf_launch<A3D_BSDF_IMAGE_LOSS, false>(k, rows, s);
    }
    A3D_LAUNCH_CHECK();
    BsdfFin f = {};
    f.rows[0] = reinterpret_cast<const double*>(desc->scratch);
    f.final_[0] = desc->out;
    f.R[0] = rows;
    f.ne[0] = 1;
    f.C[0] = 1;
    f.div = (double)k.n;
    hipLaunchKernelGGL(bsdf_finish_kernel, dim3(1, 1), dim3(THREADS), 0, s, f);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_image_loss_bwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    BsdfK k;
    long long rows;
    const int rc = bsdf_check(desc, k, __func__, true, true, &rows);
    if (rc || k.n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (loss_rows_ok(desc, k, true)) {
        hipLaunchKernelGGL(loss_rows_kernel<true>, dim3((unsigned)((k.n / 4 + TILE - 1) / TILE)), dim3(THREADS), 0, s, desc->in[0], desc->in[1],
                           k.n / 4, k.variant, desc->g_out, (double)k.n, k.in[0].gmode ? desc->g_in[0] : (float*)nullptr,
                           k.in[1].gmode ? desc->g_in[1] : (float*)nullptr, (double*)nullptr);
        A3D_LAUNCH_CHECK();
        return A3D_OK;
    }
    bsdf_launch<A3D_BSDF_IMAGE_LOSS, true>(k, rows, s);
    A3D_LAUNCH_CHECK();
    return bsdf_finish_grads(desc, k, s);
}
