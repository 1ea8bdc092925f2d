// Shading BSDFs and the HDR image loss on gfx950 (include/a3d_bsdf.h): lambert, frostbite_diffuse, pbr_specular, pbr_bsdf and image_loss
// of the reference's renderutils (ops.py:244-386, 476-498), one fused launch forward and one backward per call.  The per-pixel arithmetic
// and its hand-written derivatives are bsdf_math.h; the memory side (address modes, reduced gradients, the descriptor check, the finishing
// launch) is pixel_desc.h, shared with tangent.hip.  This file holds the operators' policies, their op / variant rule, the rule that picks
// float or double, and the image loss's fast form for contiguous images.
#include "../../include/a3d_bsdf.h"
#include "a3d_common.h"
#include "bsdf_math.h"
#include "pixel_desc.h"

namespace {

using bsdf::V3T;
using px::ROUNDS;
using px::THREADS;
using px::TILE;

constexpr int op_nin(int op) { return op == A3D_BSDF_LAMBERT ? 2 : op == A3D_BSDF_FROSTBITE ? 4 : op == A3D_BSDF_PBR_SPECULAR ? 5 : op == A3D_BSDF_PBR ? 6 : 2; }
constexpr int op_cin(int op, int i) {
    return op == A3D_BSDF_IMAGE_LOSS ? 1 : (op == A3D_BSDF_FROSTBITE && i == 3) ? 1 : (op == A3D_BSDF_PBR_SPECULAR && i == 4) ? 1 : 3;
}
constexpr int op_cout(int op) { return (op == A3D_BSDF_PBR_SPECULAR || op == A3D_BSDF_PBR) ? 3 : 1; }

// px::kernel's policy for one A3D_BSDF_* code
template <int OP>
struct BsdfOp {
    static constexpr int NIN = op_nin(OP), CO = op_cout(OP);
    static constexpr bool SUM = OP == A3D_BSDF_IMAGE_LOSS;
    static constexpr int cin(int i) { return op_cin(OP, i); }

    template <bool BWD, typename T>
    static __device__ __forceinline__ void pixel(const px::K& k, const T (&x)[NIN][3], const T* go, T* o, V3T<T>* g) {
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
            o[0] = bsdf::image_loss(x[0][0], x[1][0], k.variant & 3, k.variant >> 2, da, db);
            g[0].x = go[0] * da;
            g[1].x = go[0] * db;
        }
    }
};

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
        const double s = px::block_sum(lsum, red);
        if (threadIdx.x == 0) scratch[blockIdx.x] = s;
    }
}

// the fast form applies: both inputs ROWS, everything 16-byte aligned, n a multiple of 4, no reduced gradient
bool loss_rows_ok(const a3d_bsdf_desc* d, const px::K& k, bool bwd) {
    if (k.n % 4 || k.in[0].mode != px::MODE_ROWS || k.in[1].mode != px::MODE_ROWS) return false;
    uintptr_t bits = (uintptr_t)d->in[0] | (uintptr_t)d->in[1];
    if (bwd)
        for (int i = 0; i < 2; ++i) {
            if (k.in[i].gmode == A3D_BSDF_GRAD_REDUCE) return false;
            if (k.in[i].gmode == A3D_BSDF_GRAD_DIRECT) bits |= (uintptr_t)d->g_in[i];
        }
    return (bits & 15) == 0;
}

// the op / variant rule of this file's entry points between the two halves of the shared check; fills k (n == 0: nothing to launch)
int bsdf_check(const a3d_bsdf_desc* d, px::K& k, const char* fn, bool loss, bool bwd, long long* rows) {
    if (const int rc = px::check_size(d, fn)) return rc;
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
    if (const int rc = px::check(d, k, fn, op_nin(d->op), op_cin, bwd, rows)) return rc;
    if (loss && !bwd && k.n && !d->scratch) {
        a3d_set_error("%s: invalid argument: d->scratch != nullptr", fn);
        return A3D_EINVAL;
    }
    return A3D_OK;
}

int bsdf_finish_grads(const a3d_bsdf_desc* d, const px::K& k, hipStream_t s) { return px::finish_grads(d, k, op_nin(d->op), op_cin, s); }

// T, the scalar the per-pixel arithmetic is carried in: float, except in the backward of a BSDF call that reduces a gradient over pixels
// (a [B,1,1,3] camera): there it is double, so that the few numbers such a gradient consists of carry the rounding of the float32
// INPUTS only -- two float32 evaluations of a sum of thousands of ill-conditioned terms otherwise differ by a factor either way.
// (Chosen at compile time where it can be: no forward and no image loss has a double instantiation.)
template <int OP, bool BWD>
void bsdf_launch(const px::K& k, long long rows, hipStream_t stream) {
    if constexpr (BWD && OP != A3D_BSDF_IMAGE_LOSS) {
        bool reduce = false;
        for (int i = 0; i < op_nin(OP); ++i) reduce |= k.in[i].gmode == A3D_BSDF_GRAD_REDUCE;
        if (reduce) {
            hipLaunchKernelGGL((px::kernel<BsdfOp<OP>, BWD, double>), dim3((unsigned)rows), dim3(THREADS), 0, stream, k);
            return;
        }
    }
    hipLaunchKernelGGL((px::kernel<BsdfOp<OP>, BWD, float>), dim3((unsigned)rows), dim3(THREADS), 0, stream, k);
}

template <bool BWD>
int bsdf_run(const a3d_bsdf_desc* d, a3d_stream_t stream, const char* fn, px::K& k) {
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

}  // namespace

extern "C" int64_t a3d_bsdf_rows(const a3d_bsdf_desc* desc) { return px::rows(desc); }

extern "C" int a3d_bsdf_fwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    px::K k;
    return bsdf_run<false>(desc, stream, __func__, k);
}

extern "C" int a3d_bsdf_bwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    px::K k;
    const int rc = bsdf_run<true>(desc, stream, __func__, k);
    if (rc || k.n == 0) return rc;
    return bsdf_finish_grads(desc, k, (hipStream_t)stream);
}

extern "C" int a3d_image_loss_fwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    px::K k;
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
    px::Fin f = {};
    f.rows[0] = reinterpret_cast<const double*>(desc->scratch);
    f.final_[0] = desc->out;
    f.R[0] = rows;
    f.ne[0] = 1;
    f.C[0] = 1;
    f.div = (double)k.n;
    hipLaunchKernelGGL(px::finish_kernel, dim3(1, 1), dim3(THREADS), 0, s, f);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_image_loss_bwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    px::K k;
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
