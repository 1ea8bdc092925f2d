// The tangent frame on gfx950 (include/a3d_tangent.h): the per-pixel shading normal with a tangent-space perturbation
// (prepare_shading_normal, reference renderutils/ops.py:194-227, bsdf.py:30-51) and the per-vertex tangents (compute_tangents, reference
// mesh.py:310-350).
//
// Shading normal: the memory side is bsdf.hip's -- one lane per pixel, A3D_BSDF_TILE = 4 x 256 pixels per work-group, inputs read through
// the descriptor's strides in one of three address modes (ROWS / UNIFORM / STRIDED), reduced gradients as double partial rows per
// work-group plus a finishing launch in a fixed order.  84 B per pixel forward (six 3-channel inputs, one output), nothing saved for the
// backward but the inputs.  The arithmetic is the torch statements of model/render/renderutils/ops.py operation by operation
// (-ffp-contract=off), with bsdf_math.h's normalize and its derivative.
//
// Tangents: the gather idiom of normals.hip over the same vertex -> (corner, face) lists, no atomics.  The DMTet atlas gives every face
// its own uv cell with denom ~ (0.9 / N)^2, so face tangents are huge and unrelated and their sums cancel: the face tangent, the sum
// and the two normalisations are carried in double (a few dozen operations per vertex next to ~8 x 15 gathers).
#include <limits.h>

#include "../../include/a3d_tangent.h"
#include "a3d_common.h"
#include "bsdf_math.h"
#include "topo_common.h"

namespace {

using bsdf::V3T;

constexpr int NI = A3D_BSDF_MAX_INPUTS, ND = A3D_BSDF_MAX_DIMS, TILE = A3D_BSDF_TILE, THREADS = 256, ROUNDS = TILE / THREADS;
enum { MODE_ROWS = 0, MODE_UNIFORM = 1, MODE_STRIDED = 2 };

struct SnIn {
    const float* p;
    long long st[ND];
    long long cs;
    float* g;
    int mode, gmode;
};

struct SnK {
    int variant, ndim, small, any_uniform, any_strided;
    long long n, seg, bps;
    long long shape[ND];
    SnIn in[NI];
    float* out;
    const float* g_out;
};

struct SnFin {  // the finishing launch: final[e][c] = sum over rows [e R, (e + 1) R) of rows[.][c]
    const double* rows[NI];
    float* final_[NI];
    long long R[NI], ne[NI];
};

__device__ __forceinline__ void sn_index(const SnK& k, long long p, long long* idx) {
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

__device__ __forceinline__ long long sn_offset(const SnK& k, const SnIn& in, const long long* idx) {
    long long o = 0;
    for (int d = 0; d < k.ndim; ++d) o += idx[d] * in.st[d];
    return o;
}

// sum of v over the work-group, in a fixed order (red: 4 doubles of LDS)
__device__ __forceinline__ double sn_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

template <typename T>
__device__ __forceinline__ V3T<T> cross(V3T<T> a, V3T<T> b) {
    return V3T<T>{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// x[0..5] = pos, view_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm.  Returns the shading normal; BWD: g[] for the output gradient go.
template <bool BWD, typename T>
__device__ __forceinline__ V3T<T> shading_normal(const V3T<T>* x, int variant, V3T<T> go, V3T<T>* g) {
    const bool two_sided = variant & A3D_SHADING_NORMAL_TWO_SIDED;
    const T sign = (variant & A3D_SHADING_NORMAL_OPENGL) ? T(-1.) : T(1.);
    const V3T<T> n0 = bsdf::normalize(x[3]);
    const V3T<T> vd = x[1] - x[0];
    const V3T<T> view = bsdf::normalize(vd);
    const V3T<T> t = bsdf::normalize(x[4]);
    const V3T<T> c = cross(t, n0);
    const V3T<T> bt = bsdf::normalize(c) * sign;
    const V3T<T> p = x[2];
    const T pz = bsdf::maxf(p.z, 0.0);
    const V3T<T> u = t * p.x + bt * p.y + n0 * pz;
    const V3T<T> n1 = bsdf::normalize(u);
    const bool front = !two_sided || bsdf::dot(x[5], view) > T(0.);
    const V3T<T> n2 = front ? n1 : V3T<T>{-n1.x, -n1.y, -n1.z};
    const V3T<T> g2 = front ? x[5] : V3T<T>{-x[5].x, -x[5].y, -x[5].z};
    const T thr = sizeof(T) == 8 ? T(0.1) : T(0.1f);
    const T dn = bsdf::dot(view, n2) / thr;
    const T w = bsdf::clampf(dn, 0.0, 1.0);
    const V3T<T> diff = n2 - g2;
    // torch.lerp: start + w (end - start) below one half, end - (end - start) (1 - w) from there on
    const V3T<T> out = w < T(0.5) ? g2 + diff * w : n2 - diff * (T(1.) - w);
    if (BWD) {
        V3T<T> g_g2 = go * (T(1.) - w), g_n2 = go * w;
        const T g_w = bsdf::dot(go, diff);
        const T g_d = (dn >= T(0.) && dn <= T(1.)) ? g_w / thr : T(0.);
        const V3T<T> g_view = n2 * g_d;
        g_n2 += view * g_d;
        const V3T<T> g_n1 = front ? g_n2 : V3T<T>{-g_n2.x, -g_n2.y, -g_n2.z};
        g[5] = front ? g_g2 : V3T<T>{-g_g2.x, -g_g2.y, -g_g2.z};
        const V3T<T> g_u = bsdf::normalize_bwd(u, g_n1);
        V3T<T> g_t = g_u * p.x;
        const V3T<T> g_bt = g_u * (sign * p.y);
        V3T<T> g_n0 = g_u * pz;
        g[2] = V3T<T>{bsdf::dot(g_u, t), bsdf::dot(g_u, bt), p.z >= T(0.) ? bsdf::dot(g_u, n0) : T(0.)};
        const V3T<T> g_c = bsdf::normalize_bwd(c, g_bt);
        g_t += cross(n0, g_c);   // c = t x n0:  g_t = n0 x g_c,  g_n0 = g_c x t
        g_n0 += cross(g_c, t);
        g[4] = bsdf::normalize_bwd(x[4], g_t);
        g[3] = bsdf::normalize_bwd(x[3], g_n0);
        g[1] = bsdf::normalize_bwd(vd, g_view);
        g[0] = V3T<T>{-g[1].x, -g[1].y, -g[1].z};
    }
    return out;
}

template <typename T>
__device__ __forceinline__ T comp(V3T<T> v, int c) { return c == 0 ? v.x : c == 1 ? v.y : v.z; }

// T: the scalar the per-pixel arithmetic is carried in: float forward, double backward.  bsdf.hip goes to double only when a gradient
// is reduced; here every backward does.  The adjoint of each normalize is a projection g - v (v . g): a component of the result can be
// 1e-3 of its two terms, and where most of a tensor's gradient is exactly zero (view_pos / pos outside the bend's ramp) nothing but that
// component's own relative error is left to judge it by.  In double the gradient carries the rounding of the float32 inputs and of the
// final store only.  view_pos is [B,1,1,3] in every real call, which takes this instantiation in bsdf.hip's scheme as well.
template <bool BWD, typename T>
__global__ __launch_bounds__(THREADS) void sn_kernel(const SnK k) {
    __shared__ double red[4];
    const unsigned bps = (unsigned)k.bps;
    const long long sg = blockIdx.x / bps, blk = blockIdx.x % bps;
    const long long p0 = sg * k.seg;
    long long idx[ND] = {0, 0, 0, 0};
    long long uoff[NI];
    if (k.any_uniform) {
        sn_index(k, p0, idx);
#pragma unroll
        for (int i = 0; i < NI; ++i) uoff[i] = sn_offset(k, k.in[i], idx);
    } else {
#pragma unroll
        for (int i = 0; i < NI; ++i) uoff[i] = 0;
    }
    constexpr bool ACC = BWD && sizeof(T) == 8;
    double acc[ACC ? NI : 1][3];
#pragma unroll
    for (int i = 0; i < (ACC ? NI : 1); ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.0;

    constexpr int UNROLL = BWD ? 1 : ROUNDS;
#pragma unroll UNROLL
    for (int it = 0; it < ROUNDS; ++it) {
        const long long q = blk * TILE + it * THREADS + threadIdx.x;
        if (q >= k.seg) break;
        const long long p = p0 + q;
        if (k.any_strided) sn_index(k, p, idx);
        V3T<T> x[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const SnIn& in = k.in[i];
            if (in.mode == MODE_ROWS) {
                const float* s = in.p + p * 3;
                x[i] = V3T<T>{(T)s[0], (T)s[1], (T)s[2]};
            } else {
                const float* s = in.p + (in.mode == MODE_UNIFORM ? uoff[i] : sn_offset(k, in, idx));
                x[i] = V3T<T>{(T)s[0], (T)s[in.cs], (T)s[2 * in.cs]};
            }
        }
        V3T<T> g[NI];
        V3T<T> go = V3T<T>{T(0), T(0), T(0)};
        if (BWD) go = V3T<T>{(T)k.g_out[p * 3], (T)k.g_out[p * 3 + 1], (T)k.g_out[p * 3 + 2]};
        const V3T<T> o = shading_normal<BWD, T>(x, k.variant, go, g);
        if (!BWD) {
            k.out[p * 3] = (float)o.x; k.out[p * 3 + 1] = (float)o.y; k.out[p * 3 + 2] = (float)o.z;
        } else {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const SnIn& in = k.in[i];
                if (in.gmode == A3D_BSDF_GRAD_DIRECT) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) in.g[p * 3 + c] = (float)comp(g[i], c);
                } else if (ACC && in.gmode == A3D_BSDF_GRAD_REDUCE) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[ACC ? i : 0][c] += comp(g[i], c);
                }
            }
        }
    }
    if (ACC) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (k.in[i].gmode != A3D_BSDF_GRAD_REDUCE) continue;  // (the same in every lane)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double s = sn_block_sum(acc[ACC ? i : 0][c], red);
                if (threadIdx.x == 0) reinterpret_cast<double*>(k.in[i].g)[(long long)blockIdx.x * 3 + c] = s;
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void sn_finish_kernel(const SnFin f) {
    __shared__ double red[4];
    const int i = blockIdx.y;
    const long long e = blockIdx.x;
    if (!f.rows[i] || e >= f.ne[i]) return;  // (the same in every lane of the work-group)
    const long long R = f.R[i];
    const double* rows = f.rows[i] + e * R * 3;
    for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (long long r = threadIdx.x; r < R; r += THREADS) s += rows[r * 3 + c];
        s = sn_block_sum(s, red);
        if (threadIdx.x == 0) f.final_[i][e * 3 + c] = (float)s;
    }
}

// ---- host side (the rules of bsdf.hip's bsdf_check)
// d >= the returned k are the dimensions inside a run of `run` consecutive pixels; -1 when no boundary between dimensions gives that run
int sn_run_dim(const int64_t* shape, int ndim, long long run) {
    long long prod = 1;
    if (run == 1) return ndim;
    for (int d = ndim - 1; d >= 0; --d) {
        prod *= shape[d];
        if (prod == run) return d;
        if (prod > run) return -1;
    }
    return -1;
}

bool sn_const_from(const a3d_bsdf_desc* d, int i, int from) {
    for (int j = from; j < d->ndim; ++j)
        if (d->shape[j] > 1 && d->stride[ND * i + j] != 0) return false;
    return true;
}

// validates everything that can be validated without touching a pointer; fills k (n == 0: nothing to launch)
int sn_check(const a3d_bsdf_desc* d, SnK& k, const char* fn, bool bwd, long long* rows) {
    if (!d) {
        a3d_set_error("%s: invalid argument: desc", fn);
        return A3D_EINVAL;
    }
    if (d->size < sizeof(a3d_bsdf_desc)) {  // (before any other field is read: a shorter struct does not have them)
        a3d_set_error("%s: invalid argument: desc->size %u < sizeof(a3d_bsdf_desc) %zu (a caller built against an older header)", fn, d->size,
                      sizeof(a3d_bsdf_desc));
        return A3D_EINVAL;
    }
#define SN_REQUIRE(cond)                                                \
    do {                                                                \
        if (!(cond)) {                                                  \
            a3d_set_error("%s: invalid argument: %s", fn, #cond);       \
            return A3D_EINVAL;                                          \
        }                                                               \
    } while (0)
    if (d->op != A3D_SHADING_NORMAL || d->variant < 0 || d->variant > 3) {
        a3d_set_error("%s: invalid argument: op %d / variant %d: op must be A3D_SHADING_NORMAL, variant two_sided + 2 * opengl in 0 .. 3", fn, d->op,
                      d->variant);
        return A3D_EINVAL;
    }
    SN_REQUIRE(d->ndim >= 1 && d->ndim <= A3D_BSDF_MAX_DIMS);
    long long n = 1;
    for (int j = 0; j < d->ndim; ++j) {
        if (d->shape[j] < 0 || d->shape[j] > (1ll << 40)) {
            a3d_set_error("%s: invalid argument: shape[%d] = %lld", fn, j, (long long)d->shape[j]);
            return A3D_EINVAL;
        }
        n *= d->shape[j];
        SN_REQUIRE(n <= (1ll << 40));
    }
    k.n = n;
    *rows = 0;
    if (n == 0) return A3D_OK;
    SN_REQUIRE(d->seg >= 1 && n % d->seg == 0);
    const int kseg = sn_run_dim(d->shape, d->ndim, d->seg);
    SN_REQUIRE(kseg >= 0 /* seg must be the product of trailing dimensions */);
    k.seg = d->seg;
    k.bps = (d->seg + TILE - 1) / TILE;
    SN_REQUIRE((n / d->seg) <= INT_MAX / k.bps);
    *rows = (n / d->seg) * k.bps;
    k.variant = d->variant;
    k.ndim = d->ndim;
    k.small = n < (1ll << 31);
    k.any_uniform = k.any_strided = 0;
    for (int j = 0; j < ND; ++j) k.shape[j] = j < d->ndim ? d->shape[j] : 1;
    for (int i = 0; i < NI; ++i) {
        SnIn& in = k.in[i];
        long long rowstride = 3;
        bool rows_mode = d->cstride[i] == 1;
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
        SN_REQUIRE(d->cstride[i] >= 0);
        in.p = d->in[i];
        in.cs = d->cstride[i];
        in.mode = rows_mode ? MODE_ROWS : sn_const_from(d, i, kseg) ? MODE_UNIFORM : MODE_STRIDED;
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
            SN_REQUIRE(in.gmode >= A3D_BSDF_GRAD_NONE && in.gmode <= A3D_BSDF_GRAD_REDUCE);
            if (in.gmode != A3D_BSDF_GRAD_NONE) SN_REQUIRE(d->g_in[i] != nullptr);
            if (in.gmode == A3D_BSDF_GRAD_REDUCE) {
                SN_REQUIRE(d->g_final[i] != nullptr && d->seg_div[i] >= 1 && (n / d->seg) % d->seg_div[i] == 0);
                const int kr = sn_run_dim(d->shape, d->ndim, d->seg * d->seg_div[i]);
                SN_REQUIRE(kr >= 0 && sn_const_from(d, i, kr) /* a reduced input must be constant over its runs */);
            }
        }
    }
    k.out = d->out;
    k.g_out = d->g_out;
    if (bwd) SN_REQUIRE(d->g_out != nullptr);
    else SN_REQUIRE(d->out != nullptr);
#undef SN_REQUIRE
    return A3D_OK;
}

// ---------------------------------------------------------------------------------------------- tangents
struct D3 { double x, y, z; };

// x / sqrt(max(x . x, 1e-20)) (render/util.py:28-32) and its adjoint: clamp passes the gradient where x . x >= 1e-20
__device__ __forceinline__ D3 tg_safe_normalize(D3 v, double& len, double& d) {
    d = v.x * v.x + v.y * v.y + v.z * v.z;
    len = sqrt(d < 1e-20 ? 1e-20 : d);
    return D3{v.x / len, v.y / len, v.z / len};
}
__device__ __forceinline__ D3 tg_safe_normalize_bwd(D3 y, double len, double d, D3 g) {
    D3 r{g.x / len, g.y / len, g.z / len};
    if (d >= 1e-20) {
        const double s = (y.x * g.x + y.y * g.y + y.z * g.z) / len;
        r.x -= y.x * s; r.y -= y.y * s; r.z -= y.z * s;
    }
    return r;
}

struct TgFace {
    int i0, i1, i2, c;
    double uy1, uy2, den;  // uve1.y, uve2.y, the clamped denominator
};

__device__ __forceinline__ TgFace tg_face(int key, int F, const int* __restrict__ tri, const int* __restrict__ ttri, const float* __restrict__ uv) {
    TgFace r;
    r.c = key >= 2 * F ? 2 : (key >= F ? 1 : 0);
    const int f = key - r.c * F;
    r.i0 = tri[3 * f]; r.i1 = tri[3 * f + 1]; r.i2 = tri[3 * f + 2];
    const int u0 = ttri[3 * f], u1 = ttri[3 * f + 1], u2 = ttri[3 * f + 2];
    const double x0 = uv[2ll * u0], y0 = uv[2ll * u0 + 1];
    const double e1x = (double)uv[2ll * u1] - x0, e1y = (double)uv[2ll * u1 + 1] - y0;
    const double e2x = (double)uv[2ll * u2] - x0, e2y = (double)uv[2ll * u2 + 1] - y0;
    const double denom = e1x * e2y - e1y * e2x;
    r.uy1 = e1y; r.uy2 = e2y;
    r.den = denom > 0.0 ? (denom < 1e-6 ? 1e-6 : denom) : (denom > -1e-6 ? -1e-6 : denom);
    return r;
}

__device__ __forceinline__ void tg_sort8(int a[8]) {
#define TG_CX(i, j) { const int x = min(a[i], a[j]), y = max(a[i], a[j]); a[i] = x; a[j] = y; }
    TG_CX(0, 1) TG_CX(2, 3) TG_CX(4, 5) TG_CX(6, 7)
    TG_CX(0, 2) TG_CX(1, 3) TG_CX(4, 6) TG_CX(5, 7)
    TG_CX(1, 2) TG_CX(5, 6) TG_CX(0, 4) TG_CX(3, 7)
    TG_CX(1, 5) TG_CX(2, 6)
    TG_CX(1, 4) TG_CX(3, 6)
    TG_CX(2, 4) TG_CX(3, 5)
    TG_CX(3, 4)
#undef TG_CX
}

// sum over the vertex's incident faces of the face tangent, in ascending key order (cnt >= 1)
__device__ __forceinline__ D3 tg_sum(const float* __restrict__ vp, const float* __restrict__ uv, const int* __restrict__ tri,
                                     const int* __restrict__ ttri, const int* __restrict__ adj, int lo, int cnt, int F) {
    D3 s{0.0, 0.0, 0.0};
    auto add = [&](int key) {
        const TgFace t = tg_face(key, F, tri, ttri, uv);
        const float* p0 = vp + 3ll * t.i0;
        const float* p1 = vp + 3ll * t.i1;
        const float* p2 = vp + 3ll * t.i2;
        const double ax = (double)p1[0] - p0[0], ay = (double)p1[1] - p0[1], az = (double)p1[2] - p0[2];
        const double bx = (double)p2[0] - p0[0], by = (double)p2[1] - p0[1], bz = (double)p2[2] - p0[2];
        s.x += (ax * t.uy2 - bx * t.uy1) / t.den;
        s.y += (ay * t.uy2 - by * t.uy1) / t.den;
        s.z += (az * t.uy2 - bz * t.uy1) / t.den;
    };
    int keys[8];
    nr_load_keys(adj, lo, cnt, keys);
    if (cnt > 8) {  // rare: keep the eight smallest of the whole list
        for (int e = 8; e < cnt; ++e) {
            const int k = adj[lo + e];
            int imax = 0, vmax = keys[0];
#pragma unroll
            for (int q = 1; q < 8; ++q)
                if (keys[q] > vmax) { vmax = keys[q]; imax = q; }
            if (k < vmax) {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (q == imax) keys[q] = k;
            }
        }
    }
    tg_sort8(keys);
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (e < cnt) add(keys[e]);
    int last = keys[7];
    for (int e = 8; e < cnt; ++e) {
        last = nr_next_key_mem(adj, lo, cnt, last);
        add(last);
    }
    return s;
}

// BWD = false: v_tng.  BWD = true: pass 1 of the backward (g_v_nrm and the adjoint of the sum).
template <bool BWD>
__global__ __launch_bounds__(256) void tg_vertex_kernel(const float* __restrict__ v_pos, const float* __restrict__ v_tex, long long tex_stride,
                                                        const float* __restrict__ v_nrm, const int* __restrict__ tri, const int* __restrict__ ttri,
                                                        const int* __restrict__ off, const int* __restrict__ adj, int stride, int V, int F,
                                                        float* __restrict__ v_tng, const float* __restrict__ g_tng, double* __restrict__ g_sum,
                                                        float* __restrict__ g_nrm) {
    const int vi = blockIdx.x * blockDim.x + threadIdx.x;
    if (vi >= V) return;
    const long long b = blockIdx.y, o = (b * V + vi) * 3;
    int lo, cnt;
    vf_list(off, stride, vi, lo, cnt);
    D3 s{0.0, 0.0, 0.0};
    if (cnt > 0) s = tg_sum(v_pos + b * V * 3, v_tex + b * tex_stride, tri, ttri, adj, lo, cnt, F);
    const double nc = (double)cnt;
    const D3 m{s.x / nc, s.y / nc, s.z / nc};  // (no face: 0 / 0 = NaN, as the torch statements give)
    double len1, d1, len2, d2;
    const D3 t1 = tg_safe_normalize(m, len1, d1);
    const D3 N{v_nrm[o], v_nrm[o + 1], v_nrm[o + 2]};
    const double tn = t1.x * N.x + t1.y * N.y + t1.z * N.z;
    const D3 t2{t1.x - tn * N.x, t1.y - tn * N.y, t1.z - tn * N.z};
    const D3 y = tg_safe_normalize(t2, len2, d2);
    if (!BWD) {
        v_tng[o] = (float)y.x; v_tng[o + 1] = (float)y.y; v_tng[o + 2] = (float)y.z;
        return;
    }
    const D3 go{g_tng[o], g_tng[o + 1], g_tng[o + 2]};
    const D3 g2 = tg_safe_normalize_bwd(y, len2, d2, go);
    const double gn = g2.x * N.x + g2.y * N.y + g2.z * N.z;
    // t2 = t1 - (t1 . N) N
    const D3 g1{g2.x - gn * N.x, g2.y - gn * N.y, g2.z - gn * N.z};
    g_nrm[o] = (float)(-(tn * g2.x + gn * t1.x)); g_nrm[o + 1] = (float)(-(tn * g2.y + gn * t1.y)); g_nrm[o + 2] = (float)(-(tn * g2.z + gn * t1.z));
    const D3 gm = tg_safe_normalize_bwd(t1, len1, d1, g1);
    g_sum[o] = gm.x / nc; g_sum[o + 1] = gm.y / nc; g_sum[o + 2] = gm.z / nc;
}

// pass 2: g_v_pos of one (image, vertex) = sum over its incident faces of this corner's share of the face tangent's adjoint
__global__ __launch_bounds__(256) void tg_gather_bwd_kernel(const double* __restrict__ g_sum, const float* __restrict__ v_tex, long long tex_stride,
                                                            const int* __restrict__ tri, const int* __restrict__ ttri, const int* __restrict__ off,
                                                            const int* __restrict__ adj, int stride, int V, int F, float* __restrict__ g_v) {
    const int vi = blockIdx.x * blockDim.x + threadIdx.x;
    if (vi >= V) return;
    const long long b = blockIdx.y, o = (b * V + vi) * 3;
    const double* gs = g_sum + b * V * 3;
    const float* uv = v_tex + b * tex_stride;
    int lo, cnt;
    vf_list(off, stride, vi, lo, cnt);
    D3 a{0.0, 0.0, 0.0};
    int last = -1;
    for (int e = 0; e < cnt; ++e) {  // ascending key order, whatever order the list is stored in
        last = nr_next_key_mem(adj, lo, cnt, last);
        const TgFace t = tg_face(last, F, tri, ttri, uv);
        const double* r0 = gs + 3ll * t.i0;
        const double* r1 = gs + 3ll * t.i1;
        const double* r2 = gs + 3ll * t.i2;
        // the face tangent went to all three corners: its adjoint is the sum of their rows; nom = pe1 uve2.y - pe2 uve1.y
        const double gx = (r0[0] + r1[0] + r2[0]) / t.den, gy = (r0[1] + r1[1] + r2[1]) / t.den, gz = (r0[2] + r1[2] + r2[2]) / t.den;
        const double w = t.c == 1 ? t.uy2 : (t.c == 2 ? -t.uy1 : t.uy1 - t.uy2);  // corner 1: g_pe1, corner 2: g_pe2, corner 0: -(both)
        a.x += gx * w; a.y += gy * w; a.z += gz * w;
    }
    g_v[o] = (float)a.x; g_v[o + 1] = (float)a.y; g_v[o + 2] = (float)a.z;
}

}  // namespace

extern "C" int64_t a3d_shading_normal_rows(const a3d_bsdf_desc* desc) {
    if (!desc || desc->size < sizeof(a3d_bsdf_desc) || desc->op != A3D_SHADING_NORMAL) return -1;
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

extern "C" int a3d_shading_normal_fwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    SnK k;
    long long rows;
    const int rc = sn_check(desc, k, __func__, false, &rows);
    if (rc || k.n == 0) return rc;
    hipLaunchKernelGGL((sn_kernel<false, float>), dim3((unsigned)rows), dim3(THREADS), 0, (hipStream_t)stream, k);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_shading_normal_bwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    SnK k;
    long long rows;
    const int rc = sn_check(desc, k, __func__, true, &rows);
    if (rc || k.n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    SnFin f = {};
    long long max_e = 0;
    for (int i = 0; i < NI; ++i) {
        if (k.in[i].gmode != A3D_BSDF_GRAD_REDUCE) continue;
        f.rows[i] = reinterpret_cast<const double*>(desc->g_in[i]);
        f.final_[i] = desc->g_final[i];
        f.R[i] = desc->seg_div[i] * k.bps;
        f.ne[i] = (k.n / k.seg) / desc->seg_div[i];
        if (f.ne[i] > max_e) max_e = f.ne[i];
    }
    // (always the double instantiation: see sn_kernel)
    hipLaunchKernelGGL((sn_kernel<true, double>), dim3((unsigned)rows), dim3(THREADS), 0, s, k);
    A3D_LAUNCH_CHECK();
    if (max_e == 0) return A3D_OK;
    hipLaunchKernelGGL(sn_finish_kernel, dim3((unsigned)max_e, NI), dim3(THREADS), 0, s, f);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_tangents_fwd(const float* v_pos, const float* v_tex, int64_t tex_batch_stride, const float* v_nrm, const int32_t* t_pos_idx,
                                const int32_t* t_tex_idx, const int32_t* off, const int32_t* adj, int lists_stride, int B, int V, int F,
                                float* v_tng, a3d_stream_t stream) {
    A3D_CHECK_ARG(B > 0 && B <= 65535 && V > 0 && F > 0 && (long long)3 * F < 0x7fffffffll && lists_stride >= 0 && tex_batch_stride >= 0);
    A3D_CHECK_ARG(v_pos && v_tex && v_nrm && t_pos_idx && t_tex_idx && off && adj && v_tng);
    hipLaunchKernelGGL(tg_vertex_kernel<false>, dim3(a3d_div_up(V, 256), B), dim3(256), 0, (hipStream_t)stream, v_pos, v_tex,
                       (long long)tex_batch_stride, v_nrm, t_pos_idx, t_tex_idx, off, adj, lists_stride, V, F, v_tng, (const float*)nullptr,
                       (double*)nullptr, (float*)nullptr);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_tangents_bwd(const float* g_tng, const float* v_pos, const float* v_tex, int64_t tex_batch_stride, const float* v_nrm,
                                const int32_t* t_pos_idx, const int32_t* t_tex_idx, const int32_t* off, const int32_t* adj, int lists_stride, int B,
                                int V, int F, double* g_sum_scratch, float* g_v_pos, float* g_v_nrm, a3d_stream_t stream) {
    A3D_CHECK_ARG(B > 0 && B <= 65535 && V > 0 && F > 0 && (long long)3 * F < 0x7fffffffll && lists_stride >= 0 && tex_batch_stride >= 0);
    A3D_CHECK_ARG(g_tng && v_pos && v_tex && v_nrm && t_pos_idx && t_tex_idx && off && adj && g_sum_scratch && g_v_pos && g_v_nrm);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tg_vertex_kernel<true>, dim3(a3d_div_up(V, 256), B), dim3(256), 0, s, v_pos, v_tex, (long long)tex_batch_stride, v_nrm,
                       t_pos_idx, t_tex_idx, off, adj, lists_stride, V, F, (float*)nullptr, g_tng, g_sum_scratch, g_v_nrm);
    A3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(tg_gather_bwd_kernel, dim3(a3d_div_up(V, 256), B), dim3(256), 0, s, (const double*)g_sum_scratch, v_tex,
                       (long long)tex_batch_stride, t_pos_idx, t_tex_idx, off, adj, lists_stride, V, F, g_v_pos);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
