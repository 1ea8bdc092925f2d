// The tangent frame on gfx950 (include/a3d_tangent.h): the per-pixel shading normal with a tangent-space perturbation
// (prepare_shading_normal, reference renderutils/ops.py:194-227, bsdf.py:30-51) and the per-vertex tangents (compute_tangents, reference
// mesh.py:310-350).
//
// Shading normal: a policy for pixel_desc.h's kernel, the memory side shared with bsdf.hip -- one lane per pixel, A3D_BSDF_TILE = 4 x 256
// pixels per work-group, inputs read through the descriptor's strides in one of three address modes (ROWS / UNIFORM / STRIDED), reduced
// gradients as double partial rows per work-group plus a finishing launch in a fixed order, the descriptor check.  84 B per pixel
// forward (six 3-channel inputs, one output), nothing saved for the backward but the inputs.  The arithmetic is the torch statements of model/render/renderutils/ops.py operation by operation
// (-ffp-contract=off), with bsdf_math.h's normalize and its derivative.
//
// Tangents: the gather idiom of normals.hip over the same vertex -> (corner, face) lists, no atomics.  The DMTet atlas gives every face
// its own uv cell with denom ~ (0.9 / N)^2, so face tangents are huge and unrelated and their sums cancel: the face tangent, the sum
// and the two normalisations are carried in double (a few dozen operations per vertex next to ~8 x 15 gathers).
#include "../../include/a3d_tangent.h"
#include "a3d_common.h"
#include "bsdf_math.h"
#include "pixel_desc.h"
#include "topo_common.h"

namespace {

using bsdf::V3T;

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

// px::kernel's policy.  T, the scalar the per-pixel arithmetic is carried in: float forward, double backward.  bsdf.hip goes to double
// only when a gradient is reduced; here every backward does.  The adjoint of each normalize is a projection g - v (v . g): a component
// of the result can be 1e-3 of its two terms, and where most of a tensor's gradient is exactly zero (view_pos / pos outside the bend's
// ramp) nothing but that component's own relative error is left to judge it by.  In double the gradient carries the rounding of the
// float32 inputs and of the final store only.  view_pos is [B,1,1,3] in every real call, which takes this instantiation in bsdf.hip's
// rule as well.
constexpr int sn_cin(int, int) { return 3; }

struct SnOp {
    static constexpr int NIN = 6, CO = 3;
    static constexpr bool SUM = false;
    static constexpr int cin(int i) { return sn_cin(A3D_SHADING_NORMAL, i); }

    template <bool BWD, typename T>
    static __device__ __forceinline__ void pixel(const px::K& k, const T (&x)[NIN][3], const T* go, T* o, V3T<T>* g) {
        V3T<T> v[NIN];
#pragma unroll
        for (int i = 0; i < NIN; ++i) v[i] = V3T<T>{x[i][0], x[i][1], x[i][2]};
        const V3T<T> r = shading_normal<BWD, T>(v, k.variant, V3T<T>{go[0], go[1], go[2]}, g);
        o[0] = r.x; o[1] = r.y; o[2] = r.z;
    }
};

// the op / variant rule of a3d_shading_normal_* between the two halves of the shared check; fills k (n == 0: nothing to launch)
int sn_check(const a3d_bsdf_desc* d, px::K& k, const char* fn, bool bwd, long long* rows) {
    if (const int rc = px::check_size(d, fn)) return rc;
    if (d->op != A3D_SHADING_NORMAL || d->variant < 0 || d->variant > 3) {
        a3d_set_error("%s: invalid argument: op %d / variant %d: op must be A3D_SHADING_NORMAL, variant two_sided + 2 * opengl in 0 .. 3", fn, d->op,
                      d->variant);
        return A3D_EINVAL;
    }
    return px::check(d, k, fn, SnOp::NIN, sn_cin, bwd, rows);
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
    a3d_sort8(keys);
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
    const int64_t rows = px::rows(desc);  // (>= 0: the descriptor is long enough to have an op)
    return rows < 0 || desc->op != A3D_SHADING_NORMAL ? -1 : rows;
}

extern "C" int a3d_shading_normal_fwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    px::K k;
    long long rows;
    const int rc = sn_check(desc, k, __func__, false, &rows);
    if (rc || k.n == 0) return rc;
    hipLaunchKernelGGL((px::kernel<SnOp, false, float>), dim3((unsigned)rows), dim3(px::THREADS), 0, (hipStream_t)stream, k);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_shading_normal_bwd(const a3d_bsdf_desc* desc, a3d_stream_t stream) {
    px::K k;
    long long rows;
    const int rc = sn_check(desc, k, __func__, true, &rows);
    if (rc || k.n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    // (always the double instantiation: see SnOp)
    hipLaunchKernelGGL((px::kernel<SnOp, true, double>), dim3((unsigned)rows), dim3(px::THREADS), 0, s, k);
    A3D_LAUNCH_CHECK();
    return px::finish_grads(desc, k, SnOp::NIN, sn_cin, s);
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
