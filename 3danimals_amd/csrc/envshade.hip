// Environment-lit shading on gfx950 (include/a3d_envshade.h): EnvironmentLight.shade (model/render/light.py, reference light.py:90-128)
// as one launch forward and one backward.
//
// Forward: one lane per pixel.  The statements of light.py operation by operation in float32 (-ffp-contract=off); the three lookups --
// diffuse cube (linear), FG table (2-D linear, clamp), specular stack (trilinear cube, the level from roughness) -- are tex_lookup.h, the
// device code of texture.hip.  60-72 B per pixel: five 3-channel inputs (view_pos usually one row per image), one output; the maps are
// a few KiB to a few MiB and stay in cache.
// Backward: the forward again from the inputs (es_forward, the same function: the same bits), then reverse mode by hand.  The adjoint
// arithmetic is carried in double on the float32 forward values: the adjoint of a normalisation is a difference of nearly equal terms
// (tangent.hip's reason).  g_pos / g_normal / g_kd / g_ks are stored once per pixel; g_view is -g_pos and is not written.
// Texel gradients: every map of at most ES_LDS_MAX_SIZE^2 texels per face is summed in LDS per work-group (all pixels scatter into these
// 18 KiB maps: memory-side float atomics would serialise on them) and leaves as one global atomic per non-zero float, adjacent lanes on
// adjacent floats; larger levels take tex_bwd_kernel's route: per (level slot, tap) the wave merges equal texel rows (ts_merge) and the
// survivors add three adjacent floats.  A wave holds an 8 x 8 pixel tile when H >= 8 and W >= 8 and 64 consecutive pixels otherwise, so
// a [1,1,P] point list fills every lane; the layout decides only which lanes merge, never a pixel's arithmetic.
#include "../../include/a3d_envshade.h"
#include "a3d_common.h"
#include "tex_lookup.h"
#include "tile_scatter.h"

namespace {

constexpr int ES_NIN = A3D_ENV_SHADE_INPUTS;
constexpr int ES_LDS_MAX_SIZE = 16;  // a level gradient [6,S,S,3] is summed in LDS when S <= this (18 KiB at 16; 72 KiB at 32: unmeasured)

struct EsIn {
    const float* p;
    long long ps, is;  // pixel, image stride (elements)
};

struct EsK {
    TexK dif, spec, fg;
    int lds_dif, lds_spec[TX_MAXL];  // first float of the map's gradient in LDS, -1 = the merge route (or not wanted)
    int lds_floats, any_merge;
    EsIn in[ES_NIN];
    const float* mtx;
    int mtx_batch, specular, B, H, W, tiles_x, tiles_y, tiled;
    float lo, hi;
    float* out;
    const float* g_out;
    float* g_in[4];
};

struct F3 { float x, y, z; };
struct D3 { double x, y, z; };

__device__ __forceinline__ F3 es_load(const EsIn& in, long long b, long long p) {
    const float* s = in.p + b * in.is + p * in.ps;
    return F3{s[0], s[1], s[2]};
}
__device__ __forceinline__ float es_dot(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double es_dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 es_d(F3 a) { return D3{(double)a.x, (double)a.y, (double)a.z}; }
// torch.clamp(x, min=lo): NaN stays NaN
__device__ __forceinline__ float es_clamp_min(float x, float lo) { return x < lo ? lo : x; }
__device__ __forceinline__ float es_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// x / sqrt(max(x . x, 1e-20)) (render/util.py:15-21)
__device__ __forceinline__ F3 es_safe_normalize(F3 v, float& d, float& len) {
    d = es_dot(v, v);
    len = sqrtf(es_clamp_min(d, 1e-20f));
    return F3{v.x / len, v.y / len, v.z / len};
}
// its adjoint for the result y: the clamp passes from 1e-20 on
__device__ __forceinline__ D3 es_safe_normalize_bwd(F3 yf, float d, float len, D3 g) {
    const double L = (double)len;
    D3 r{g.x / L, g.y / L, g.z / L};
    if (d >= 1e-20f) {
        const D3 y = es_d(yf);
        const double s = es_dot(y, g) / L;
        r.x -= y.x * s; r.y -= y.y * s; r.z -= y.z * s;
    }
    return r;
}

// rows 0..2 of the [4,4] lookup transform times (v, 0): xfm_vectors.  The statement is a matmul, and light.py does not say how its inner
// product rounds.  ASSUMED here: the BLAS behind it accumulates k = 0..3 with fused multiply-adds (the w = 0 term adds nothing), so the
// chain is written with __fmaf_rn.  Either form is inside the tests' bounds on all but one case: with plain multiply-adds the
// single-pixel list under the 64 / 32 / 16 light had g_specular[2] at 1.11 of its bound (tests/test_envshade_gpu.py), with this chain it
// is inside.
__device__ __forceinline__ F3 es_rotate(const float* __restrict__ m, F3 v) {
    return F3{__fmaf_rn(m[2], v.z, __fmaf_rn(m[1], v.y, m[0] * v.x)), __fmaf_rn(m[6], v.z, __fmaf_rn(m[5], v.y, m[4] * v.x)),
              __fmaf_rn(m[10], v.z, __fmaf_rn(m[9], v.y, m[8] * v.x))};
}
__device__ __forceinline__ D3 es_rotate_t(const float* __restrict__ m, D3 g) {
    return D3{((double)m[0] * g.x + (double)m[4] * g.y) + (double)m[8] * g.z, ((double)m[1] * g.x + (double)m[5] * g.y) + (double)m[9] * g.z,
              ((double)m[2] * g.x + (double)m[6] * g.y) + (double)m[10] * g.z};
}

// acc += sum over the quad's taps of (w lw) texel: tex_fwd_kernel's rule (a tap of weight 0 or row -1 is not read)
template <int C>
__device__ __forceinline__ void es_sample(const float* __restrict__ base, const Quad& q, float lw, float* acc) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float wt = q.w[t] * lw;
        if (q.row[t] >= 0 && wt != 0.f) {
            const float* p = base + (long long)q.row[t] * C;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += wt * p[c];
        }
    }
}

// d (g . sample) / d (x, y) in texel units and the level slot's own value g . sample: tex_bwd_kernel's rule (every tap with a row)
template <int C>
__device__ __forceinline__ void es_quad_grad(const float* __restrict__ base, const Quad& q, const float* g, double& gx, double& gy, double& gs) {
    gx = gy = gs = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (q.row[t] < 0) continue;
        const float* p = base + (long long)q.row[t] * C;
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) v += (double)g[c] * (double)p[c];
        gx += (double)q.wx[t] * v;
        gy += (double)q.wy[t] * v;
        gs += (double)q.w[t] * v;
    }
}

// the same for a 2-D bilinear quad without dropped taps (clamp): the weights' derivatives come in pairs of opposite sign, wx = (-a, a, -b, b)
// and wy = (-c, -d, c, d), so each pair is one difference of the two taps.  Two taps clamped onto one texel row then cancel exactly
// (a coordinate outside the table has no gradient), which the plain sum leaves to rounding.
template <int C>
__device__ __forceinline__ void es_quad_grad_2d(const float* __restrict__ base, const Quad& q, const float* g, double& gx, double& gy) {
    double v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float* p = base + (long long)q.row[t] * C;
        v[t] = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) v[t] += (double)g[c] * (double)p[c];
    }
    gx = (double)q.wx[1] * (v[1] - v[0]) + (double)q.wx[3] * (v[3] - v[2]);
    gy = (double)q.wy[2] * (v[2] - v[0]) + (double)q.wy[3] * (v[3] - v[1]);
}

__device__ __forceinline__ void es_add(D3& v, int i, double x) {  // v[i] += x without a dynamic index
    v.x += i == 0 ? x : 0.0;
    v.y += i == 1 ? x : 0.0;
    v.z += i == 2 ? x : 0.0;
}

// face coordinates -> direction: s = sa uv[ia] / |uv[im]|, t = sb uv[ib] / |uv[im]| (gu, gv: d / d s, d / d t)
__device__ __forceinline__ D3 es_cube_dir_grad(const Lookup& L, double gu, double gv) {
    D3 d{0.0, 0.0, 0.0};
    const double gsu = gu * (double)L.inv_m, gtv = gv * (double)L.inv_m;
    es_add(d, L.ia, gsu * (double)L.sa);
    es_add(d, L.ib, gtv * (double)L.sb);
    es_add(d, L.im, -(gsu * (double)L.s + gtv * (double)L.t) * (double)L.sm);
    return d;
}

// Everything the forward computes for one pixel; the backward calls the same function.
struct EsPixel {
    F3 n, kd, ks, wr, wo, rr, refl, nd, rd;  // inputs; view - pos, its normalisation; the reflection before / after its own; lookup directions
    float d1, len1, d2, len2, dn, ndv, mip, omm, vis, fgA, fgB;
    F3 diff_col, spec_col, reflectance, dif, spec, shaded;
    Lookup Ld, Ls, Lf;
    Quad qd, qs[2], qf;
    Lod lod;
    const float* m;
};

__device__ __forceinline__ void es_empty(Quad& q) {  // a lookup that samples nothing (a zero direction): no tap, no gradient
#pragma unroll
    for (int t = 0; t < 4; ++t) { q.row[t] = -1; q.w[t] = q.wx[t] = q.wy[t] = 0.f; }
}

__device__ __forceinline__ void es_forward(const EsK& k, long long b, long long p, EsPixel& e) {
    const F3 pos = es_load(k.in[A3D_ENV_SHADE_POS], b, p), view = es_load(k.in[A3D_ENV_SHADE_VIEW], b, p);
    e.n = es_load(k.in[A3D_ENV_SHADE_NORMAL], b, p);
    e.kd = es_load(k.in[A3D_ENV_SHADE_KD], b, p);
    e.ks = es_load(k.in[A3D_ENV_SHADE_KS], b, p);
    e.wr = F3{view.x - pos.x, view.y - pos.y, view.z - pos.z};
    e.wo = es_safe_normalize(e.wr, e.d1, e.len1);
    e.dn = es_dot(e.wo, e.n);
    const float two_dn = 2.f * e.dn;
    e.rr = F3{two_dn * e.n.x - e.wo.x, two_dn * e.n.y - e.wo.y, two_dn * e.n.z - e.wo.z};
    e.refl = es_safe_normalize(e.rr, e.d2, e.len2);
    e.m = k.mtx_batch ? k.mtx + (k.mtx_batch == 1 ? 0 : b * 16) : nullptr;
    e.rd = e.m ? es_rotate(e.m, e.refl) : e.refl;
    e.nd = e.m ? es_rotate(e.m, e.n) : e.n;

    {  // diffuse irradiance: cube, linear
        const float d[3] = {e.nd.x, e.nd.y, e.nd.z};
        e.Ld = make_lookup(k.dif, d, 0, 1);
        float acc[3] = {0.f, 0.f, 0.f};
        if (e.Ld.valid) {
            level_quad(k.dif, e.Ld, d, 0, 0, false, e.qd);
            es_sample<3>(k.dif.level[0], e.qd, 1.f, acc);
        } else {
            es_empty(e.qd);
        }
        e.dif = F3{acc[0], acc[1], acc[2]};
    }
    e.vis = 1.f - e.ks.x;
    if (!k.specular) {
        e.diff_col = e.kd;
        e.shaded = F3{e.dif.x * e.kd.x, e.dif.y * e.kd.y, e.dif.z * e.kd.z};
        return;
    }
    const float rough = e.ks.y, metal = e.ks.z;
    e.omm = 1.f - metal;
    const float f0 = e.omm * 0.04f;
    e.spec_col = F3{f0 + e.kd.x * metal, f0 + e.kd.y * metal, f0 + e.kd.z * metal};
    e.diff_col = F3{e.kd.x * e.omm, e.kd.y * e.omm, e.kd.z * e.omm};
    e.shaded = F3{e.dif.x * e.diff_col.x, e.dif.y * e.diff_col.y, e.dif.z * e.diff_col.z};
    {  // FG term of the split sum: 2-D, linear, clamp
        e.ndv = es_clamp_min(e.dn, 1e-4f);
        const float uv[2] = {e.ndv, rough};
        e.Lf = make_lookup(k.fg, uv, 0, 1);
        level_quad(k.fg, e.Lf, uv, 0, 0, false, e.qf);
        float acc[2] = {0.f, 0.f};
        es_sample<2>(k.fg.level[0], e.qf, 1.f, acc);
        e.fgA = acc[0]; e.fgB = acc[1];
    }
    {  // roughness-adjusted specular lookup: get_mip as the level bias, no uv_da
        const float nl2 = (float)(k.spec.levels - 2);
        e.mip = rough < k.hi ? (es_clamp(rough, k.lo, k.hi) - k.lo) / (k.hi - k.lo) * nl2
                             : ((es_clamp(rough, k.hi, 1.f) - k.hi) / (1.f - k.hi) + (float)k.spec.levels) - 2.f;
        const float d[3] = {e.rd.x, e.rd.y, e.rd.z};
        e.Ls = make_lookup(k.spec, d, 0, 1);
        float acc[3] = {0.f, 0.f, 0.f};
        if (e.Ls.valid) {
            const float bias[1] = {e.mip};
            lod_of(k.spec, e.Ls, nullptr, bias, 0, e.lod);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                level_quad(k.spec, e.Ls, d, 0, e.lod.lv[j], false, e.qs[j]);
                es_sample<3>(k.spec.level[e.lod.lv[j]], e.qs[j], e.lod.lw[j], acc);
            }
        } else {
            es_empty(e.qs[0]);
            es_empty(e.qs[1]);
            e.lod.lv[0] = e.lod.lv[1] = 0; e.lod.lw[0] = e.lod.lw[1] = 0.f; e.lod.live = false;
        }
        e.spec = F3{acc[0], acc[1], acc[2]};
    }
    e.reflectance = F3{e.spec_col.x * e.fgA + e.fgB, e.spec_col.y * e.fgA + e.fgB, e.spec_col.z * e.fgA + e.fgB};
    e.shaded = F3{e.shaded.x + e.spec.x * e.reflectance.x, e.shaded.y + e.spec.y * e.reflectance.y, e.shaded.z + e.spec.z * e.reflectance.z};
}

__global__ __launch_bounds__(256) void es_fwd_kernel(const EsK k, long long n, long long per_image) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long b = i / per_image, p = i - b * per_image;
    EsPixel e;
    es_forward(k, b, p, e);
    float* o = k.out + i * 3;
    o[0] = e.shaded.x * e.vis; o[1] = e.shaded.y * e.vis; o[2] = e.shaded.z * e.vis;
}

// The texel scatter of one level slot.  Every lane of the wave calls this, in wave-uniform control flow (the merge is cross-lane);
// ``on`` = this lane has a contribution.  lds_off >= 0: the level's gradient lives in LDS.
__device__ __forceinline__ void es_scatter(const TexK& k, bool any_merge, bool on, int l, int lds_off, const Quad& q, float lw, const float* g,
                                           float* __restrict__ lds) {
    float* gl = k.grad[l];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float wt = q.w[t] * lw;
        const bool live = on && gl && q.row[t] >= 0 && wt != 0.f;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) { v[0] = g[0] * wt; v[1] = g[1] * wt; v[2] = g[2] * wt; }
        if (live && lds_off >= 0) {
            float* dst = lds + lds_off + q.row[t] * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (v[c] != 0.f) atomicAdd(dst + c, v[c]);
        }
        if (any_merge) {  // (the same in every lane: a kernel argument)
            int key = (live && lds_off < 0) ? k.keybase[l] + q.row[t] : -1;
            if (__ballot(key >= 0)) {  // (wave-uniform)
                if (key < 0) v[0] = v[1] = v[2] = 0.f;
                ts_merge<4, 6>(key, v);
                if (key >= 0) {
                    float* dst = gl + (long long)q.row[t] * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (v[c] != 0.f) atomicAdd(dst + c, v[c]);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void es_bwd_kernel(const EsK k) {
    extern __shared__ __attribute__((aligned(16))) float es_lds[];
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long per_image = (long long)k.H * k.W, n = per_image * k.B;
    long long b, p;
    bool valid;
    if (k.tiled) {
        const long long tiles = (long long)k.tiles_x * k.tiles_y;
        b = wave / tiles;
        const long long r = wave - b * tiles;
        const int px = (int)(r % k.tiles_x) * 8 + (lane & 7), py = (int)(r / k.tiles_x) * 8 + (lane >> 3);
        valid = b < k.B && px < k.W && py < k.H;
        p = (long long)py * k.W + px;
    } else {
        const long long i = wave * 64 + lane;
        valid = i < n;
        b = i / per_image;
        p = i - b * per_image;
    }
    if (!valid) b = p = 0;  // (lanes without a pixel recompute pixel 0 and contribute nothing: the merges and barriers need the whole wave)
    if (k.lds_floats) {
        for (int j = threadIdx.x; j < k.lds_floats; j += 256) es_lds[j] = 0.f;
        __syncthreads();
    }
    const long long i = b * per_image + p;
    EsPixel e;
    es_forward(k, b, p, e);
    const float* gop = k.g_out + i * 3;
    const float go[3] = {gop[0], gop[1], gop[2]};
    const float gsh[3] = {go[0] * e.vis, go[1] * e.vis, go[2] * e.vis};  // to the colour before the visibility factor
    const double g_ksx = -(((double)go[0] * (double)e.shaded.x + (double)go[1] * (double)e.shaded.y) + (double)go[2] * (double)e.shaded.z);
    const float gdv[3] = {gsh[0] * e.diff_col.x, gsh[1] * e.diff_col.y, gsh[2] * e.diff_col.z};  // to the diffuse sample
    const D3 g_dc{(double)gsh[0] * (double)e.dif.x, (double)gsh[1] * (double)e.dif.y, (double)gsh[2] * (double)e.dif.z};
    D3 g_kd = g_dc, g_n{0.0, 0.0, 0.0}, g_refl{0.0, 0.0, 0.0};
    double g_rough = 0.0, g_metal = 0.0, g_dn = 0.0;

    // ---- diffuse lookup: direction gradient and texel scatter
    D3 g_nd{0.0, 0.0, 0.0};
    if (e.Ld.valid) {
        double gx, gy, gs;
        es_quad_grad<3>(k.dif.level[0], e.qd, gdv, gx, gy, gs);
        const double half = 0.5 * (double)k.dif.w[0];
        g_nd = es_cube_dir_grad(e.Ld, gx * half, gy * half);
    }
    es_scatter(k.dif, k.any_merge, valid && e.Ld.valid, 0, k.lds_dif, e.qd, 1.f, gdv, es_lds);

    if (k.specular) {  // (the same in every lane)
        const D3 kd = es_d(e.kd);
        const float gsv[3] = {gsh[0] * e.reflectance.x, gsh[1] * e.reflectance.y, gsh[2] * e.reflectance.z};  // to the specular sample
        const D3 g_R{(double)gsh[0] * (double)e.spec.x, (double)gsh[1] * (double)e.spec.y, (double)gsh[2] * (double)e.spec.z};
        const double A = (double)e.fgA, metal = (double)e.ks.z;
        const D3 g_sc{g_R.x * A, g_R.y * A, g_R.z * A};
        const float g_fg[2] = {(float)es_dot(g_R, es_d(e.spec_col)), (float)((g_R.x + g_R.y) + g_R.z)};
        const double omm = (double)e.omm;
        g_kd = D3{g_sc.x * metal + g_dc.x * omm, g_sc.y * metal + g_dc.y * omm, g_sc.z * metal + g_dc.z * omm};
        g_metal = (es_dot(g_sc, kd) - (double)0.04f * ((g_sc.x + g_sc.y) + g_sc.z)) - es_dot(g_dc, kd);
        {  // FG table: uv = (ndv, roughness)
            double gx, gy;
            es_quad_grad_2d<2>(k.fg.level[0], e.qf, g_fg, gx, gy);
            if (e.dn >= 1e-4f) g_dn = gx * (double)k.fg.w[0];
            g_rough = gy * (double)k.fg.h[0];
        }
        D3 g_rd{0.0, 0.0, 0.0};
        const bool son = e.Ls.valid;
        if (son) {
            double gu = 0.0, gv = 0.0, gsl[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                double gx, gy;
                const int l = e.lod.lv[j];
                es_quad_grad<3>(k.spec.level[l], e.qs[j], gsv, gx, gy, gsl[j]);
                const double f = (double)e.lod.lw[j] * 0.5 * (double)k.spec.w[l];
                gu += gx * f;
                gv += gy * f;
            }
            g_rd = es_cube_dir_grad(e.Ls, gu, gv);
            if (e.lod.live) {  // the level is not clamped: it reaches the roughness through get_mip
                const float rough = e.ks.y;
                const double glev = gsl[1] - gsl[0];
                if (rough < k.hi) {
                    if (rough >= k.lo && rough <= k.hi) g_rough += glev * ((double)(k.spec.levels - 2) / (double)(k.hi - k.lo));
                } else if (rough >= k.hi && rough <= 1.f) {
                    g_rough += glev / (double)(1.f - k.hi);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int l = e.lod.lv[j];
            es_scatter(k.spec, k.any_merge, valid && son, l, k.lds_spec[l], e.qs[j], e.lod.lw[j], gsv, es_lds);
        }
        g_refl = e.m ? es_rotate_t(e.m, g_rd) : g_rd;
    }
    g_n = e.m ? es_rotate_t(e.m, g_nd) : g_nd;

    // ---- refl = safe_normalize(2 dot(wo, n) n - wo), dn = dot(wo, n), wo = safe_normalize(view - pos)
    const D3 nv = es_d(e.n), wo = es_d(e.wo);
    const D3 g_rr = es_safe_normalize_bwd(e.refl, e.d2, e.len2, g_refl);
    g_dn += 2.0 * es_dot(g_rr, nv);
    const double two_dn = 2.0 * (double)e.dn;
    const D3 g_wo{g_dn * nv.x - g_rr.x, g_dn * nv.y - g_rr.y, g_dn * nv.z - g_rr.z};
    g_n = D3{g_n.x + two_dn * g_rr.x + g_dn * wo.x, g_n.y + two_dn * g_rr.y + g_dn * wo.y, g_n.z + two_dn * g_rr.z + g_dn * wo.z};
    const D3 g_wr = es_safe_normalize_bwd(e.wo, e.d1, e.len1, g_wo);
    if (valid) {
        if (float* g = k.g_in[0]) { g[i * 3] = (float)-g_wr.x; g[i * 3 + 1] = (float)-g_wr.y; g[i * 3 + 2] = (float)-g_wr.z; }
        if (float* g = k.g_in[1]) { g[i * 3] = (float)g_n.x; g[i * 3 + 1] = (float)g_n.y; g[i * 3 + 2] = (float)g_n.z; }
        if (float* g = k.g_in[2]) { g[i * 3] = (float)g_kd.x; g[i * 3 + 1] = (float)g_kd.y; g[i * 3 + 2] = (float)g_kd.z; }
        if (float* g = k.g_in[3]) { g[i * 3] = (float)g_ksx; g[i * 3 + 1] = (float)g_rough; g[i * 3 + 2] = (float)g_metal; }
    }

    // ---- the LDS-resident gradients leave: one global atomic per non-zero float, adjacent lanes on adjacent floats
    if (k.lds_floats) {
        __syncthreads();
        if (k.lds_dif >= 0) {
            const int cnt = 18 * k.dif.w[0] * k.dif.w[0];
            for (int j = threadIdx.x; j < cnt; j += 256) {
                const float v = es_lds[k.lds_dif + j];
                if (v != 0.f) atomicAdd(k.dif.grad[0] + j, v);
            }
        }
        for (int l = 0; l < k.spec.levels; ++l) {
            if (k.lds_spec[l] < 0) continue;
            const int cnt = 18 * k.spec.w[l] * k.spec.w[l];
            for (int j = threadIdx.x; j < cnt; j += 256) {
                const float v = es_lds[k.lds_spec[l] + j];
                if (v != 0.f) atomicAdd(k.spec.grad[l] + j, v);
            }
        }
    }
}

void es_clear(TexK& k) {
    for (int l = 0; l < TX_MAXL; ++l) { k.level[l] = nullptr; k.grad[l] = nullptr; k.h[l] = k.w[l] = 1; k.keybase[l] = 0; }
    k.C = 3; k.tex_batch = 1; k.filter = A3D_TEX_LINEAR; k.boundary = A3D_TEX_CUBE; k.levels = 1; k.cube = 1;
}

// validates everything that can be validated without touching a pointer; fills k
int es_check(const a3d_env_shade_desc* d, EsK& k, const char* fn, bool bwd) {
#define ES_REQUIRE(cond)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            a3d_set_error("%s: invalid argument: %s", fn, #cond); \
            return A3D_EINVAL;                                    \
        }                                                         \
    } while (0)
    if (!d) {
        a3d_set_error("%s: invalid argument: desc", fn);
        return A3D_EINVAL;
    }
    if (d->size < sizeof(a3d_env_shade_desc)) {  // (before any other field is read: a shorter struct does not have them)
        a3d_set_error("%s: invalid argument: desc->size %u < sizeof(a3d_env_shade_desc) %zu (a caller built against an older header)", fn,
                      d->size, sizeof(a3d_env_shade_desc));
        return A3D_EINVAL;
    }
    ES_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0);
    ES_REQUIRE((long long)d->B * d->H * d->W < (1ll << 31) / 3);
    ES_REQUIRE(d->diffuse != nullptr && d->diffuse_size > 0 && d->diffuse_size <= 8192);
    ES_REQUIRE(d->mtx_batch == 0 || d->mtx_batch == 1 || d->mtx_batch == d->B);
    ES_REQUIRE(d->mtx_batch == 0 || d->mtx != nullptr);
    for (int i = 0; i < ES_NIN; ++i) {
        if (!d->in[i] || d->pixel_stride[i] < 0 || d->image_stride[i] < 0) {
            a3d_set_error("%s: invalid argument: in[%d] is NULL or has a negative stride", fn, i);
            return A3D_EINVAL;
        }
        k.in[i] = EsIn{d->in[i], (long long)d->pixel_stride[i], (long long)d->image_stride[i]};
    }
    es_clear(k.dif);
    es_clear(k.spec);
    es_clear(k.fg);
    k.dif.level[0] = d->diffuse;
    k.dif.h[0] = k.dif.w[0] = d->diffuse_size;
    k.specular = d->specular != 0;
    if (k.specular) {
        if (d->levels < 3 || d->levels > A3D_TEX_MAX_LEVELS) {
            a3d_set_error("%s: invalid argument: %d specular levels: at least 3 specular levels (the level rule divides by levels - 2), at most %d",
                          fn, d->levels, A3D_TEX_MAX_LEVELS);
            return A3D_EINVAL;
        }
        long long rows = 0;
        for (int l = 0; l < d->levels; ++l) {
            const int S = d->spec_size[l];
            if (!d->spec[l] || S <= 0 || S > 8192) {
                a3d_set_error("%s: invalid argument: specular level %d is NULL or has size %d", fn, l, S);
                return A3D_EINVAL;
            }
            if (l > 0) {
                const int s0 = d->spec_size[l - 1];
                if (!((s0 == 1 || s0 % 2 == 0) && S == (s0 > 1 ? s0 / 2 : 1))) {
                    a3d_set_error("%s: invalid argument: specular level %d is %d x %d, the halving rule gives it from %d x %d", fn, l, S, S, s0, s0);
                    return A3D_EINVAL;
                }
            }
            k.spec.level[l] = d->spec[l];
            k.spec.h[l] = k.spec.w[l] = S;
            k.spec.keybase[l] = (int)rows;
            rows += 6ll * S * S;
        }
        ES_REQUIRE(rows < 0x7fffffffll);
        k.spec.levels = d->levels;
        k.spec.filter = A3D_TEX_LINEAR_MIPMAP_LINEAR;
        ES_REQUIRE(d->fg != nullptr && d->fg_height > 0 && d->fg_width > 0 && d->fg_height <= 32768 && d->fg_width <= 32768);
        k.fg.level[0] = d->fg;
        k.fg.h[0] = d->fg_height; k.fg.w[0] = d->fg_width;
        k.fg.C = 2; k.fg.boundary = A3D_TEX_CLAMP; k.fg.cube = 0;
        ES_REQUIRE(d->min_roughness >= 0.f && d->min_roughness < d->max_roughness && d->max_roughness < 1.f);
    }
    k.lo = d->min_roughness; k.hi = d->max_roughness;
    k.mtx = d->mtx; k.mtx_batch = d->mtx_batch;
    k.B = d->B; k.H = d->H; k.W = d->W;
    k.tiled = d->H >= 8 && d->W >= 8;
    k.tiles_x = a3d_div_up(d->W, 8); k.tiles_y = a3d_div_up(d->H, 8);
    k.out = d->out; k.g_out = d->g_out;
    k.lds_dif = -1; k.lds_floats = 0; k.any_merge = 0;
    for (int l = 0; l < TX_MAXL; ++l) k.lds_spec[l] = -1;
    for (int j = 0; j < 4; ++j) k.g_in[j] = nullptr;
    if (!bwd) {
        ES_REQUIRE(d->out != nullptr);
        return A3D_OK;
    }
    ES_REQUIRE(d->g_out != nullptr);
    for (int j = 0; j < 4; ++j) k.g_in[j] = d->g_in[j];
    // the LDS plan: every wanted gradient of a small map, one after the other
    auto place = [&](int S, float* g, int& off) {
        if (!g) return;
        if (S <= ES_LDS_MAX_SIZE) { off = k.lds_floats; k.lds_floats += 18 * S * S; }
        else k.any_merge = 1;
    };
    k.dif.grad[0] = d->g_diffuse;
    place(d->diffuse_size, d->g_diffuse, k.lds_dif);
    if (k.specular)
        for (int l = 0; l < d->levels; ++l) {
            k.spec.grad[l] = d->g_spec[l];
            place(d->spec_size[l], d->g_spec[l], k.lds_spec[l]);
        }
#undef ES_REQUIRE
    return A3D_OK;
}

}  // namespace

extern "C" int a3d_env_shade_fwd(const a3d_env_shade_desc* desc, a3d_stream_t stream) {
    EsK k;
    if (const int rc = es_check(desc, k, __func__, false)) return rc;
    const long long per_image = (long long)k.H * k.W, n = per_image * k.B;
    hipLaunchKernelGGL(es_fwd_kernel, dim3(a3d_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, k, n, per_image);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_env_shade_bwd(const a3d_env_shade_desc* desc, a3d_stream_t stream) {
    EsK k;
    if (const int rc = es_check(desc, k, __func__, true)) return rc;
    const long long n = (long long)k.H * k.W * k.B;
    const long long waves = k.tiled ? (long long)k.tiles_x * k.tiles_y * k.B : (n + 63) / 64;
    hipLaunchKernelGGL(es_bwd_kernel, dim3(a3d_div_up(waves, 4)), dim3(256), sizeof(float) * (size_t)k.lds_floats, (hipStream_t)stream, k);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
