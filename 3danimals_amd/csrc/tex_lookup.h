// The texture lookup as device code, once: the descriptor the kernels see, the cube face rule with its edge walk and corner tap, a level's
// bilinear quad with the derivatives of its weights, the level of detail and the row helpers.  texture.hip (dr.texture in every mode)
// and envshade.hip (the three lookups of EnvironmentLight.shade inside one launch) include it; the semantics are written out in ops.py
// texture().
#pragma once
#include "a3d_common.h"

namespace {

constexpr int TX_MAXL = A3D_TEX_MAX_LEVELS;

// the descriptor as the kernels see it (by value): level pointers, sizes, and the first key of each level in one row numbering
struct TexK {
    const float* level[TX_MAXL];
    float* grad[TX_MAXL];
    int h[TX_MAXL], w[TX_MAXL];
    int keybase[TX_MAXL];
    int C, tex_batch, filter, boundary, levels, cube;
};

struct Lookup {
    bool valid;
    int b;        // image
    int face;     // cube face
    float s, t;   // cube face coordinates (-1..1)
    float inv_m;  // 1 / |major component|
    int ia, ib, im;
    float sa, sb, sm;  // signs: s = sa uv[ia] / |uv[im]|, t = sb uv[ib] / |uv[im]|, sm = sign(uv[im])
};

// Face of a direction and its coordinates: the face of the largest |component| (ties x before y before z), the exact inverse of the
// reference's cube_to_dir (model/render/util.py:96-103): +x (-z,-y), -x (z,-y), +y (x,z), -y (x,-z), +z (x,-y), -z (-x,-y), over |major|.
__device__ __forceinline__ void cube_face(float x, float y, float z, int& face, int& ia, int& ib, int& im, float& sa, float& sb, float& sm) {
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    if (ax >= ay && ax >= az) {
        im = 0; ia = 2; ib = 1; sb = -1.f;
        if (x >= 0.f) { face = 0; sa = -1.f; sm = 1.f; } else { face = 1; sa = 1.f; sm = -1.f; }
    } else if (ay >= az) {
        im = 1; ia = 0; ib = 2; sa = 1.f;
        if (y >= 0.f) { face = 2; sb = 1.f; sm = 1.f; } else { face = 3; sb = -1.f; sm = -1.f; }
    } else {
        im = 2; ia = 0; ib = 1; sb = -1.f;
        if (z >= 0.f) { face = 4; sa = 1.f; sm = 1.f; } else { face = 5; sa = -1.f; sm = -1.f; }
    }
}

// the reference's cube_to_dir(face, s, t)
__device__ __forceinline__ void cube_dir(int face, float s, float t, float& x, float& y, float& z) {
    switch (face) {
        case 0: x = 1.f; y = -t; z = -s; break;
        case 1: x = -1.f; y = -t; z = s; break;
        case 2: x = s; y = 1.f; z = t; break;
        case 3: x = s; y = -1.f; z = -t; break;
        case 4: x = s; y = -t; z = 1.f; break;
        default: x = -s; y = -t; z = -1.f; break;
    }
}

__device__ __forceinline__ float comp(const float* v, int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : v[2]); }

// Where a lookup's coordinates come from.  GEN = false: the caller's uv in memory.  GEN = true: generated from the element index of an
// [B, H, W] grid -- the two environment-probe resamplers (include/a3d.h "Texture sampling", generated coordinates; reference
// model/render/util.py:105-133), every statement rounded once in float32 (the files that include this header build with
// -ffp-contract=off) with the full-precision sinf / cosf / atan2f / acosf:
//   2-D texture:  B = 6 faces; uv of (face, y, x) = the lat-long coordinates of normalize(cube_to_dir(face, gx, gy));
//   cube texture: the direction of (b, y, x) = (sin(theta) sin(phi), cos(theta), -sin(theta) cos(phi)), theta = gy pi, phi = gx pi.
// lin_at is torch.linspace's two-sided rule; the end points are the reference's Python doubles rounded to float32 once.
__device__ __forceinline__ float lin_at(float a, float b, int n, int i) {
    if (n == 1) return a;
    const float step = (b - a) / (float)(n - 1);
    return i < n / 2 ? a + step * (float)i : b - step * (float)(n - 1 - i);
}

template <bool GEN>
struct UvSrc {
    const float* __restrict__ uv;  // GEN = false
    int H, W;                      // GEN = true: the lookup grid

    __device__ __forceinline__ void grid(long long i, int& p, float& gx, float& gy, double y_first) const {
        const long long per = (long long)H * W, r = i % per;
        const int y = (int)(r / W), x = (int)(r % W);
        p = (int)(i / per);
        const double ry = 1.0 / (double)H, rx = 1.0 / (double)W;
        gy = lin_at((float)(y_first + ry), (float)(1.0 - ry), H, y);
        gx = lin_at((float)(-1.0 + rx), (float)(1.0 - rx), W, x);
    }
    // the direction of a cube lookup
    __device__ __forceinline__ void dir(long long i, float* d) const {
        if constexpr (GEN) {
            int b;
            float gx, gy;
            grid(i, b, gx, gy, 0.0);
            const float pi = 3.14159265358979323846f;
            const float theta = gy * pi, phi = gx * pi;
            const float st = sinf(theta), ct = cosf(theta), sp = sinf(phi), cp = cosf(phi);
            d[0] = st * sp; d[1] = ct; d[2] = -(st * cp);
        } else {
            d[0] = uv[3 * i]; d[1] = uv[3 * i + 1]; d[2] = uv[3 * i + 2];
        }
    }
    // the coordinates of a 2-D lookup
    __device__ __forceinline__ void uv2(long long i, float& u, float& v) const {
        if constexpr (GEN) {
            int face;
            float gx, gy, d[3];
            grid(i, face, gx, gy, -1.0);
            cube_dir(face, gx, gy, d[0], d[1], d[2]);
            const float len = sqrtf(fmaxf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2], 1e-20f));
            const float vx = d[0] / len, vy = d[1] / len, vz = d[2] / len;
            u = atan2f(vx, -vz) / 6.28318530717958647692f + 0.5f;  // (-vz: an exact negation, atan2f(+0, -0) = pi)
            v = acosf(fminf(fmaxf(vy, -1.f), 1.f)) / 3.14159265358979323846f;
        } else {
            u = uv[2 * i]; v = uv[2 * i + 1];
        }
    }
};

template <bool GEN>
__device__ __forceinline__ Lookup make_lookup(const TexK& k, const UvSrc<GEN>& src, long long i, long long per_image) {
    Lookup L;
    L.valid = true;
    L.b = k.tex_batch == 1 ? 0 : (int)(i / per_image);
    L.face = 0; L.s = L.t = 0.f; L.inv_m = 0.f; L.ia = L.ib = L.im = 0; L.sa = L.sb = L.sm = 1.f;
    if (k.cube) {
        float d[3];
        src.dir(i, d);
        cube_face(d[0], d[1], d[2], L.face, L.ia, L.ib, L.im, L.sa, L.sb, L.sm);
        const float m = fabsf(comp(d, L.im));
        if (!(m > 0.f) || !(m < INFINITY)) {  // zero or non-finite direction: output 0, no gradient
            L.valid = false;
            return L;
        }
        L.inv_m = 1.f / m;
        L.s = L.sa * comp(d, L.ia) / m;
        L.t = L.sb * comp(d, L.ib) / m;
    }
    return L;
}
__device__ __forceinline__ Lookup make_lookup(const TexK& k, const float* __restrict__ uv, long long i, long long per_image) {
    return make_lookup(k, UvSrc<false>{uv, 0, 0}, i, per_image);
}

// texel row of a cube tap (ix, iy) on the lookup's face at size S, after the edge walk; -1 = a corner tap (both coordinates outside)
__device__ __forceinline__ int cube_row(const Lookup& L, int S, int ix, int iy) {
    const bool inx = ix >= 0 && ix < S, iny = iy >= 0 && iy < S;
    if (inx && iny) return ((L.b * 6 + L.face) * S + iy) * S + ix;
    if (!inx && !iny) return -1;
    // the virtual texel centre on the extended face plane -> its direction -> the face it lies on, clamped into range
    const float sv = -1.f + (float)(2 * ix + 1) / (float)S, tv = -1.f + (float)(2 * iy + 1) / (float)S;
    float d[3];
    cube_dir(L.face, sv, tv, d[0], d[1], d[2]);
    int face, ia, ib, im;
    float sa, sb, sm;
    cube_face(d[0], d[1], d[2], face, ia, ib, im, sa, sb, sm);
    const float m = fabsf(comp(d, im));
    const float s2 = sa * comp(d, ia) / m, t2 = sb * comp(d, ib) / m;
    const int jx = min(max((int)floorf((s2 + 1.f) * 0.5f * (float)S), 0), S - 1);
    const int jy = min(max((int)floorf((t2 + 1.f) * 0.5f * (float)S), 0), S - 1);
    return ((L.b * 6 + face) * S + jy) * S + jx;
}

__device__ __forceinline__ int wrap_index(int i, int n, int boundary, bool& inside) {
    inside = i >= 0 && i < n;
    if (boundary == A3D_TEX_WRAP) {
        const int r = i % n;
        return r < 0 ? r + n : r;
    }
    return min(max(i, 0), n - 1);
}

// floor of a texel coordinate as an int, kept far inside the int range whatever the input (NaN included: fmaxf / fminf drop it)
__device__ __forceinline__ float safe_floor(float x) { return floorf(fminf(fmaxf(x, -1.0e9f), 1.0e9f)); }

// A 2-D texel coordinate beyond +-2^22 has lost the half of "u * size - 0.5" (and beyond safe_floor's 1e9 its fraction): reduce before
// the floor.  Wrap: the taps and the fraction of (u - floor(u)) * size - 0.5 are those of u * size - 0.5 (u - floorf(u) is exact in fp32).
// Clamp / zero: a coordinate below -2 has the taps and the result of -2, one above size + 1 those of size + 1.  Ordinary lookups
// never come here, so their results stay bit-identical; for every finite uv the weights stay in [0, 1] and sum to 1.
constexpr float TX_FAR = 4194304.f;  // 2^22
__device__ __forceinline__ float far_coord(float u, int size, int boundary, float x) {
    if (boundary == A3D_TEX_WRAP) return (u - floorf(u)) * (float)size - 0.5f;
    return fminf(fmaxf(x, -2.f), (float)size + 1.f);
}

// The 4 taps (nearest: 1) of a level: row (-1 = contributes nothing), weight, d weight / d x and d y in texel units
struct Quad {
    int row[4];
    float w[4], wx[4], wy[4];
};

template <bool GEN>
__device__ __forceinline__ void level_quad(const TexK& k, const Lookup& L, const UvSrc<GEN>& src, long long i, int l, bool nearest,
                                           Quad& q) {
    const int H = k.h[l], W = k.w[l];
    float x, y;
    if (k.cube) {
        x = (L.s + 1.f) * 0.5f * (float)W - 0.5f;
        y = (L.t + 1.f) * 0.5f * (float)W - 0.5f;
    } else {
        float u, v;
        src.uv2(i, u, v);
        x = u * (float)W - 0.5f;
        y = v * (float)H - 0.5f;
        if (fabsf(x) > TX_FAR) x = far_coord(u, W, k.boundary, x);
        if (fabsf(y) > TX_FAR) y = far_coord(v, H, k.boundary, y);
    }
    if (nearest) {
        const int ix = (int)safe_floor(x + 0.5f), iy = (int)safe_floor(y + 0.5f);
        if (k.cube) {
            q.row[0] = ((L.b * 6 + L.face) * W + min(max(iy, 0), W - 1)) * W + min(max(ix, 0), W - 1);
        } else {
            bool inx, iny;
            const int jx = wrap_index(ix, W, k.boundary, inx), jy = wrap_index(iy, H, k.boundary, iny);
            q.row[0] = (k.boundary == A3D_TEX_ZERO && !(inx && iny)) ? -1 : (L.b * H + jy) * W + jx;
        }
        q.w[0] = 1.f; q.wx[0] = q.wy[0] = 0.f;
        for (int j = 1; j < 4; ++j) { q.row[j] = -1; q.w[j] = q.wx[j] = q.wy[j] = 0.f; }
        return;
    }
    const float x0 = safe_floor(x), y0 = safe_floor(y);
    const float fx = x - x0, fy = y - y0;
    const int ix = (int)x0, iy = (int)y0;
    q.w[0] = (1.f - fx) * (1.f - fy); q.wx[0] = -(1.f - fy); q.wy[0] = -(1.f - fx);
    q.w[1] = fx * (1.f - fy);         q.wx[1] = (1.f - fy);  q.wy[1] = -fx;
    q.w[2] = (1.f - fx) * fy;         q.wx[2] = -fy;         q.wy[2] = (1.f - fx);
    q.w[3] = fx * fy;                 q.wx[3] = fy;          q.wy[3] = fx;
    if (k.cube) {
        // (no dynamic index into the quad: it would live in scratch)
        float cw = 0.f, cwx = 0.f, cwy = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            q.row[j] = cube_row(L, W, ix + (j & 1), iy + (j >> 1));
            if (q.row[j] < 0) { cw = q.w[j]; cwx = q.wx[j]; cwy = q.wy[j]; q.w[j] = q.wx[j] = q.wy[j] = 0.f; }
        }
        // the corner texel (at most one per quad) = mean of the other three: its weight and derivatives go to them in thirds
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q.row[j] >= 0) { q.w[j] += cw * (1.f / 3.f); q.wx[j] += cwx * (1.f / 3.f); q.wy[j] += cwy * (1.f / 3.f); }
    } else {
        bool in0, in1, jn0, jn1;
        const int x_0 = wrap_index(ix, W, k.boundary, in0), x_1 = wrap_index(ix + 1, W, k.boundary, in1);
        const int y_0 = wrap_index(iy, H, k.boundary, jn0), y_1 = wrap_index(iy + 1, H, k.boundary, jn1);
        const bool zero = k.boundary == A3D_TEX_ZERO;
        const int base = L.b * H;
        q.row[0] = zero && !(in0 && jn0) ? -1 : (base + y_0) * W + x_0;
        q.row[1] = zero && !(in1 && jn0) ? -1 : (base + y_0) * W + x_1;
        q.row[2] = zero && !(in0 && jn1) ? -1 : (base + y_1) * W + x_0;
        q.row[3] = zero && !(in1 && jn1) ? -1 : (base + y_1) * W + x_1;
    }
}

__device__ __forceinline__ void level_quad(const TexK& k, const Lookup& L, const float* __restrict__ uv, long long i, int l, bool nearest,
                                           Quad& q) {
    level_quad(k, L, UvSrc<false>{uv, 0, 0}, i, l, nearest, q);
}

// Level of detail and the two level slots.  lw[j] = weight of level lv[j]; dlod[4] = d level / d (J00, J01, J10, J11) (0 when the level is
// clamped or the mode does not differentiate it); J (texel units) is returned for the uv_da chain.
struct Lod {
    int lv[2];
    float lw[2];
    bool live;  // linear-mipmap-linear and not clamped: g_level flows to uv_da and the bias
    float dl[4];
};

__device__ __forceinline__ void lod_of(const TexK& k, const Lookup& L, const float* __restrict__ uv_da, const float* __restrict__ bias,
                                       long long i, Lod& o) {
    o.lv[0] = o.lv[1] = 0; o.lw[0] = 1.f; o.lw[1] = 0.f; o.live = false;
    o.dl[0] = o.dl[1] = o.dl[2] = o.dl[3] = 0.f;
    if (k.filter < A3D_TEX_LINEAR_MIPMAP_NEAREST) return;
    float lod = 0.f;
    bool lod_ok = true;  // (a zero Jacobian: level -inf, clamped to 0, no gradient)
    float dlam[4] = {0.f, 0.f, 0.f, 0.f}, dlod_dlam = 0.f;
    if (uv_da) {
        const float* dq = uv_da + 6 * i;  // (cube)
        const float4 d4 = k.cube ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4*>(uv_da)[i];
        float J00, J01, J10, J11, a, c, bb, hd, r, lam;
        // J of uv_da * 2^-ex (exact: J is linear in uv_da), lambda_max(J J^T) and its parts
        auto eig = [&](int ex) {
            auto sc = [ex](float v) { return ex ? ldexpf(v, -ex) : v; };
            if (k.cube) {
                const float half = 0.5f * (float)k.w[0];
                const float mX = L.sm * sc(dq[2 * L.im]), mY = L.sm * sc(dq[2 * L.im + 1]);
                J00 = half * (L.sa * sc(dq[2 * L.ia]) - L.s * mX) * L.inv_m;
                J01 = half * (L.sa * sc(dq[2 * L.ia + 1]) - L.s * mY) * L.inv_m;
                J10 = half * (L.sb * sc(dq[2 * L.ib]) - L.t * mX) * L.inv_m;
                J11 = half * (L.sb * sc(dq[2 * L.ib + 1]) - L.t * mY) * L.inv_m;
            } else {
                J00 = sc(d4.x) * (float)k.w[0]; J01 = sc(d4.y) * (float)k.w[0];
                J10 = sc(d4.z) * (float)k.h[0]; J11 = sc(d4.w) * (float)k.h[0];
            }
            a = J00 * J00 + J01 * J01; c = J10 * J10 + J11 * J11; bb = J00 * J10 + J01 * J11;
            hd = 0.5f * (a - c); r = sqrtf(hd * hd + bb * bb);
            lam = 0.5f * (a + c) + r;
        };
        eig(0);
        int ex = 0;
        if (!(lam > 0.f && lam < INFINITY)) {
            // lambda over- or underflowed fp32 (|J| beyond ~6e9 or below ~1e-19 texels per pixel) for a finite, non-zero uv_da: redo it on
            // uv_da * 2^-ex (its largest component into [0.5, 1)); level = 0.5 log2(lambda') + ex, and d level / d J scales by 2^-ex.
            // A zero J stays a zero J (level 0); a non-finite uv_da is outside the specification (level 0 too).
            float m = k.cube ? 0.f : fmaxf(fmaxf(fabsf(d4.x), fabsf(d4.y)), fmaxf(fabsf(d4.z), fabsf(d4.w)));
            if (k.cube)
                for (int j = 0; j < 6; ++j) m = fmaxf(m, fabsf(dq[j]));
            if (m > 0.f && m < INFINITY) {
                frexpf(m, &ex);
                eig(ex);
            }
        }
        if (lam > 0.f && lam < INFINITY) {
            lod = 0.5f * log2f(lam) + (float)ex;
            dlod_dlam = ldexpf(0.5f / (lam * 0.69314718055994531f), -ex);
            const float da = r > 0.f ? 0.5f + hd / (2.f * r) : 0.5f, dc = r > 0.f ? 0.5f - hd / (2.f * r) : 0.5f, db = r > 0.f ? bb / r : 0.f;
            dlam[0] = 2.f * J00 * da + J10 * db;
            dlam[1] = 2.f * J01 * da + J11 * db;
            dlam[2] = 2.f * J10 * dc + J00 * db;
            dlam[3] = 2.f * J11 * dc + J01 * db;
        } else {
            lod_ok = false;
        }
    }
    float level = lod + (bias ? bias[i] : 0.f);
    const float top = (float)(k.levels - 1);
    const bool clamped = !lod_ok || !(level >= 0.f && level <= top);
    level = lod_ok ? fminf(fmaxf(level, 0.f), top) : 0.f;
    if (k.filter == A3D_TEX_LINEAR_MIPMAP_NEAREST) {
        o.lv[0] = min((int)floorf(level + 0.5f), k.levels - 1);
        return;
    }
    const int l0 = min((int)floorf(level), k.levels - 1);
    o.lv[0] = l0; o.lv[1] = min(l0 + 1, k.levels - 1);
    o.lw[1] = level - (float)l0; o.lw[0] = 1.f - o.lw[1];
    if (!clamped && L.valid) {
        o.live = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.dl[j] = dlod_dlam * dlam[j];
    }
}

template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ p, int c, int C) {
    if (VEC) return *reinterpret_cast<const float4*>(p + c);
    return make_float4(p[c], c + 1 < C ? p[c + 1] : 0.f, c + 2 < C ? p[c + 2] : 0.f, c + 3 < C ? p[c + 3] : 0.f);
}
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, int c, int C, float4 v) {
    if (VEC) { *reinterpret_cast<float4*>(p + c) = v; return; }
    p[c] = v.x;
    if (c + 1 < C) p[c + 1] = v.y;
    if (c + 2 < C) p[c + 2] = v.z;
    if (c + 3 < C) p[c + 3] = v.w;
}
__device__ __forceinline__ void fma4(float4& a, float w, float4 b) { a.x += w * b.x; a.y += w * b.y; a.z += w * b.z; a.w += w * b.w; }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

}  // namespace
