// Texture sampling on gfx950 -- replaces dr.texture in every mode the reference calls it in (include/a3d.h "Texture sampling";
// the specification, unpinned against upstream nvdiffrast, is written out in ops.py texture()).
//
// Forward: one lane per lookup.  Level selection, the (up to) two levels' bilinear quads and the cube face walk stay in registers; each
// lookup reads its 4 or 8 texel rows and writes one output row, 16-byte loads and stores when C % 4 == 0.
// Backward: the same taps, recomputed.  g_uv / g_uv_da / g_bias are plain stores.  The texel scatter into the level gradients does NOT
// issue one float atomic per lane and texel: a wave holds an 8 x 8 block of lookups, and neighbouring lookups magnify the same texels,
// so for each (level slot, tap slot) the lanes first merge equal texel rows with the quadtree of tile_scatter.h (ts_merge: partners at
// lane distance 1, 8, 2, 16, 4, 32) and only the surviving lanes add their rows, C adjacent floats each.  A lane whose row differs from
// its partner's simply keeps it: correctness never depends on how much merges.
// Mip stack: the box-filter chain is built one level per launch (thread = output element, float4 when C % 4 == 0); its backward walks
// from the coarsest level down, each fine element reading its one coarse parent (no atomics).
#include "a3d_common.h"
#include "tile_scatter.h"

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

__device__ __forceinline__ Lookup make_lookup(const TexK& k, const float* __restrict__ uv, long long i, long long per_image) {
    Lookup L;
    L.valid = true;
    L.b = k.tex_batch == 1 ? 0 : (int)(i / per_image);
    L.face = 0; L.s = L.t = 0.f; L.inv_m = 0.f; L.ia = L.ib = L.im = 0; L.sa = L.sb = L.sm = 1.f;
    if (k.cube) {
        const float d[3] = {uv[3 * i], uv[3 * i + 1], uv[3 * i + 2]};
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

__device__ __forceinline__ void level_quad(const TexK& k, const Lookup& L, const float* __restrict__ uv, long long i, int l, bool nearest,
                                           Quad& q) {
    const int H = k.h[l], W = k.w[l];
    float x, y;
    if (k.cube) {
        x = (L.s + 1.f) * 0.5f * (float)W - 0.5f;
        y = (L.t + 1.f) * 0.5f * (float)W - 0.5f;
    } else {
        const float u = uv[2 * i], v = uv[2 * i + 1];
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

template <bool VEC>
__global__ __launch_bounds__(256) void tex_fwd_kernel(const TexK k, const float* __restrict__ uv, const float* __restrict__ uv_da,
                                                      const float* __restrict__ bias, long long n, long long per_image,
                                                      float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int C = k.C;
    float* o = out + i * C;
    const Lookup L = make_lookup(k, uv, i, per_image);
    if (!L.valid) {
        for (int c = 0; c < C; c += 4) store4<VEC>(o, c, C, make_float4(0.f, 0.f, 0.f, 0.f));
        return;
    }
    Lod lod;
    lod_of(k, L, uv_da, bias, i, lod);
    const int nl = k.filter == A3D_TEX_LINEAR_MIPMAP_LINEAR ? 2 : 1;
    const bool nearest = k.filter == A3D_TEX_NEAREST;
    Quad q[2];
    const float* base[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j >= nl) break;
        level_quad(k, L, uv, i, lod.lv[j], nearest, q[j]);
        base[j] = k.level[lod.lv[j]];
#pragma unroll
        for (int t = 0; t < 4; ++t) q[j].w[t] *= lod.lw[j];
    }
    const int nt = nearest ? 1 : 4;
    for (int c = 0; c < C; c += 4) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (j < nl && t < nt && q[j].row[t] >= 0 && q[j].w[t] != 0.f) fma4(acc, q[j].w[t], load4<VEC>(base[j] + (long long)q[j].row[t] * C, c, C));
        store4<VEC>(o, c, C, acc);
    }
}

// Backward: a wave = an 8 x 8 block of lookups of one image when W >= 8 (lane bits 0..2 = x, 3..5 = y: ts_merge's partner lanes are
// neighbours), 64 consecutive lookups otherwise.  Every lane runs every merge (the merge needs the whole wave); lanes without a lookup
// carry key -1.
template <bool VEC>
__global__ __launch_bounds__(256) void tex_bwd_kernel(const TexK k, const float* __restrict__ g_out, const float* __restrict__ uv,
                                                      const float* __restrict__ uv_da, const float* __restrict__ bias, int B, int H, int W,
                                                      int tiles_x, int tiles_y, float* __restrict__ g_uv, float* __restrict__ g_uv_da,
                                                      float* __restrict__ g_bias) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long per_image = (long long)H * W, n = per_image * B;
    long long i;
    bool valid;
    if (W >= 8) {
        const long long tiles = (long long)tiles_x * tiles_y;
        const long long b = wave / tiles, r = wave - b * tiles;
        const int px = (int)(r % tiles_x) * 8 + (lane & 7), py = (int)(r / tiles_x) * 8 + (lane >> 3);
        valid = b < B && px < W && py < H;
        i = (b * H + py) * (long long)W + px;
    } else {
        i = wave * 64 + lane;
        valid = i < n;
    }
    if (!valid) i = 0;
    const int C = k.C;
    Lookup L = make_lookup(k, uv, i, per_image);
    L.valid = L.valid && valid;
    Lod lod;
    lod_of(k, L, uv_da, bias, i, lod);
    const int nl = k.filter == A3D_TEX_LINEAR_MIPMAP_LINEAR ? 2 : 1;  // (wave-uniform: the merge loops below must be)
    const bool nearest = k.filter == A3D_TEX_NEAREST;
    const int nt = nearest ? 1 : 4;
    Quad q[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (j < nl) level_quad(k, L, uv, i, lod.lv[j], nearest, q[j]);
    const float* g = g_out + i * C;
    // ---- the lookup's own gradients: d out / d x, d y per level slot, and the two levels' difference for d out / d level
    float gx[2] = {0.f, 0.f}, gy[2] = {0.f, 0.f}, gs[2] = {0.f, 0.f};
    if (L.valid && !nearest) {
        for (int c = 0; c < C; c += 4) {
            const float4 gc = load4<VEC>(g, c, C);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j >= nl) break;
                const float* base = k.level[lod.lv[j]];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (q[j].row[t] < 0) continue;
                    const float v = dot4(gc, load4<VEC>(base + (long long)q[j].row[t] * C, c, C));
                    gx[j] += q[j].wx[t] * v;
                    gy[j] += q[j].wy[t] * v;
                    gs[j] += q[j].w[t] * v;
                }
            }
        }
    }
    if (valid) {
        if (g_uv) {
            float gu = 0.f, gv = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j >= nl) break;
                const int l = lod.lv[j];
                if (k.cube) {
                    gu += lod.lw[j] * gx[j] * 0.5f * (float)k.w[l];
                    gv += lod.lw[j] * gy[j] * 0.5f * (float)k.w[l];
                } else {
                    gu += lod.lw[j] * gx[j] * (float)k.w[l];
                    gv += lod.lw[j] * gy[j] * (float)k.h[l];
                }
            }
            if (k.cube) {  // s = sa uv[ia] / |m|, t = sb uv[ib] / |m|
                float d[3] = {0.f, 0.f, 0.f};
                if (L.valid) {
                    const float gsu = gu * L.inv_m, gtv = gv * L.inv_m;
                    d[L.ia] += gsu * L.sa;
                    d[L.ib] += gtv * L.sb;
                    d[L.im] -= (gsu * L.s + gtv * L.t) * L.sm;
                }
                g_uv[3 * i] = d[0]; g_uv[3 * i + 1] = d[1]; g_uv[3 * i + 2] = d[2];
            } else {
                g_uv[2 * i] = gu; g_uv[2 * i + 1] = gv;
            }
        }
        const float glev = lod.live ? gs[1] - gs[0] : 0.f;  // (lw = (1 - f, f): d out / d f = S1 - S0)
        if (g_bias) g_bias[i] = glev;
        if (g_uv_da) {
            const float gJ[4] = {glev * lod.dl[0], glev * lod.dl[1], glev * lod.dl[2], glev * lod.dl[3]};
            if (k.cube) {
                float d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (lod.live) {
                    const float f = 0.5f * (float)k.w[0] * L.inv_m;
                    d[2 * L.ia] += gJ[0] * f * L.sa; d[2 * L.ia + 1] += gJ[1] * f * L.sa;
                    d[2 * L.ib] += gJ[2] * f * L.sb; d[2 * L.ib + 1] += gJ[3] * f * L.sb;
                    d[2 * L.im] -= (gJ[0] * L.s + gJ[2] * L.t) * f * L.sm;
                    d[2 * L.im + 1] -= (gJ[1] * L.s + gJ[3] * L.t) * f * L.sm;
                }
                for (int j = 0; j < 6; ++j) g_uv_da[6 * i + j] = d[j];
            } else {
                reinterpret_cast<float4*>(g_uv_da)[i] = make_float4(gJ[0] * (float)k.w[0], gJ[1] * (float)k.w[0], gJ[2] * (float)k.h[0],
                                                                    gJ[3] * (float)k.h[0]);
            }
        }
    }
    // ---- the texel scatter: per (level slot, tap slot), merge equal rows inside the wave, survivors add C adjacent floats
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j >= nl) break;
        const int l = lod.lv[j];
        float* gl = k.grad[l];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t >= nt) break;
            const float wt = q[j].w[t] * lod.lw[j];
            const int key = (L.valid && gl && q[j].row[t] >= 0 && wt != 0.f) ? k.keybase[l] + q[j].row[t] : -1;
            for (int c = 0; c < C; c += 4) {
                float4 gc = make_float4(0.f, 0.f, 0.f, 0.f);
                if (key >= 0) gc = load4<VEC>(g, c, C);
                float v[4] = {gc.x * wt, gc.y * wt, gc.z * wt, gc.w * wt};
                int kk = key;
                ts_merge<4, 6>(kk, v);
                if (kk >= 0) {
                    float* dst = gl + (long long)q[j].row[t] * C + c;
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        if (c + m < C && v[m] != 0.f) atomicAdd(dst + m, v[m]);
                }
            }
        }
    }
}

// one mip level from the one before: out[p, y, x, :] = mean of the box (sy x sx) at (y * sy, x * sx); p = image (and face)
template <bool VEC>
__global__ __launch_bounds__(256) void tex_mip_fwd_kernel(const float* __restrict__ in, int Hi, int Wi, int Ho, int Wo, int C, long long n,
                                                          float* __restrict__ out) {
    const int CV = VEC ? C / 4 : C;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int cv = (int)(e % CV);
    const long long px = e / CV;
    const int x = (int)(px % Wo);
    const long long py = px / Wo;
    const int y = (int)(py % Ho);
    const long long p = py / Ho;
    const int sy = Hi > Ho ? 2 : 1, sx = Wi > Wo ? 2 : 1;
    const float scale = 1.f / (float)(sx * sy);
    const long long r0 = (p * Hi + (long long)y * sy) * Wi + (long long)x * sx;
    if (VEC) {
        const float4* src = reinterpret_cast<const float4*>(in);
        float4 a = src[r0 * CV + cv];
        if (sx == 2) fma4(a, 1.f, src[(r0 + 1) * CV + cv]);
        if (sy == 2) {
            fma4(a, 1.f, src[(r0 + Wi) * CV + cv]);
            if (sx == 2) fma4(a, 1.f, src[(r0 + Wi + 1) * CV + cv]);
        }
        reinterpret_cast<float4*>(out)[e] = make_float4(a.x * scale, a.y * scale, a.z * scale, a.w * scale);
    } else {
        float a = in[r0 * C + cv];
        if (sx == 2) a += in[(r0 + 1) * C + cv];
        if (sy == 2) {
            a += in[(r0 + Wi) * C + cv];
            if (sx == 2) a += in[(r0 + Wi + 1) * C + cv];
        }
        out[e] = a * scale;
    }
}

// the box filter's adjoint: every fine element gets its coarse parent's gradient / box size (added in place)
template <bool VEC>
__global__ __launch_bounds__(256) void tex_mip_bwd_kernel(const float* __restrict__ g_coarse, int Hi, int Wi, int Ho, int Wo, int C,
                                                          long long n, float* __restrict__ g_fine) {
    const int CV = VEC ? C / 4 : C;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int cv = (int)(e % CV);
    const long long px = e / CV;
    const int x = (int)(px % Wi);
    const long long py = px / Wi;
    const int y = (int)(py % Hi);
    const long long p = py / Hi;
    const int sy = Hi > Ho ? 2 : 1, sx = Wi > Wo ? 2 : 1;
    const float scale = 1.f / (float)(sx * sy);
    const long long pr = (p * Ho + y / sy) * Wo + x / sx;
    if (VEC) {
        const float4 gc = reinterpret_cast<const float4*>(g_coarse)[pr * CV + cv];
        float4& d = reinterpret_cast<float4*>(g_fine)[e];
        fma4(d, scale, gc);
    } else {
        g_fine[e] += scale * g_coarse[pr * C + cv];
    }
}

int tex_check(const a3d_tex_desc* d, TexK& k, const char* fn) {
    if (!d) {
        a3d_set_error("%s: invalid argument: desc", fn);
        return A3D_EINVAL;
    }
    if (d->size < sizeof(a3d_tex_desc)) {  // (before any other field is read: a shorter struct does not have them)
        a3d_set_error("%s: invalid argument: desc->size %u < sizeof(a3d_tex_desc) %zu (a caller built against an older header)", fn,
                      d->size, sizeof(a3d_tex_desc));
        return A3D_EINVAL;
    }
    const bool cube = d->boundary == A3D_TEX_CUBE;
    bool ok = d->C > 0 && d->tex_batch > 0 && d->filter >= A3D_TEX_NEAREST && d->filter <= A3D_TEX_LINEAR_MIPMAP_LINEAR &&
              d->boundary >= A3D_TEX_WRAP && d->boundary <= A3D_TEX_CUBE && d->levels >= 1 && d->levels <= TX_MAXL;
    long long rows = 0;
    for (int l = 0; ok && l < d->levels; ++l) {
        ok = d->level[l] && d->height[l] > 0 && d->width[l] > 0 && (!cube || d->height[l] == d->width[l]);
        k.level[l] = d->level[l];
        k.grad[l] = d->grad[l];
        k.h[l] = d->height[l];
        k.w[l] = d->width[l];
        k.keybase[l] = (int)rows;
        rows += (long long)d->tex_batch * (cube ? 6 : 1) * d->height[l] * d->width[l];
        ok = ok && rows < 0x7fffffffll;
    }
    if (!ok) {
        a3d_set_error("%s: invalid argument: descriptor (C, tex_batch, filter, boundary, levels, level sizes / pointers, < 2^31 texels)", fn);
        return A3D_EINVAL;
    }
    for (int l = d->levels; l < TX_MAXL; ++l) { k.level[l] = nullptr; k.grad[l] = nullptr; k.h[l] = k.w[l] = 1; k.keybase[l] = 0; }
    k.C = d->C; k.tex_batch = d->tex_batch; k.filter = d->filter; k.boundary = d->boundary; k.levels = d->levels; k.cube = cube;
    return A3D_OK;
}

bool tex_vec(const TexK& k) {  // 16-byte rows: every level (and gradient) pointer 16-byte aligned and C % 4 == 0
    if (k.C % 4) return false;
    for (int l = 0; l < k.levels; ++l)
        if ((uintptr_t)k.level[l] % 16 || (uintptr_t)k.grad[l] % 16) return false;
    return true;
}

int tex_halving_ok(const a3d_tex_desc* d, const char* fn) {
    for (int l = 1; l < d->levels; ++l) {
        const int h = d->height[l - 1], w = d->width[l - 1];
        const bool ok = (h == 1 || h % 2 == 0) && (w == 1 || w % 2 == 0) && d->height[l] == (h > 1 ? h / 2 : 1) && d->width[l] == (w > 1 ? w / 2 : 1);
        if (!ok) {
            a3d_set_error("%s: invalid argument: level %d is %d x %d, the halving rule gives it from %d x %d", fn, l, d->height[l],
                          d->width[l], h, w);
            return A3D_EINVAL;
        }
    }
    return A3D_OK;
}

}  // namespace

extern "C" int a3d_texture_fwd(const a3d_tex_desc* desc, const float* uv, const float* uv_da_or_null, const float* bias_or_null, int B, int H,
                               int W, float* out, a3d_stream_t stream) {
    TexK k;
    const int rc = tex_check(desc, k, __func__);
    if (rc) return rc;
    A3D_CHECK_ARG(uv && out && B > 0 && H > 0 && W > 0);
    A3D_CHECK_ARG(k.tex_batch == 1 || k.tex_batch == B);
    const long long per_image = (long long)H * W, n = per_image * B;
    const bool vec = tex_vec(k) && (uintptr_t)out % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(tex_fwd_kernel<true>, dim3(a3d_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, k, uv, uv_da_or_null, bias_or_null,
                           n, per_image, out);
    else
        hipLaunchKernelGGL(tex_fwd_kernel<false>, dim3(a3d_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, k, uv, uv_da_or_null, bias_or_null,
                           n, per_image, out);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_texture_bwd(const a3d_tex_desc* desc, const float* g_out, const float* uv, const float* uv_da_or_null,
                               const float* bias_or_null, int B, int H, int W, float* g_uv_or_null, float* g_uv_da_or_null, float* g_bias_or_null,
                               a3d_stream_t stream) {
    TexK k;
    const int rc = tex_check(desc, k, __func__);
    if (rc) return rc;
    A3D_CHECK_ARG(g_out && uv && B > 0 && H > 0 && W > 0);
    A3D_CHECK_ARG(k.tex_batch == 1 || k.tex_batch == B);
    A3D_CHECK_ARG(!g_uv_da_or_null || uv_da_or_null);
    A3D_CHECK_ARG(!g_bias_or_null || bias_or_null);
    const long long n = (long long)H * W * B;
    const int tiles_x = a3d_div_up(W, 8), tiles_y = a3d_div_up(H, 8);
    const long long waves = W >= 8 ? (long long)tiles_x * tiles_y * B : (n + 63) / 64;
    const bool vec = tex_vec(k) && (uintptr_t)g_out % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(tex_bwd_kernel<true>, dim3(a3d_div_up(waves, 4)), dim3(256), 0, (hipStream_t)stream, k, g_out, uv, uv_da_or_null,
                           bias_or_null, B, H, W, tiles_x, tiles_y, g_uv_or_null, g_uv_da_or_null, g_bias_or_null);
    else
        hipLaunchKernelGGL(tex_bwd_kernel<false>, dim3(a3d_div_up(waves, 4)), dim3(256), 0, (hipStream_t)stream, k, g_out, uv, uv_da_or_null,
                           bias_or_null, B, H, W, tiles_x, tiles_y, g_uv_or_null, g_uv_da_or_null, g_bias_or_null);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_texture_mip_fwd(const a3d_tex_desc* desc, a3d_stream_t stream) {
    TexK k;
    int rc = tex_check(desc, k, __func__);
    if (rc) return rc;
    if ((rc = tex_halving_ok(desc, __func__))) return rc;
    const long long planes = (long long)k.tex_batch * (k.cube ? 6 : 1);
    const bool vec = tex_vec(k);
    for (int l = 1; l < k.levels; ++l) {
        const long long n = planes * k.h[l] * k.w[l] * (vec ? k.C / 4 : k.C);
        if (vec)
            hipLaunchKernelGGL(tex_mip_fwd_kernel<true>, dim3(a3d_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, k.level[l - 1], k.h[l - 1],
                               k.w[l - 1], k.h[l], k.w[l], k.C, n, desc->level[l]);
        else
            hipLaunchKernelGGL(tex_mip_fwd_kernel<false>, dim3(a3d_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, k.level[l - 1], k.h[l - 1],
                               k.w[l - 1], k.h[l], k.w[l], k.C, n, desc->level[l]);
        A3D_LAUNCH_CHECK();
    }
    return A3D_OK;
}

extern "C" int a3d_texture_mip_bwd(const a3d_tex_desc* desc, a3d_stream_t stream) {
    TexK k;
    int rc = tex_check(desc, k, __func__);
    if (rc) return rc;
    if ((rc = tex_halving_ok(desc, __func__))) return rc;
    for (int l = 0; l < k.levels; ++l) A3D_CHECK_ARG(desc->grad[l]);
    const long long planes = (long long)k.tex_batch * (k.cube ? 6 : 1);
    const bool vec = k.C % 4 == 0 && [&] {
        for (int l = 0; l < k.levels; ++l)
            if ((uintptr_t)k.grad[l] % 16) return false;
        return true;
    }();
    for (int l = k.levels - 1; l >= 1; --l) {
        const long long n = planes * k.h[l - 1] * k.w[l - 1] * (vec ? k.C / 4 : k.C);
        if (vec)
            hipLaunchKernelGGL(tex_mip_bwd_kernel<true>, dim3(a3d_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, k.grad[l], k.h[l - 1],
                               k.w[l - 1], k.h[l], k.w[l], k.C, n, k.grad[l - 1]);
        else
            hipLaunchKernelGGL(tex_mip_bwd_kernel<false>, dim3(a3d_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, k.grad[l], k.h[l - 1],
                               k.w[l - 1], k.h[l], k.w[l], k.C, n, k.grad[l - 1]);
        A3D_LAUNCH_CHECK();
    }
    return A3D_OK;
}
