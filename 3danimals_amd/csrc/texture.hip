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
// The lookup itself (descriptor, cube face rule, quads, level of detail) is tex_lookup.h, shared with envshade.hip.
// Generated coordinates (uv == NULL): the forward and backward kernels are also instantiated with the coordinates computed from the
// element index -- the environment-probe resamplers latlong_to_cubemap / cubemap_to_latlong in one launch each way (tex_lookup.h UvSrc).
#include "a3d_common.h"
#include "tex_lookup.h"
#include "tile_scatter.h"

namespace {

// GEN: the coordinates are generated from the element index of the [B, gh, gw] grid instead of read from uv (tex_lookup.h UvSrc)
template <bool VEC, bool GEN>
__global__ __launch_bounds__(256) void tex_fwd_kernel(const TexK k, const float* __restrict__ uv_ptr, const float* __restrict__ uv_da,
                                                      const float* __restrict__ bias, long long n, long long per_image, int gh, int gw,
                                                      float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const UvSrc<GEN> uv{uv_ptr, gh, gw};
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
template <bool VEC, bool GEN>
__global__ __launch_bounds__(256) void tex_bwd_kernel(const TexK k, const float* __restrict__ g_out, const float* __restrict__ uv_ptr,
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
    const UvSrc<GEN> uv{uv_ptr, H, W};
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
    if (!GEN && L.valid && !nearest) {  // (generated coordinates have no gradient of their own: only the texel scatter below)
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

// uv == NULL: the coordinates are generated (include/a3d.h).  Every rule is checked before any launch and named in the message.
int tex_generated_check(const TexK& k, const void* uv_da, const void* bias, const void* g_uv, const void* g_uv_da, const void* g_bias, int B,
                        const char* fn) {
    const char* rule = nullptr;
    if (uv_da || bias || g_uv_da || g_bias) rule = "uv_da, bias and their gradients must be NULL";
    else if (g_uv) rule = "g_uv must be NULL";
    else if (k.filter != A3D_TEX_LINEAR) rule = "filter must be A3D_TEX_LINEAR";
    else if (k.levels != 1) rule = "only level 0 is read: levels must be 1";
    else if (k.boundary != A3D_TEX_WRAP && k.boundary != A3D_TEX_CUBE) rule = "boundary must be A3D_TEX_WRAP (lat-long -> cube) or A3D_TEX_CUBE (cube -> lat-long)";
    else if (!k.cube && k.tex_batch != 1) rule = "a 2-D texture needs tex_batch == 1";
    else if (!k.cube && B != 6) rule = "a 2-D texture needs B == 6 (the faces of the cube)";
    else if (k.cube && B != k.tex_batch) rule = "a cube texture needs B == tex_batch";
    if (!rule) return A3D_OK;
    a3d_set_error("%s: invalid argument: generated coordinates (uv == NULL): %s", fn, rule);
    return A3D_EINVAL;
}

}  // namespace

extern "C" int a3d_texture_fwd(const a3d_tex_desc* desc, const float* uv, const float* uv_da_or_null, const float* bias_or_null, int B, int H,
                               int W, float* out, a3d_stream_t stream) {
    TexK k;
    const int rc = tex_check(desc, k, __func__);
    if (rc) return rc;
    A3D_CHECK_ARG(out && B > 0 && H > 0 && W > 0);
    if (!uv) {
        const int rg = tex_generated_check(k, uv_da_or_null, bias_or_null, nullptr, nullptr, nullptr, B, __func__);
        if (rg) return rg;
    }
    A3D_CHECK_ARG(k.tex_batch == 1 || k.tex_batch == B);
    const long long per_image = (long long)H * W, n = per_image * B;
    const bool vec = tex_vec(k) && (uintptr_t)out % 16 == 0;
    const dim3 grid(a3d_div_up(n, 256));
#define TEX_FWD(VEC, GEN)                                                                                                                \
    hipLaunchKernelGGL((tex_fwd_kernel<VEC, GEN>), grid, dim3(256), 0, (hipStream_t)stream, k, uv, uv_da_or_null, bias_or_null, n, per_image, H, \
                       W, out)
    if (uv) {
        if (vec) TEX_FWD(true, false); else TEX_FWD(false, false);
    } else {
        if (vec) TEX_FWD(true, true); else TEX_FWD(false, true);
    }
#undef TEX_FWD
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_texture_bwd(const a3d_tex_desc* desc, const float* g_out, const float* uv, const float* uv_da_or_null,
                               const float* bias_or_null, int B, int H, int W, float* g_uv_or_null, float* g_uv_da_or_null, float* g_bias_or_null,
                               a3d_stream_t stream) {
    TexK k;
    const int rc = tex_check(desc, k, __func__);
    if (rc) return rc;
    A3D_CHECK_ARG(g_out && B > 0 && H > 0 && W > 0);
    if (!uv) {
        const int rg = tex_generated_check(k, uv_da_or_null, bias_or_null, g_uv_or_null, g_uv_da_or_null, g_bias_or_null, B, __func__);
        if (rg) return rg;
    }
    A3D_CHECK_ARG(k.tex_batch == 1 || k.tex_batch == B);
    A3D_CHECK_ARG(!g_uv_da_or_null || uv_da_or_null);
    A3D_CHECK_ARG(!g_bias_or_null || bias_or_null);
    const long long n = (long long)H * W * B;
    const int tiles_x = a3d_div_up(W, 8), tiles_y = a3d_div_up(H, 8);
    const long long waves = W >= 8 ? (long long)tiles_x * tiles_y * B : (n + 63) / 64;
    const bool vec = tex_vec(k) && (uintptr_t)g_out % 16 == 0;
    const dim3 grid(a3d_div_up(waves, 4));
#define TEX_BWD(VEC, GEN)                                                                                                                  \
    hipLaunchKernelGGL((tex_bwd_kernel<VEC, GEN>), grid, dim3(256), 0, (hipStream_t)stream, k, g_out, uv, uv_da_or_null, bias_or_null, B, H, W, \
                       tiles_x, tiles_y, g_uv_or_null, g_uv_da_or_null, g_bias_or_null)
    if (uv) {
        if (vec) TEX_BWD(true, false); else TEX_BWD(false, false);
    } else {
        if (vec) TEX_BWD(true, true); else TEX_BWD(false, true);
    }
#undef TEX_BWD
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
