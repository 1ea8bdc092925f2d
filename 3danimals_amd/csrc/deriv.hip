// Image-space derivatives on gfx950 (include/a3d_deriv.h): the second output of dr.rasterize (rast_db) and of dr.interpolate with
// rast_db / diff_attrs (out_da), forward and backward -- the two operators that produce uv_da for dr.texture.
//
// Forward kernels: one lane per pixel.  16 B of raster texel read (coalesced), three index loads, 48 B of clip-space vertices (or 3 S
// attribute values) gathered from the L2-resident vertex array -- neighbouring pixels are mostly on the same triangle -- and one 16-byte
// row written (16-byte pieces of the 8 S-byte row where S is even).  HBM traffic per pixel: 16 + 16 B (rast_db), 32 + 8 S B (out_da).
// Backward kernels: one thread per pixel of a 16 x 16 tile; the forward is recomputed, the three gradient rows of a pixel merge with the
// rows of the lanes on the same triangle (ts_merge), meet their neighbours' in the work-group's LDS table and leave as one row of adjacent
// atomics per vertex and tile (tile_scatter.h) -- the scheme of a3d_rast_bwd / a3d_interp_bwd.  The arithmetic is specified operation by
// operation (deriv_math.h; -ffp-contract=off).
#include "a3d_common.h"
#include "../../include/a3d_deriv.h"
#include "tile_scatter.h"
#include "deriv_math.h"

#define DV_MAXC 64  // (IP_MAXC of interp.hip)

// the stored triangle's clip-space corners and the pixel's set-up; false where s == 0 (a triangle that is edge-on AT this pixel centre:
// the rasteriser never stores one; a fabricated raster gets zeros instead of 0 / 0)
__device__ __forceinline__ bool dv_load(const float4* __restrict__ clip, long long vb, const int* __restrict__ tri, int f, int px, int py,
                                        float kx, float ky, DvPixel& d, float& fx, float& fy, int (&idx)[3]) {
    idx[0] = tri[3 * f]; idx[1] = tri[3 * f + 1]; idx[2] = tri[3 * f + 2];
    const float4 p0 = clip[vb + idx[0]], p1 = clip[vb + idx[1]], p2 = clip[vb + idx[2]];
    const float x[3] = {p0.x, p1.x, p2.x}, y[3] = {p0.y, p1.y, p2.y}, w[3] = {p0.w, p1.w, p2.w};
    fx = ((float)px + 0.5f) * kx - 1.f;
    fy = ((float)py + 0.5f) * ky - 1.f;
    dv_setup(x, y, w, fx, fy, d);
    return d.s != 0.f;
}

__global__ __launch_bounds__(256) void dv_rast_db_fwd_kernel(const float4* __restrict__ clip, int clip_batch, const int* __restrict__ tri,
                                                             const float4* __restrict__ rast, int V, int F, int H, int W, long long npix,
                                                             float4* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int f = (int)rast[i].w - 1;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (f >= 0 && f < F) {
        const int px = (int)(i % W), py = (int)((i / W) % H);
        const long long vb = clip_batch == 1 ? 0ll : (i / ((long long)H * W)) * V;
        const float kx = 2.f / (float)W, ky = 2.f / (float)H;
        DvPixel d;
        float fx, fy;
        int idx[3];
        if (dv_load(clip, vb, tri, f, px, py, kx, ky, d, fx, fy, idx)) dv_forward(d, kx, ky, o);
    }
    out[i] = make_float4(o[0], o[1], o[2], o[3]);
}

// g_db [B,H,W,4] -> g_clip [B|1,V,4] (x, y, -, w): rs_bwd_kernel's shape (raster.hip) around dv_backward
__global__ __launch_bounds__(256) void dv_rast_db_bwd_kernel(const float4* __restrict__ g_db, const float4* __restrict__ clip, int clip_batch,
                                                             const int* __restrict__ tri, const float4* __restrict__ rast, int V, int F, int H,
                                                             int W, int tiles_x, float* __restrict__ g_clip) {
    extern __shared__ __align__(16) unsigned char dv_bwd_lds[];
    const int b = blockIdx.y, tile = blockIdx.x;
    int px, py;
    ts_pixel((tile % tiles_x) * TS_TILE, (tile / tiles_x) * TS_TILE, px, py);
    const bool inside = px < W && py < H;
    const long long i = ((long long)b * H + py) * W + px;
    int f = -1;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) f = (int)rast[i].w - 1;
    bool live = inside && f >= 0 && f < F;
    if (live) {
        g = g_db[i];
        live = g.x != 0.f || g.y != 0.f || g.z != 0.f || g.w != 0.f;
    }
    if (!__syncthreads_or(live)) return;
    TileScatter ts;
    ts.init(dv_bwd_lds, 4);
    const int vb = clip_batch == 1 ? 0 : b * V;
    int idx[3] = {0, 0, 0}, key = -1;
    float c[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // (x, y, w) of the three corners
    if (live) {
        const float kx = 2.f / (float)W, ky = 2.f / (float)H;
        DvPixel d;
        float fx, fy;
        if (dv_load(clip, vb, tri, f, px, py, kx, ky, d, fx, fy, idx)) {
            const float gg[4] = {g.x, g.y, g.z, g.w};
            dv_backward(d, kx, ky, fx, fy, gg, c);
            key = f;
        }
    }
    ts_merge<9, 6>(key, c);
    __syncthreads();  // (table initialised)
    const int e0 = ts.entries(key >= 0, 3);
    if (key >= 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int row = vb + idx[k];
            const int sl = ts.slot(row);
            if (sl >= 0) {
                *reinterpret_cast<float4*>(ts.e_val + 4 * (e0 + k)) = make_float4(c[3 * k], c[3 * k + 1], 0.f, c[3 * k + 2]);
                ts.link(e0 + k, sl);
            } else {
                float* o = g_clip + (long long)row * 4;
                atomicAdd(o, c[3 * k]); atomicAdd(o + 1, c[3 * k + 1]); atomicAdd(o + 3, c[3 * k + 2]);
            }
        }
    }
    __syncthreads();
    ts.flush<4>(g_clip, 4, 2);
}

// channel of selected attribute s (sel == nullptr: 'all', s itself); -1 for an index outside [0, C): it then reads and adds nothing
__device__ __forceinline__ int dv_channel(const int* __restrict__ sel, int s, int C) {
    const int ch = sel ? sel[s] : s;
    return (unsigned)ch < (unsigned)C ? ch : -1;
}

// out_da [B,H,W,2S] = (dA/dX, dA/dY) per selected attribute: dA/dX = du/dX (A0 - A2) + dv/dX (A1 - A2).  VEC: S even, 16-byte stores.
template <bool VEC>
__global__ __launch_bounds__(256) void dv_interp_da_fwd_kernel(const float* __restrict__ attr, int attr_batch, int C, const int* __restrict__ sel,
                                                               int S, const float4* __restrict__ rast, const float4* __restrict__ rast_db,
                                                               const int* __restrict__ tri, int V, int F, long long hw, long long npix,
                                                               float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int f = (int)rast[i].w - 1;
    float* o = out + i * 2 * S;
    if (f < 0 || f >= F) {
        if (VEC) {
            for (int s = 0; s < S; s += 2) *reinterpret_cast<float4*>(o + 2 * s) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int s = 0; s < 2 * S; ++s) o[s] = 0.f;
        }
        return;
    }
    const float4 db = rast_db[i];
    const long long vb = attr_batch == 1 ? 0ll : (i / hw) * V;
    const float* a0 = attr + (vb + tri[3 * f]) * C;
    const float* a1 = attr + (vb + tri[3 * f + 1]) * C;
    const float* a2 = attr + (vb + tri[3 * f + 2]) * C;
    float v[4];
    for (int s = 0; s < S; s += (VEC ? 2 : 1)) {
#pragma unroll
        for (int t = 0; t < (VEC ? 2 : 1); ++t) {
            const int ch = dv_channel(sel, s + t, C);
            float d0 = 0.f, d1 = 0.f;
            if (ch >= 0) {
                const float x2 = a2[ch];
                d0 = a0[ch] - x2;
                d1 = a1[ch] - x2;
            }
            v[2 * t] = db.x * d0 + db.z * d1;
            v[2 * t + 1] = db.y * d0 + db.w * d1;
        }
        if (VEC) {
            *reinterpret_cast<float4*>(o + 2 * s) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            o[2 * s] = v[0];
            o[2 * s + 1] = v[1];
        }
    }
}

// what one pixel hands back for selected attribute s: the four sums of g_rast_db and the rows of vertex 0 and 1 (vertex 2 = -(t0 + t1))
__device__ __forceinline__ void dv_da_term(const float4 db, float gX, float gY, float d0, float d1, float4& gd, float& t0, float& t1) {
    gd.x += gX * d0; gd.y += gY * d0; gd.z += gX * d1; gd.w += gY * d1;
    t0 = db.x * gX + db.y * gY;
    t1 = db.z * gX + db.w * gY;
}

// S <= 16: the tile scatter over rows of the S SELECTED columns (SM = S rounded up: register rows); the flush maps column s to channel
// sel[s], so a channel listed twice receives both columns and an unselected channel keeps the callee's zero.
template <int SM, int ROUNDS>
__global__ __launch_bounds__(256) void dv_interp_da_bwd_tile_kernel(const float* __restrict__ g_da, const float* __restrict__ attr, int attr_batch,
                                                                    int C, const int* __restrict__ sel, int S, const float4* __restrict__ rast,
                                                                    const float4* __restrict__ rast_db, const int* __restrict__ tri, int V, int F,
                                                                    int H, int W, int tiles_x, float* __restrict__ g_attr,
                                                                    float4* __restrict__ g_rast_db) {
    extern __shared__ __align__(16) unsigned char dv_da_lds[];
    const int b = blockIdx.y, tile = blockIdx.x;
    int px, py;
    ts_pixel((tile % tiles_x) * TS_TILE, (tile / tiles_x) * TS_TILE, px, py);
    const bool inside = px < W && py < H;
    const long long i = ((long long)b * H + py) * W + px;
    int f = -1;
    if (inside) f = (int)rast[i].w - 1;
    const bool live = inside && f >= 0 && f < F;
    if (!__syncthreads_or(live)) {
        if (inside && g_rast_db) g_rast_db[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    TileScatter ts;
    if (g_attr) ts.init(dv_da_lds, S);
    float4 gd = make_float4(0.f, 0.f, 0.f, 0.f);
    float c[3 * SM];
#pragma unroll
    for (int n = 0; n < 3 * SM; ++n) c[n] = 0.f;
    int row[3] = {0, 0, 0}, key = -1;
    if (live) {
        const float4 db = rast_db[i];
        const int vb = attr_batch == 1 ? 0 : b * V;
        row[0] = vb + tri[3 * f]; row[1] = vb + tri[3 * f + 1]; row[2] = vb + tri[3 * f + 2];
        const float* a0 = attr + (long long)row[0] * C;
        const float* a1 = attr + (long long)row[1] * C;
        const float* a2 = attr + (long long)row[2] * C;
        const float* g = g_da + i * 2 * S;
#pragma unroll
        for (int s = 0; s < SM; ++s) {
            if (s < S) {
                const int ch = dv_channel(sel, s, C);
                if (ch >= 0) {
                    const float x2 = a2[ch];
                    float t0, t1;
                    dv_da_term(db, g[2 * s], g[2 * s + 1], a0[ch] - x2, a1[ch] - x2, gd, t0, t1);
                    c[s] = t0; c[SM + s] = t1; c[2 * SM + s] = -(t0 + t1);
                }
            }
        }
        key = f;
    }
    if (inside && g_rast_db) g_rast_db[i] = gd;
    if (!g_attr) return;
    ts_merge<3 * SM, ROUNDS>(key, c);
    __syncthreads();  // (table initialised)
    const int e0 = ts.entries(key >= 0, 3);
    if (key >= 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int sl = ts.slot(row[k]);
#pragma unroll
            for (int s = 0; s < SM; ++s) {
                if (s < S) {
                    const float v = c[k * SM + s];
                    if (sl >= 0) {
                        ts.e_val[(e0 + k) * S + s] = v;
                    } else if (v != 0.f) {
                        const int ch = dv_channel(sel, s, C);
                        if (ch >= 0) atomicAdd(g_attr + (long long)row[k] * C + ch, v);
                    }
                }
            }
            if (sl >= 0) ts.link(e0 + k, sl);
        }
    }
    __syncthreads();
    // (an index outside [0, C) staged zeros only, and the flush adds no zero sum: its column's target is never formed into an address)
    ts.flush<SM>(g_attr, C, -1, sel);
}

// S > 16 (more selected attributes than the tile kernel keeps in registers): one thread per pixel, three atomics per selected attribute
__global__ __launch_bounds__(256) void dv_interp_da_bwd_pixel_kernel(const float* __restrict__ g_da, const float* __restrict__ attr, int attr_batch,
                                                                     int C, const int* __restrict__ sel, int S, const float4* __restrict__ rast,
                                                                     const float4* __restrict__ rast_db, const int* __restrict__ tri, int V, int F,
                                                                     long long hw, long long npix, float* __restrict__ g_attr,
                                                                     float4* __restrict__ g_rast_db) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int f = (int)rast[i].w - 1;
    float4 gd = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f >= 0 && f < F) {
        const float4 db = rast_db[i];
        const long long vb = attr_batch == 1 ? 0ll : (i / hw) * V;
        const long long o0 = (vb + tri[3 * f]) * C, o1 = (vb + tri[3 * f + 1]) * C, o2 = (vb + tri[3 * f + 2]) * C;
        const float* g = g_da + i * 2 * S;
        for (int s = 0; s < S; ++s) {
            const int ch = dv_channel(sel, s, C);
            if (ch < 0) continue;
            const float x2 = attr[o2 + ch];
            float t0, t1;
            dv_da_term(db, g[2 * s], g[2 * s + 1], attr[o0 + ch] - x2, attr[o1 + ch] - x2, gd, t0, t1);
            if (g_attr && (t0 != 0.f || t1 != 0.f)) {
                atomicAdd(g_attr + o0 + ch, t0);
                atomicAdd(g_attr + o1 + ch, t1);
                atomicAdd(g_attr + o2 + ch, -(t0 + t1));
            }
        }
    }
    if (g_rast_db) g_rast_db[i] = gd;
}

#define DV_CHECK_FRAME()                                                                                   \
    A3D_CHECK_ARG(B > 0 && V > 0 && F >= 0 && H > 0 && W > 0);                                             \
    A3D_CHECK_ARG(F == 0 || tri);                                                                          \
    A3D_CHECK_ARG((long long)B * H * W < 0x7fffffffll && B <= 65535 && (long long)B * V < 0x7fffffffll)

extern "C" int a3d_rast_db_fwd(const float* clip, int clip_batch, const int32_t* tri, const float* rast, int B, int V, int F, int H, int W,
                               float* rast_db, a3d_stream_t stream) {
    A3D_CHECK_ARG(clip && rast && rast_db);
    DV_CHECK_FRAME();
    A3D_CHECK_ARG(clip_batch == 1 || clip_batch == B);
    const long long npix = (long long)B * H * W;
    hipLaunchKernelGGL(dv_rast_db_fwd_kernel, dim3(a3d_div_up(npix, 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)clip, clip_batch, tri,
                       (const float4*)rast, V, F, H, W, npix, (float4*)rast_db);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_rast_db_bwd(const float* g_db, const float* clip, int clip_batch, const int32_t* tri, const float* rast, int B, int V, int F,
                               int H, int W, float* g_clip, a3d_stream_t stream) {
    A3D_CHECK_ARG(g_db && clip && rast && g_clip);
    DV_CHECK_FRAME();
    A3D_CHECK_ARG(clip_batch == 1 || clip_batch == B);
    hipStream_t s = (hipStream_t)stream;
    A3D_HIP(hipMemsetAsync(g_clip, 0, sizeof(float) * 4 * (size_t)clip_batch * V, s));
    if (F == 0) return A3D_OK;
    const int tiles_x = a3d_div_up(W, TS_TILE), tiles_y = a3d_div_up(H, TS_TILE);
    hipLaunchKernelGGL(dv_rast_db_bwd_kernel, dim3(tiles_x * tiles_y, B), dim3(256), TileScatter::lds_bytes(4), s, (const float4*)g_db,
                       (const float4*)clip, clip_batch, tri, (const float4*)rast, V, F, H, W, tiles_x, g_clip);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_interp_da_fwd(const float* attr, int attr_batch, int C, const int32_t* sel_or_null, int S, const float* rast,
                                 const float* rast_db, const int32_t* tri, int B, int V, int F, int H, int W, float* out_da,
                                 a3d_stream_t stream) {
    A3D_CHECK_ARG(attr && rast && rast_db && out_da && C > 0 && C <= DV_MAXC && S > 0 && S <= A3D_DERIV_MAX_SELECTED);
    A3D_CHECK_ARG(sel_or_null || S == C);
    DV_CHECK_FRAME();
    A3D_CHECK_ARG(attr_batch == 1 || attr_batch == B);
    const long long hw = (long long)H * W, npix = hw * B;
#define DV_FWD(VEC_)                                                                                                                          \
    hipLaunchKernelGGL(dv_interp_da_fwd_kernel<VEC_>, dim3(a3d_div_up(npix, 256)), dim3(256), 0, (hipStream_t)stream, attr, attr_batch, C,    \
                       sel_or_null, S, (const float4*)rast, (const float4*)rast_db, tri, V, F, hw, npix, out_da)
    if (S % 2 == 0) DV_FWD(true); else DV_FWD(false);
#undef DV_FWD
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_interp_da_bwd(const float* g_da, const float* attr, int attr_batch, int C, const int32_t* sel_or_null, int S,
                                 const float* rast, const float* rast_db, const int32_t* tri, int B, int V, int F, int H, int W,
                                 float* g_attr_or_null, float* g_rast_db_or_null, a3d_stream_t stream) {
    A3D_CHECK_ARG(g_da && attr && rast && rast_db && C > 0 && C <= DV_MAXC && S > 0 && S <= A3D_DERIV_MAX_SELECTED);
    A3D_CHECK_ARG(sel_or_null || S == C);
    A3D_CHECK_ARG(g_attr_or_null || g_rast_db_or_null);
    DV_CHECK_FRAME();
    A3D_CHECK_ARG(attr_batch == 1 || attr_batch == B);
    hipStream_t s = (hipStream_t)stream;
    if (g_attr_or_null) A3D_HIP(hipMemsetAsync(g_attr_or_null, 0, sizeof(float) * (size_t)attr_batch * V * C, s));
    const long long hw = (long long)H * W, npix = hw * B;
    if (S <= 16) {
        const int tiles_x = a3d_div_up(W, TS_TILE), tiles_y = a3d_div_up(H, TS_TILE);
#define DV_TILE(SM_, R_)                                                                                                                     \
    hipLaunchKernelGGL((dv_interp_da_bwd_tile_kernel<SM_, R_>), dim3(tiles_x * tiles_y, B), dim3(256),                                       \
                       g_attr_or_null ? TileScatter::lds_bytes(S) : 0, s, g_da, attr, attr_batch, C, sel_or_null, S, (const float4*)rast,    \
                       (const float4*)rast_db, tri, V, F, H, W, tiles_x, g_attr_or_null, (float4*)g_rast_db_or_null)
        if (S <= 4) DV_TILE(4, 6); else if (S <= 8) DV_TILE(8, 4); else DV_TILE(16, 4);
#undef DV_TILE
    } else {
        hipLaunchKernelGGL(dv_interp_da_bwd_pixel_kernel, dim3(a3d_div_up(npix, 256)), dim3(256), 0, s, g_da, attr, attr_batch, C, sel_or_null, S,
                           (const float4*)rast, (const float4*)rast_db, tri, V, F, hw, npix, g_attr_or_null, (float4*)g_rast_db_or_null);
    }
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

A3D_PROFILE_TU(deriv)
