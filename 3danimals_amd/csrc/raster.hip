// Rasteriser on gfx950: triangle-parallel depth test with 64-bit atomics, then a pixel-parallel resolve.
//
// Replaces dr.DepthPeeler(...).rasterize_next_layer() / dr.rasterize (model/render/render.py:292-294, :351;
// nvdiffrast, third party, goes through OpenGL).  The meshes on this path are marching-tets surfaces: tens of
// thousands of triangles per 256x256 image whose pixel boxes hold ~10 candidates and ~2 covered pixels each.
//
//   clear   : keys[B,H,W] (u64) <- ~0       (hipMemsetAsync, 8 B/pixel; skipped when the caller hands back the buffer of the
//             previous call on the same stream: the resolve re-arms every key it consumes)
//   tri     : 4 lanes per (image, triangle): 12 B of indices + 3 x 16 B vertex gathers (L2 resident), the
//             conservative pixel box; the candidate pixels of a wave's 16 triangles are then POOLED (prefix of the box sizes,
//             triangle data through LDS) and dealt out evenly over the 64 lanes; every covered pixel
//             does atomicMin(keys[pixel], order(z/w) << 32 | id).  min over (depth, id) is order independent, so
//             the image is deterministic with no sorting or binning, and the work is balanced over all 256 CUs
//             no matter where on screen the object is.  Boxes above 64 px are found with a ballot and
//             rasterised cooperatively by the whole wave.
//   resolve : 1 thread per pixel: key -> winner's barycentrics recomputed -> float4 texel, fully coalesced.
//
// Two LDS-tile designs were measured first on the bench workload (B=16, F=11.5k, 256x256; rocprofv3):
// workgroup-per-64x64-tile scanning all triangles 277 us; 32x32 tiles + per-triangle box pre-pass +
// 4-lanes-per-survivor 108 us, of which 85 us was fragment work serialised in the quarter of the tiles the object
// covers (4 waves each).  The triangle-parallel form removes that imbalance ("Rasteriser").
// HBM traffic per image: 16 B/vertex + 12 B/face in, 16 B/pixel out, + 8 B/pixel of keys written, updated in L2
// and read once.  The per-fragment arithmetic mirrors oracle/raster_ref.c operation by operation; this TU is
// compiled with -ffp-contract=off so that the edge functions of a shared edge are exact negations (watertight)
// and the triangle ids match the oracle bit for bit.
#include "a3d_common.h"
#include "tile_scatter.h"
#include "raster_common.h"
#include "topo_common.h"
#include "normals_common.h"
#include "cover_common.h"
#include "gbuffer_common.h"

#define RS_EMPTY 0xFFFFFFFFFFFFFFFFull
#define RS_BIG 512          // boxes above this many pixels go through the tile stage
#define RS_TILE_CHUNK 512   // tiles tested per round of the work-group (survivors <= this: the LDS list cannot overflow)
// absolute part of the tile test's and the row span's ``tol``: below 2^-126 a float carries an absolute error of up to 2^-150 per
// operation, not a relative one, and a tolerance that is a fraction of the products' size vanishes with them -- next to a vertex
// whose w is denormal the edge functions live there (~13 roundings each in the culls' polynomial and in rs_frag: ~28 denormal steps)
#define RS_TOL_ABS 4e-44f

// the vertex-normals job that may ride in the triangle launch (a3d_rast_fwd: normals_*)
struct RsNormalsJob {
    const float *v_a, *v_b;
    const int *off, *adj;
    float *acc_a, *nrm_a, *acc_b, *nrm_b;
    int B_a, B_b, wg_per_row, stride;  // stride: layout of off / adj (topo_common.h: vf_list), also of topo_off / topo_adj
};

struct RsFrag {
    float u, v, zw;
    bool hit;
    bool pos;  // sign of the triangle's screen-space area (s > 0)
};

// Fragment test; same operations in the same order as frag() in oracle/raster_ref.c (branch-light form).
__device__ __forceinline__ RsFrag rs_frag(const float4 p0, const float4 p1, const float4 p2, float fx, float fy) {
    RsFrag r;
    r.u = 0.f; r.v = 0.f; r.zw = 0.f; r.hit = false; r.pos = false;
    const float q0x = __builtin_fmaf(-fx, p0.w, p0.x), q0y = __builtin_fmaf(-fy, p0.w, p0.y);
    const float q1x = __builtin_fmaf(-fx, p1.w, p1.x), q1y = __builtin_fmaf(-fy, p1.w, p1.y);
    const float q2x = __builtin_fmaf(-fx, p2.w, p2.x), q2y = __builtin_fmaf(-fy, p2.w, p2.y);
    const float a0 = q1x * q2y - q1y * q2x;
    const float a1 = q2x * q0y - q2y * q0x;
    const float a2 = q0x * q1y - q0y * q1x;
    const float s = (a0 + a1) + a2;
    const float sg = s > 0.f ? 1.f : -1.f;
    const float e0 = a0 * sg, e1 = a1 * sg, e2 = a2 * sg;
    bool in = (s != 0.f) && (s == s) && (e0 >= 0.f) && (e1 >= 0.f) && (e2 >= 0.f);  // NaN fails every comparison
    if (in && (e0 == 0.f || e1 == 0.f || e2 == 0.f)) {
        // pixel centre exactly on an edge line (rare): the owner is decided by the sign of the line's normal
        if (e0 == 0.f) {
            const float A = (p1.y * p2.w - p1.w * p2.y) * sg, B = (p1.w * p2.x - p1.x * p2.w) * sg;
            in = in && (A > 0.f || (A == 0.f && B > 0.f));
        }
        if (e1 == 0.f) {
            const float A = (p2.y * p0.w - p2.w * p0.y) * sg, B = (p2.w * p0.x - p2.x * p0.w) * sg;
            in = in && (A > 0.f || (A == 0.f && B > 0.f));
        }
        if (e2 == 0.f) {
            const float A = (p0.y * p1.w - p0.w * p1.y) * sg, B = (p0.w * p1.x - p0.x * p1.w) * sg;
            in = in && (A > 0.f || (A == 0.f && B > 0.f));
        }
    }
    if (!in) return r;
    const float zn = (p0.z * a0 + p1.z * a1) + p2.z * a2;
    const float wn = (p0.w * a0 + p1.w * a1) + p2.w * a2;
    if (!(wn * sg > 0.f)) return r;
    const float zw = zn / wn;
    if (!(zw >= -1.f && zw <= 1.f)) return r;
    const float iw = 1.f / s;
    r.u = fminf(fmaxf(a0 * iw, 0.f), 1.f);
    r.v = fminf(fmaxf(a1 * iw, 0.f), 1.f);
    r.zw = zw;
    r.hit = true;
    r.pos = s > 0.f;
    return r;
}

// monotone float -> uint.  -0 is taken as +0 first: as bit patterns -0 ranks strictly in front of +0, while the oracle's f.zw < best_z
// holds them equal and gives the pixel to the lower id -- clip-space z = -0 yields z/w = -0 for either winding, and two coplanar
// triangles at +0 and -0 came out by depth instead of by id (tests/raster_cases.py: signed_zero_pair; also in the peel's ``prev`` key)
__device__ __forceinline__ unsigned rs_order(float f) {
    unsigned u = __float_as_uint(f == 0.f ? 0.f : f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (round 6) The columns of pixel row ``py`` a triangle can cover, as a conservative span [xa, xb] inside [xlo, xhi] (xa > xb: none).
// rs_frag's three edge functions are LINEAR in the pixel centre: a_k = C_k + A_k fx + B_k fy (the tile stage below uses the same form);
// on a row, a_k >= 0 is a half-line in fx, the triangle is where all three a_k have one sign.  Both sign cases are solved and their
// hull taken (the sign of the triangle's area is a per-pixel matter under perspective), with the inequalities relaxed by ``tol`` -- the
// rounding of rs_frag's own products, the tile stage's bound -- and the span widened by one pixel either side: the exact test (rs_frag,
// unchanged) still decides every pixel, the span only says where it need not be asked.  A sliver's cost then follows its area +
// perimeter, not its box: 9.45 M box pixels for 3.6e5 covered ones after 600 optimiser steps (profiles/r05_long_run_diag.txt).
__device__ __forceinline__ void rs_row_span(const float4 p0, const float4 p1, const float4 p2, float fy, float xs, float xo, float fx_abs_max,
                                            int xlo, int xhi, int& xa, int& xb) {
    float lo_p = -INFINITY, hi_p = INFINITY, lo_n = -INFINITY, hi_n = INFINITY;
    bool none_p = false, none_n = false;
    const float4 pp[3] = {p0, p1, p2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 u = pp[(k + 1) % 3], v = pp[(k + 2) % 3];
        const float C = u.x * v.y - u.y * v.x, A = -(u.w * v.y - u.y * v.w), Bc = -(u.x * v.w - u.w * v.x);
        const float tol = 5e-6f * ((fabsf(u.x * v.y) + fabsf(u.y * v.x)) + 2.f * (fabsf(u.w * v.y) + fabsf(u.y * v.w)) + 2.f * (fabsf(u.x * v.w) + fabsf(u.w * v.x))
                                   + 2.f * fabsf(u.w * v.w) * fx_abs_max * fabsf(fy)) + RS_TOL_ABS;
        const float D = C + Bc * fy;
        if (A != 0.f) {
            const float rA = 1.f / A;
            const float tp = (-tol - D) * rA, tn = (tol - D) * rA;  // a_k >= -tol  <=>  A fx >= -tol - D ;  a_k <= tol  <=>  A fx <= tol - D
            // (|A| so small that its reciprocal overflows -- an edge at a vertex with a denormal w --: tp, tn are +-inf whatever the true
            // quotients, and an inf on the wrong side emptied the span; such an edge bounds nothing here)
            if (fabsf(rA) < INFINITY) {
                if (A > 0.f) { lo_p = fmaxf(lo_p, tp); hi_n = fminf(hi_n, tn); }
                else { hi_p = fminf(hi_p, tp); lo_n = fmaxf(lo_n, tn); }
            }
        } else {
            none_p = none_p || (D < -tol);
            none_n = none_n || (D > tol);
        }
    }
    none_p = none_p || !(lo_p <= hi_p);
    none_n = none_n || !(lo_n <= hi_n);
    const float lo = none_p ? (none_n ? INFINITY : lo_n) : (none_n ? lo_p : fminf(lo_p, lo_n));
    const float hi = none_p ? (none_n ? -INFINITY : hi_n) : (none_n ? hi_p : fmaxf(hi_p, hi_n));
    // pixel column of an NDC x: (fx - xo) / xs; one pixel of margin either side, clamped to the box in float before the conversion
    const float ixs = 1.f / xs;
    const float ca = fminf(fmaxf(floorf((lo - xo) * ixs) - 1.f, (float)xlo), (float)xhi + 1.f);
    const float cb = fmaxf(fminf(ceilf((hi - xo) * ixs) + 1.f, (float)xhi), (float)xlo - 1.f);
    xa = (int)ca;
    xb = (int)cb;
}

// ``prev`` (depth peeling, layer n > 0): the texels of the previous layer of this image; only fragments strictly behind the previous
// layer's (depth, id) survive, pixels the previous layer left empty stay empty
__device__ __forceinline__ void rs_test_pixel(const float4 p0, const float4 p1, const float4 p2, int px, int py, int W, float xs, float xo,
                                              float ys, float yo, unsigned f, unsigned long long* __restrict__ keys,
                                              const float4* __restrict__ prev) {
    const RsFrag fr = rs_frag(p0, p1, p2, __builtin_fmaf(xs, (float)px, xo), __builtin_fmaf(ys, (float)py, yo));
    if (fr.hit) {
        const unsigned long long key = ((unsigned long long)rs_order(fr.zw) << 32) | f;
        if (prev) {
            const float4 pr = prev[(long long)py * W + px];
            if (!(pr.w > 0.f)) return;
            const unsigned long long key_prev = ((unsigned long long)rs_order(pr.z) << 32) | (unsigned)((int)pr.w - 1);
            if (key <= key_prev) return;
        }
        unsigned long long* slot = keys + (long long)py * W + px;
        // fire and forget.  (Reading the key first to skip atomics that cannot win looked like a saving and measured as a loss: the
        // dependent 8-byte read costs more than the ~50 % of atomics it removes -- 42.7 us with the filter, 33.0 us without.)
        atomicMin(slot, key);
    }
}

// LPT lanes per (image, triangle); blockDim = 256 = 256 / LPT triangles.
template <int LPT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void rs_tri_kernel(const float4* __restrict__ clip, int clip_batch, const int* __restrict__ tri, int V, int F,
                                                     int H, int W, unsigned long long* __restrict__ keys, const float4* __restrict__ prev,
                                                     int nb_tri, float2* __restrict__ aa_screen, int* __restrict__ aa_count, int aa_shards,
                                                     int* __restrict__ cover_group_sum, int cover_groups, int nb_screen,
                                                     const int* __restrict__ topo_off, const int* __restrict__ topo_adj,
                                                     int* __restrict__ topo_opp, int nb_opp, RsNormalsJob nj) {
    const int b = blockIdx.y;
    A3D_STAMP(0, 0);  // (A3D_STAMP kernel ids of this file: 0 = rs_tri_kernel -- triangle work-groups only stamp 1..5 --, 1 = rs_resolve_kernel)
    // the riding jobs (dependent-gather chains: vertex normals, opposite-vertex table, screen positions) are DISPATCHED FIRST:
    // their round trips then run under the triangle work instead of as the launch's tail.  bx = the work-group's index in the order the
    // branches below are written in (triangles first).
    const int n_extra = (int)gridDim.x - nb_tri;
    const int bx = (int)blockIdx.x < n_extra ? nb_tri + (int)blockIdx.x : (int)blockIdx.x - n_extra;
    if (bx >= nb_tri + nb_screen + nb_opp) {
        // yet more extra work-groups: the vertex normals of the mesh being rasterised (and of a second, small vertex array over the same
        // triangle list) -- normals.hip's forward pass, which the G-buffer pass of this frame reads next.  As a launch of its own it is
        // 9 us of dependent gathers plus a launch gap on a latency-bound stretch; here it runs beside the triangle work, which is bound
        // by the memory-side atomics and leaves the gather path idle.  Batches of 4 index rows keep this branch inside the triangle
        // path's register budget.
        const int j = (int)blockIdx.y * nj.wg_per_row + (bx - nb_tri - nb_screen - nb_opp);  // flat work-group of the job
        const int nbv = (V + 255) / 256;
        if (j >= nbv * (nj.B_a + nj.B_b)) return;
        const int image = j / nbv, vi = (j - image * nbv) * 256 + (int)threadIdx.x;
        if (vi >= V) return;
        if (image < nj.B_a) nr_fwd_vertex<4>(nj.v_a + (long long)image * V * 3, tri, nj.off, nj.adj, nj.stride, F, vi, nj.acc_a, nj.nrm_a, ((long long)image * V + vi) * 3);
        else nr_fwd_vertex<4>(nj.v_b + (long long)(image - nj.B_a) * V * 3, tri, nj.off, nj.adj, nj.stride, F, vi, nj.acc_b, nj.nrm_b, ((long long)(image - nj.B_a) * V + vi) * 3);
        return;
    }
    if (bx >= nb_tri + nb_screen) {
        // more extra work-groups: the opposite-vertex table of the silhouette analysis (one per mesh, not per image: its ceil(3 F / 256)
        // work-groups are spread over the B rows of the grid, nb_opp per row -- as "image 0 only" every other row carried that many
        // work-groups that left at once, 2085 of the launch's 5856 on the bench mesh, all dispatched before the triangle work), looked up
        // in the vertex -> face lists the DMTet extraction left (no edge hash on that path).  Each lookup is a chain of five dependent
        // gathers -- inside the analysis it doubled that kernel's time (13 -> 24 us); here it runs beside the triangle work for free.
        const int idx = ((int)blockIdx.y * nb_opp + (bx - nb_tri - nb_screen)) * 256 + threadIdx.x;
        if (idx < 3 * F) topo_opp[idx] = aa_opposite_from_lists(tri, topo_off, topo_adj, nj.stride, F, idx / 3, idx - 3 * (idx / 3));
        return;
    }
    // the covered-pixel list's group sums, accumulated by the resolve launch that follows: zeroed here (no memset launch)
    if (cover_group_sum && bx == 0 && b == 0)
        for (int i = threadIdx.x; i < cover_groups; i += blockDim.x) cover_group_sum[i] = 0;
    if (bx >= nb_tri) {
        // extra work-groups: what the silhouette analysis of this frame needs first -- pixel-space vertex positions, once per (image,
        // vertex), with the operations of antialias.hip's aa_screen_kernel (p.x / p.w * W/2, unfused), and its append counters at zero
        if (b == 0 && bx == nb_tri && (int)threadIdx.x < aa_shards) aa_count[threadIdx.x] = 0;
        if (clip_batch == 1 && b > 0) return;
        const int i = (bx - nb_tri) * 256 + threadIdx.x;
        if (i >= V) return;
        const float4 p = clip[(clip_batch == 1 ? 0ll : (long long)b * V) + i];
        aa_screen[(long long)b * V + i] = make_float2(p.x / p.w * (0.5f * W), p.y / p.w * (0.5f * H));
        return;
    }
    constexpr int TPW = 64 / LPT;  // triangles per wave
    // the four waves of a work-group take their TPW consecutive triangles from four places a quarter of the list apart (wave w: chunk
    // w nb_tri + blockIdx.x): a run of neighbouring triangles with huge boxes -- a spike of a mesh that training has driven apart --
    // then loads four times as many work-groups a quarter as much each; the pool below is per work-group whatever it holds, and a
    // wave's index reads stay one contiguous run
    const int f = (((int)threadIdx.x >> 6) * nb_tri + bx) * TPW + ((int)threadIdx.x & 63) / LPT;
    const int sub = threadIdx.x % LPT, lane = threadIdx.x & 63;
    const float4* pb = clip + (clip_batch == 1 ? 0ll : (long long)b * V);
    unsigned long long* kb = keys + (long long)b * H * W;
    const float4* pv = prev ? prev + (long long)b * H * W : nullptr;
    const float xs = 2.f / (float)W, xo = 1.f / (float)W - 1.f;
    const float ys = 2.f / (float)H, yo = 1.f / (float)H - 1.f;
    float4 p0 = make_float4(0, 0, 0, 0), p1 = p0, p2 = p0;
    int x0 = 0, y0 = 0, bw = 1, area = 0;
    if (f < F && sub == 0) {  // (the triangle's first lane alone: the other LPT - 1 only take their share of the pooled pixels below)
        const int i0 = tri[3 * f], i1 = tri[3 * f + 1], i2 = tri[3 * f + 2];
        if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
            p0 = pb[i0]; p1 = pb[i1]; p2 = pb[i2];
            area = rs_box(p0, p1, p2, H, W, x0, y0, bw);
        }
    }
    // The candidate pixels of the work-group's 256 / LPT triangles are POOLED and dealt out evenly over its 256 lanes (a culled box
    // carries area 0).  (Each triangle's lanes walking their own box made a wave as slow as its largest box: ~10 trips of the fragment
    // test where the pooled form needs ceil(sum / lanes); the fragment tests, not the atomics, were 11.6 of this kernel's 18.8 us.)
    // Pooled per work-group, boxes of any size: per wave, with boxes above 64 pixels walked by the whole wave one after the other
    // (with an integer division per pixel), a mesh that training had driven into spikes -- a few triangles of thousands of pixels,
    // every tenth above 64 -- took the launch from 36 to 190 us; a 9000-pixel box is 35 trips of the work-group now, not 140 of a wave.
    // Triangle data and the prefix of the box sizes go through LDS, one slice per wave.
    // LPT: the set-up (two dependent gathers + the box) is latency bound and wants many waves -- 4 lanes per triangle at B F = 1.9e5
    // (16.9 us against 22.1 with one) --, but is pure repetition once the waves suffice: one lane per triangle at B F = 7.7e5 (19.8 us
    // against 28.6 with four).
    // (round 4) A box above RS_BIG pixels does not enter the pool: its 8x8 TILES are tested first (below) and only the pixels of the
    // tiles the triangle can touch are -- a sliver's cost follows its area, not its box (a 9000-pixel box: ~20 of 140 tiles).
    __shared__ float4 s_p[4][TPW][3];
    __shared__ int4 s_box[4][TPW];  // x0, y0, bw | bh << 16, f
    __shared__ int s_pre[4][TPW + 1];
    __shared__ unsigned short s_big[256];
    __shared__ int s_nbig, s_ns;
    __shared__ int s_tiles[RS_TILE_CHUNK];
    __shared__ int s_bpre[257], s_wsum[4];
    const int wv = threadIdx.x >> 6, q = lane / LPT;  // this wave's slice, this lane's triangle slot
    bool big = area > RS_BIG;
    const int bh_all = area > 0 ? area / bw : 0;
    const int mine = (area > 0 && !big) ? area : 0;
    if (threadIdx.x == 0) { s_nbig = 0; s_ns = 0; }
    if (sub == 0) {
        s_p[wv][q][0] = p0; s_p[wv][q][1] = p1; s_p[wv][q][2] = p2;
        s_box[wv][q] = make_int4(x0, y0, bw | (bh_all << 16), f);  // (H, W < 2^15: checked by the entry point)
    }
    {   // inclusive scan of the TPW box sizes (held by the lanes LPT q)
        int incl = mine;
#pragma unroll
        for (int d = LPT; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (sub == 0) s_pre[wv][q + 1] = incl;
        if (lane == 0) s_pre[wv][0] = 0;
    }
    // (the barrier also says whether the work-group holds a big box at all: the usual one does not and ends after its pooled pixels,
    // without the second barrier the big boxes' list needs -- 0.8 us of every work-group's ~7 in a launch bound by seats x lifetime)
    const int any_big = __syncthreads_or(big);
    A3D_STAMP(0, 1);
    // candidate c of the work-group: first the wave slice (three compares on the four totals), then the slot inside it
    const int t0 = s_pre[0][TPW], t1 = t0 + s_pre[1][TPW], t2 = t1 + s_pre[2][TPW], total = t2 + s_pre[3][TPW];
    // (round 6, measured and dropped: boxes above 48 pixels pooled ROW by row -- the lane that draws a row solves its span of columns
    // (rs_row_span) and tests only those -- in every work-group: 45.9 -> 51.9 us on the trained-like mesh, 28.9 -> 31.1 fresh (a row is
    // ~6 pixel tests by ONE lane while the lanes with single pixels wait, and a usual work-group's pool is only 2-3 trips of its 256 lanes
    // anyway); only in work-groups whose pool exceeds 256 .. 16384 candidates: 54.7 .. 47.2 against 47.2 without.  The pooled phase is
    // not bound by its candidate count.  The row spans stay where every lane has one: the surviving tiles of the big boxes, below.)
    for (int c = threadIdx.x; c < total; c += 256) {
        const int w = c < t1 ? (c < t0 ? 0 : 1) : (c < t2 ? 2 : 3);
        const int cw = c - (w == 0 ? 0 : (w == 1 ? t0 : (w == 2 ? t1 : t2)));
        int j = 0;  // the triangle slot that owns the candidate: largest j with pre[j] <= cw
#pragma unroll
        for (int step = TPW / 2; step > 0; step >>= 1)
            if (s_pre[w][j + step] <= cw) j += step;
        int4 bx = s_box[w][j];
        bx.z &= 0xFFFF;
        const int i = cw - s_pre[w][j];
        // i / bw through the reciprocal: (i + 0.5) / bw is at least 0.5 / bw away from an integer and the product is off by ~2.4e-7 of
        // its value (< area / bw): exact for every box below ~1e6 pixels; larger ones (whole frames of >= 1024^2) divide
        int cy;
        if (i < (1 << 20)) cy = (int)(((float)i + 0.5f) * __builtin_amdgcn_rcpf((float)bx.z));
        else cy = i / bx.z;
        const int cx = i - cy * bx.z;
        rs_test_pixel(s_p[w][j][0], s_p[w][j][1], s_p[w][j][2], bx.x + cx, bx.y + cy, W, xs, xo, ys, yo, (unsigned)bx.w, kb, pv);
    }
    // ---- the big boxes of this work-group: their TILES are pooled like the pixels above (prefix of the tile counts, a search per
    // lane), tested, and the pixels of the surviving tiles pooled in turn -- per chunk of RS_TILE_CHUNK tiles, so that the survivor
    // list lives in 2 KB of LDS.  (One big box after the other, each with its own barriers, made a work-group whose 64 neighbouring
    // triangles are all big -- a spike of the drifted mesh -- slower than walking their boxes: 152 against 109 us.)
    A3D_STAMP(0, 2);
    if (!any_big) return;  // (uniform)
    if (sub == 0 && big) s_big[atomicAdd(&s_nbig, 1)] = (unsigned short)((wv << 8) | q);  // (LDS; s_nbig was zeroed before the barrier above)
    __syncthreads();
    const int nbig = s_nbig;
    A3D_STAMP(0, 3);
    if (nbig == 0) return;  // (uniform)
    {   // exclusive prefix of the tile counts over the list (nbig <= 256: one entry per thread)
        int cnt = 0;
        if ((int)threadIdx.x < nbig) {
            const int4 bx = s_box[s_big[threadIdx.x] >> 8][s_big[threadIdx.x] & 255];
            cnt = (((bx.z & 0xFFFF) + 7) >> 3) * (((bx.z >> 16) + 7) >> 3);
        }
        const int excl = a3d_block_excl_scan<4>(cnt, s_wsum);  // (every thread is here: the returns above are uniform)
        s_bpre[threadIdx.x] = excl;
        if (threadIdx.x == 255) s_bpre[256] = excl + cnt;
    }
    __syncthreads();
    const int total_tiles = s_bpre[256];
    const float hx = 0.5f * xs * 8.f, hy = 0.5f * ys * 8.f;  // half a tile in NDC (a tile cut by the box is tested whole: conservative)
    for (int tb = 0; tb < total_tiles; tb += RS_TILE_CHUNK) {  // (uniform)
#pragma unroll
        for (int r = 0; r < RS_TILE_CHUNK / 256; ++r) {
            const int g = tb + r * 256 + (int)threadIdx.x;
            bool keep = false;
            int packed = 0;
            if (g < total_tiles) {
                int j = 0;  // the big box that owns tile g: largest j with bpre[j] <= g
#pragma unroll
                for (int step = 128; step > 0; step >>= 1)
                    if (j + step < nbig && s_bpre[j + step] <= g) j += step;
                const int w = s_big[j] >> 8, qs = s_big[j] & 255, t = g - s_bpre[j];
                const int4 bx = s_box[w][qs];
                const int ntx = ((bx.z & 0xFFFF) + 7) >> 3, ty = t / ntx, tx = t - ty * ntx;
                // The three edge functions of rs_frag are LINEAR in the pixel centre (fx, fy): a_k = C_k + A_k fx + B_k fy (the fx fy
                // terms cancel); a pixel is inside iff all three are >= 0 or all three <= 0.  Over a tile a_k ranges over its value at
                // the centre +- (|A_k| hx + |B_k| hy); a tile where some a_k stays < 0 AND some a_k' stays > 0 holds no covered pixel.
                // tol: the rounding of rs_frag's own products (it evaluates the same polynomial through q = p - f w), a few ulps of
                // the largest term, taken ~40x wider.
                const float fx = __builtin_fmaf(xs, (float)(bx.x + 8 * tx) + 3.5f, xo), fy = __builtin_fmaf(ys, (float)(bx.y + 8 * ty) + 3.5f, yo);
                bool pos = true, neg = true;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float4 u = s_p[w][qs][(k + 1) % 3], v = s_p[w][qs][(k + 2) % 3];
                    const float C = u.x * v.y - u.y * v.x, A = -(u.w * v.y - u.y * v.w), Bc = -(u.x * v.w - u.w * v.x);
                    // (+ the q1x q2y products' own w w f f terms, which cancel in exact arithmetic but not in their rounding: they
                    // dominate when two vertices project next to the NDC origin and the tile lies far from it)
                    const float tol = 5e-6f * ((fabsf(u.x * v.y) + fabsf(u.y * v.x)) + 2.f * (fabsf(u.w * v.y) + fabsf(u.y * v.w)) + 2.f * (fabsf(u.x * v.w) + fabsf(u.w * v.x))
                                               + 2.f * fabsf(u.w * v.w) * (fabsf(fx) + hx) * (fabsf(fy) + hy)) + RS_TOL_ABS;
                    const float vk = C + A * fx + Bc * fy, ext = fabsf(A) * hx + fabsf(Bc) * hy + tol;
                    pos = pos && (vk + ext >= 0.f);
                    neg = neg && (vk - ext <= 0.f);
                }
                keep = pos || neg;
                packed = (j << 24) | t;  // (t < 2^24: a 32767 x 32767 frame has 1.7e7 tiles)
            }
            const unsigned long long m = __ballot(keep);
            int base = 0;
            if (lane == 0 && m) base = atomicAdd(&s_ns, __popcll(m));
            base = __shfl(base, 0, 64);
            if (keep) s_tiles[base + a3d_wave_prefix(m)] = packed;
        }
        __syncthreads();
        const int ns = s_ns;
        // (round 6) a surviving tile is worked off ROW by row: the lane that draws (tile, row) solves the row's span inside the tile
        // (rs_row_span) and tests those pixels -- a sliver crossing a tile covers ~10 of its 64 pixels
        for (int i = threadIdx.x; i < ns * 8; i += 256) {
            const int e = s_tiles[i >> 3], j = (e >> 24) & 255, t = e & 0xFFFFFF;
            const int w = s_big[j] >> 8, qs = s_big[j] & 255;
            const int4 bx = s_box[w][qs];
            const int bwid = bx.z & 0xFFFF, bh = (bx.z >> 16) & 0x7FFF, ntx = (bwid + 7) >> 3, ty = t / ntx, tx = t - ty * ntx;
            const int cy = 8 * ty + (i & 7);
            if (cy >= bh) continue;
            const float4 q0 = s_p[w][qs][0], q1 = s_p[w][qs][1], q2 = s_p[w][qs][2];
            const int xl = bx.x + 8 * tx, xh = min(xl + 7, bx.x + bwid - 1), py = bx.y + cy;
            const float fxm = fmaxf(fabsf(__builtin_fmaf(xs, (float)xl, xo)), fabsf(__builtin_fmaf(xs, (float)xh, xo)));
            int xa, xb;
            rs_row_span(q0, q1, q2, __builtin_fmaf(ys, (float)py, yo), xs, xo, fxm, xl, xh, xa, xb);
            for (int px = xa; px <= xb; ++px) rs_test_pixel(q0, q1, q2, px, py, W, xs, xo, ys, yo, (unsigned)bx.w, kb, pv);
        }
        __syncthreads();
        if (threadIdx.x == 0) s_ns = 0;
        __syncthreads();
    }
    A3D_STAMP(0, 5);
}

// grid (ceil(H*W / 256), B): the image comes from blockIdx.y and the row/column from one 32-bit division.
// TILE: the work-group walks its 256 pixels as four 8x8 tiles in the covered-pixel list's order (cover.hip) and leaves that list's
// per-256-entry block count behind, so a3d_cover_count can skip its own pass over the frame.
template <bool TILE>
__global__ __launch_bounds__(256) void rs_resolve_kernel(const float4* __restrict__ clip, int clip_batch, const int* __restrict__ tri, int V,
                                                         int H, int W, unsigned long long* __restrict__ keys,
                                                         float4* __restrict__ rast, int* __restrict__ cover_block_count) {
    __shared__ int s_wave[4];
    A3D_STAMP(1, 0);
    const unsigned hw = (unsigned)H * (unsigned)W;
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_frame = k < hw;
    unsigned rem = k;
    int px, py;
    if (TILE) {  // (H, W multiples of 8 and H*W a multiple of 256: checked by the entry point)
        const unsigned in_tile = k & 63u, t = k >> 6, tw = (unsigned)W >> 3;
        const unsigned ty = t / tw, tx = t - ty * tw;
        py = (int)(ty * 8u + (in_tile >> 3));
        px = (int)(tx * 8u + (in_tile & 7u));
        rem = (unsigned)py * (unsigned)W + (unsigned)px;
    } else {
        if (!in_frame) return;
        py = (int)(rem / (unsigned)W);
        px = (int)(rem - (unsigned)py * (unsigned)W);
    }
    const int b = blockIdx.y;
    const long long i = (long long)b * hw + rem;
    const unsigned long long key = keys[i];
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (key != RS_EMPTY) {
        keys[i] = RS_EMPTY;  // leave the key buffer armed for the next call (saves its 8 B/pixel clear launch: scratch_is_clean)
        const float4* pb = clip + (clip_batch == 1 ? 0ll : (long long)b * V);
        const int f = (int)(unsigned)(key & 0xFFFFFFFFull);
        const float4 p0 = pb[tri[3 * f]], p1 = pb[tri[3 * f + 1]], p2 = pb[tri[3 * f + 2]];
        const float xs = 2.f / (float)W, xo = 1.f / (float)W - 1.f;
        const float ys = 2.f / (float)H, yo = 1.f / (float)H - 1.f;
        const RsFrag fr = rs_frag(p0, p1, p2, __builtin_fmaf(xs, (float)px, xo), __builtin_fmaf(ys, (float)py, yo));
        o = make_float4(fr.u, fr.v, fr.zw, (float)(f + 1));
    }
    rast[i] = o;
    if (TILE) {
        const unsigned long long m = __ballot(key != RS_EMPTY);
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) {
            const int blk = b * (int)gridDim.x + (int)blockIdx.x, c = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
            cover_block_count[blk] = c;
            // the sum of this block's group of 64 (cover.hip): <= 64 fire-and-forget adds per address
            if (c) atomicAdd(cover_block_count + (long long)gridDim.x * gridDim.y + (long long)(blk / A3D_COVER_GROUP) * A3D_COVER_GROUP_STRIDE, c);
        }
    }
    A3D_STAMP(1, 5);
}

// ---- resolve + covered-pixel list + G-buffer rows in ONE launch (round 5): the atomic path's second launch and a3d_cover_gbuffer_fwd
// are both one work-group per 256-pixel block in the list's tile order, the second one reading back the texels the first has just
// written; what kept them apart is that a block's place in the list is the number of covered pixels in all blocks before it.  Here
// every work-group counts its own (the keys say: covered <=> key != EMPTY), PUBLISHES the count, and its first wave looks the earlier
// ones up -- two levels, like the sums the resolve used to leave: the counts of the earlier blocks of its group of 64 and the totals of
// the earlier groups (published by each group's last block), <= 63 + nb / 64 flags, all requested at once, each awaited with an
// agent-scope load in a sleep loop.  Work-groups are dispatched in the order of their linear index (x fastest), the list's order, and
// a flag is published before its work-group waits for anything: the lowest-numbered unfinished work-group never waits on an
// undispatched one, so the loop ends.  (A spin budget backs that up: when it runs out the work-group raises a status word and goes on
// with what it has -- the caller re-runs through the two-launch path; nothing hangs.)  The gathers of the resolve and the look-up
// are issued together, so the look-up hides behind them.
// ``p_cap``: rows the caller allocated for the list (it does not know P yet: the previous frame's + a margin); entries past it are
// dropped and the caller, who reads P from the group sums as before, re-runs a3d_cover_gbuffer_fwd when P > p_cap (the texels, the
// block counts and the sums are complete either way).
__device__ __forceinline__ int rs_await(const int* p, int* timeout) {
    // (a RETURNING atomic, not a load: the flags live in ordinary device memory, which an XCD's L2 caches without cross-XCD coherence inside
    // a kernel -- an sc1 load that has once fetched the line keeps answering from it, and the first version of this loop spun for
    // seconds on flags that had long been published; atomics are performed at the memory side, where the publishers' adds land)
    int v = __hip_atomic_fetch_add(const_cast<int*>(p), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int spin = 0; v == 0 && spin < (1 << 15); ++spin) {  // (~50 ms: a correct run waits microseconds)
        __builtin_amdgcn_s_sleep(8);
        v = __hip_atomic_fetch_add(const_cast<int*>(p), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (v == 0) { *timeout = 1; return 0; }
    return v - 1;
}

__global__ __launch_bounds__(256) void rs_resolve_cover_kernel(const float4* __restrict__ clip, int clip_batch, const int* __restrict__ tri, int V,
                                                               int F, int H, int W, unsigned long long* __restrict__ keys,
                                                               float4* __restrict__ rast, int* __restrict__ block_count,
                                                               int* __restrict__ group_sum, int* blk_flag, int* grp_flag, int nb_total,
                                                               long long* __restrict__ pix, int* __restrict__ inv, long long p_cap,
                                                               const float* __restrict__ v_pos, const float* __restrict__ v_nrm,
                                                               const float* __restrict__ prior, int prior_batch, float* __restrict__ out,
                                                               const float* __restrict__ extra, int E, float* __restrict__ extra_out,
                                                               float4* __restrict__ zero_rows, long long n_zero4,
                                                               const GbAux aux) {
    float* __restrict__ tex_out = aux.tex_out;
    long long* __restrict__ img_out = aux.img_out;
    __shared__ int wave_n[4];
    __shared__ int s_off;
    __shared__ int s_total;
    A3D_STAMP(3, 0);  // (kernel id 3 = rs_resolve_cover_kernel)
    const int b = blockIdx.y, L = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned hw = (unsigned)H * (unsigned)W;
    const unsigned k = blockIdx.x * 256u + threadIdx.x;
    const unsigned in_tile = k & 63u, t = k >> 6, tw = (unsigned)W >> 3;
    const unsigned ty = t / tw, tx = t - ty * tw;
    const int py = (int)(ty * 8u + (in_tile >> 3)), px = (int)(tx * 8u + (in_tile & 7u));
    const long long flat = (long long)b * hw + (unsigned)py * (unsigned)W + (unsigned)px;
    for (long long z = (long long)L * 256 + threadIdx.x; z < n_zero4; z += (long long)nb_total * 256) zero_rows[z] = make_float4(0.f, 0.f, 0.f, 0.f);
    const unsigned long long key = keys[flat];
    const bool on = key != RS_EMPTY;
    const unsigned long long m = __ballot(on);
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    const int cnt = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    if (threadIdx.x == 0) {  // published before this work-group waits for anything
        block_count[L] = cnt;
        // (an atomic ADD onto the zeroed flag, not a store: device atomics are performed at the memory side, where every XCD's waiters look;
        // a plain agent-scope store may sit in this XCD's L2 until the kernel ends)
        __hip_atomic_fetch_add(blk_flag + L, cnt + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the winner's texel: gathers requested now, the look-up below runs while they are in flight
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) {
        keys[flat] = RS_EMPTY;  // re-armed for the next call (scratch_is_clean)
        const float4* pb = clip + (clip_batch == 1 ? 0ll : (long long)b * V);
        const int f = (int)(unsigned)(key & 0xFFFFFFFFull);
        const float4 p0 = pb[tri[3 * f]], p1 = pb[tri[3 * f + 1]], p2 = pb[tri[3 * f + 2]];
        const float xs = 2.f / (float)W, xo = 1.f / (float)W - 1.f;
        const float ys = 2.f / (float)H, yo = 1.f / (float)H - 1.f;
        const RsFrag fr = rs_frag(p0, p1, p2, __builtin_fmaf(xs, (float)px, xo), __builtin_fmaf(ys, (float)py, yo));
        o = make_float4(fr.u, fr.v, fr.zw, (float)(f + 1));
    }
    rast[flat] = o;
    const int g = L / A3D_COVER_GROUP, r = L - g * A3D_COVER_GROUP;
    const bool last_of_group = r == A3D_COVER_GROUP - 1 || L == nb_total - 1;
    // the launch's LAST work-group also learns the length of the whole list (it looks every earlier group up anyway when it holds a
    // covered pixel; with padding rows to fill it does so regardless) and fills the fields' padding rows behind it
    const bool pads = L == nb_total - 1 && aux.pad_to > 0 && (aux.tex_out || aux.img_out);
    if (wave == 0 && (cnt > 0 || last_of_group)) {
        int timeout = 0;
        int own = lane < r ? rs_await(blk_flag + g * A3D_COVER_GROUP + lane, &timeout) : 0;  // earlier blocks of my group
        own = a3d_group_sum(own);
        // (a group's total depends on its own blocks' counts ONLY and is published before this wave waits for the totals of earlier groups: no
        // chain from group to group)
        if (last_of_group && lane == 0) {
            group_sum[(long long)g * A3D_COVER_GROUP_STRIDE] = own + cnt;  // (plain: what the host adds up, as before)
            __hip_atomic_fetch_add(grp_flag + g, own + cnt + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (cnt > 0 || pads) {
            int before = 0;
            for (int j = lane; j < g; j += 64) before += rs_await(grp_flag + j, &timeout);  // earlier groups
            before = a3d_group_sum(before);
            if (lane == 0) { s_off = before + own; s_total = before + own + cnt; }
        }
        if (__ballot(timeout != 0) && lane == 0) atomicOr(group_sum + 3, 1);  // status word (never in the sums: word 3 of the first line)
    }
    A3D_STAMP(3, 1);
    if (pads) {  // (uniform)
        __syncthreads();
        const long long total = s_total;
        gb_fill_padding(aux, total < p_cap ? total : p_cap, (int)gridDim.y - 1);
    }
    if (cnt == 0) {  // (uniform) background only: the map entries and out
        if (inv) inv[flat] = -1;
        A3D_STAMP(3, 5);
        return;
    }
    __syncthreads();
    if (!on) {
        if (inv) inv[flat] = -1;
        A3D_STAMP(3, 5);
        return;
    }
    int oidx = s_off + a3d_wave_prefix(m);
    for (int w = 0; w < wave; ++w) oidx += wave_n[w];
    if (inv) inv[flat] = oidx;
    if (oidx < p_cap) {
        pix[oidx] = flat;
        gb_row(o, flat, oidx, tri, v_pos, v_nrm, prior, prior_batch, V, F, (long long)hw, out, extra, E, extra_out, tex_out, img_out);
    }
    A3D_STAMP(3, 5);
}

// backward of (u,v) w.r.t. clip-space x, y, w of the three vertices.  Round 6: one thread per pixel of a 16 x 16 tile; the three
// (x, y, -, w) gradient rows of a pixel meet their neighbours' in the work-group's LDS table (tile_scatter.h) and leave as one row of
// adjacent atomics per vertex and tile.  (Until round 5: four lanes per pixel, one line-coalesced atomic request per (pixel, vertex),
// bound by the 6e5 requests to the memory-side atomic units.  Kernel us at B = 16, 256 x 256, rocprofv3: 42.6 -> 18.6 on the fresh
// mesh, 74.4 -> 20.3 on the trained-like one; where the 18.6 go: tile_scatter.h and tools/shim_bwd_phases.py.)
__global__ __launch_bounds__(256) void rs_bwd_kernel(const float4* __restrict__ g_rast, const float4* __restrict__ rast,
                                                     const float4* __restrict__ clip, int clip_batch, const int* __restrict__ tri,
                                                     int V, int F, int H, int W, int tiles_x, float* __restrict__ g_clip) {
    extern __shared__ __align__(16) unsigned char rs_bwd_lds[];
    A3D_STAMP(4, 0);
    const int b = blockIdx.y, tile = blockIdx.x;
    int px, py;
    ts_pixel((tile % tiles_x) * TS_TILE, (tile / tiles_x) * TS_TILE, px, py);
    const bool inside = px < W && py < H;
    const long long i = ((long long)b * H + py) * W + px;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f), g = r;
    if (inside) r = rast[i];
    const int f = (int)r.w - 1;
    bool live = inside && f >= 0 && f < F;
    if (live) {
        g = g_rast[i];
        live = g.x != 0.f || g.y != 0.f;
    }
    if (!__syncthreads_or(live)) return;
    TileScatter ts;
    ts.init(rs_bwd_lds, 4);
    const int vb = clip_batch == 1 ? 0 : b * V;
    int i0 = 0, i1 = 0, i2 = 0, key = -1;
    float c[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // (x, y, w) of the three corners
    if (live) {
        i0 = tri[3 * f]; i1 = tri[3 * f + 1]; i2 = tri[3 * f + 2];
        const float4 p0 = clip[vb + i0], p1 = clip[vb + i1], p2 = clip[vb + i2];
        const float fx = ((float)px + 0.5f) * (2.f / (float)W) - 1.f;
        const float fy = ((float)py + 0.5f) * (2.f / (float)H) - 1.f;
        const float q0x = p0.x - fx * p0.w, q0y = p0.y - fy * p0.w;
        const float q1x = p1.x - fx * p1.w, q1y = p1.y - fy * p1.w;
        const float q2x = p2.x - fx * p2.w, q2y = p2.y - fy * p2.w;
        const float a0 = q1x * q2y - q1y * q2x, a1 = q2x * q0y - q2y * q0x, a2 = q0x * q1y - q0y * q1x;
        const float s = a0 + a1 + a2;
        if (s != 0.f) {
            const float is = 1.f / s;
            const float u = a0 * is, v = a1 * is;
            const float t = g.x * u + g.y * v;
            const float ga0 = (g.x - t) * is, ga1 = (g.y - t) * is, ga2 = -t * is;
            c[0] = -ga1 * q2y + ga2 * q1y; c[1] = ga1 * q2x - ga2 * q1x;
            c[3] = ga0 * q2y - ga2 * q0y;  c[4] = -ga0 * q2x + ga2 * q0x;
            c[6] = -ga0 * q1y + ga1 * q0y; c[7] = ga0 * q1x - ga1 * q0x;
#pragma unroll
            for (int k = 0; k < 3; ++k) c[3 * k + 2] = -fx * c[3 * k] - fy * c[3 * k + 1];
            key = f;
        }
    }
    A3D_STAMP(4, 1);
    ts_merge<9, 6>(key, c);
    A3D_STAMP(4, 2);
    __syncthreads();  // (table initialised)
    const int e0 = ts.entries(key >= 0, 3);
    if (key >= 0) {
        const int row[3] = {vb + i0, vb + i1, vb + i2};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int sl = ts.slot(row[k]);
            if (sl >= 0) {
                *reinterpret_cast<float4*>(ts.e_val + 4 * (e0 + k)) = make_float4(c[3 * k], c[3 * k + 1], 0.f, c[3 * k + 2]);
                ts.link(e0 + k, sl);
            } else {
                float* o = g_clip + (long long)row[k] * 4;
                atomicAdd(o, c[3 * k]); atomicAdd(o + 1, c[3 * k + 1]); atomicAdd(o + 3, c[3 * k + 2]);
            }
        }
    }
    A3D_STAMP(4, 3);
    __syncthreads();
    A3D_STAMP(4, 4);
    ts.flush<4>(g_clip, 4, 2);
    A3D_STAMP(4, 5);
}

extern "C" size_t a3d_rast_scratch_bytes(int B, int H, int W) { return sizeof(unsigned long long) * (size_t)B * (size_t)H * (size_t)W; }

extern "C" int a3d_rast_fwd(const float* clip, int clip_batch, const int32_t* tri, int B, int V, int F, int H, int W, float* rast, void* scratch,
                            int scratch_is_clean, const a3d_rast_opts* opts_or_null, a3d_stream_t stream) {
    a3d_rast_opts o = {};
    if (opts_or_null) {
        A3D_CHECK_ARG(opts_or_null->size >= sizeof(a3d_rast_opts));
        o = *opts_or_null;
    }
    const float* prev_rast_or_null = o.prev_rast;
    void* cover_scratch_or_null = o.cover_scratch;
    float* aa_screen_or_null = o.aa_screen;
    int32_t* aa_count_or_null = o.aa_count;
    const int32_t *topo_off_or_null = o.topo_off, *topo_adj_or_null = o.topo_adj;
    int32_t* topo_opp_or_null = o.topo_opp;
    const float *normals_v_a_or_null = o.normals_v_a, *normals_v_b_or_null = o.normals_v_b;
    const int normals_B_a = o.normals_B_a, normals_B_b = o.normals_B_b, lists_stride = o.lists_stride;
    const int32_t *normals_off = o.normals_off, *normals_adj = o.normals_adj;
    float *normals_acc_a = o.normals_acc_a, *normals_a = o.normals_a, *normals_acc_b = o.normals_acc_b, *normals_b = o.normals_b;
    A3D_CHECK_ARG(clip && rast && B > 0 && V > 0 && F >= 0 && H > 0 && W > 0);
    A3D_CHECK_ARG(F == 0 || (tri && scratch));
    A3D_CHECK_ARG(clip_batch == 1 || clip_batch == B);
    A3D_CHECK_ARG((long long)H * W < 0x7fffffffll && B <= 65535 && H < 32768 && W < 32768);
    hipStream_t s = (hipStream_t)stream;
    const long long npix = (long long)B * H * W;
    // the covered-pixel block counts ride along when the list's tile order applies and its blocks do not cross images
    A3D_CHECK_ARG(!cover_scratch_or_null || (H % 8 == 0 && W % 8 == 0 && ((long long)H * W) % 256 == 0));
    const int cover_nb = (int)(npix / 256);
    // (words zeroed behind the block counts by the triangle launch: the group-sum area, and -- defer_resolve -- the look-back flags after it)
    const bool defer = o.defer_resolve != 0 && cover_scratch_or_null && !prev_rast_or_null && F > 0;
    A3D_CHECK_ARG(!o.defer_resolve || defer);
    const int cover_ng = a3d_div_up(cover_nb, A3D_COVER_GROUP) * A3D_COVER_GROUP_STRIDE + (defer ? cover_nb + a3d_div_up(cover_nb, A3D_COVER_GROUP) : 0);
    A3D_CHECK_ARG(F > 0 || !normals_v_a_or_null);  // (no triangle launch to ride in)
    if (F == 0) {
        A3D_HIP(hipMemsetAsync(rast, 0, sizeof(float) * 4 * (size_t)npix, s));
        if (cover_scratch_or_null) A3D_HIP(hipMemsetAsync(cover_scratch_or_null, 0, sizeof(int) * ((size_t)cover_nb + cover_ng), s));
        return A3D_OK;
    }
    unsigned long long* keys = (unsigned long long*)scratch;
    if (!scratch_is_clean) A3D_HIP(hipMemsetAsync(keys, 0xFF, sizeof(unsigned long long) * (size_t)npix, s));
    A3D_CHECK_ARG((aa_screen_or_null == nullptr) == (aa_count_or_null == nullptr) && a3d_aa_shards() <= 256);
    A3D_CHECK_ARG((topo_opp_or_null == nullptr) == (topo_off_or_null == nullptr) && (topo_opp_or_null == nullptr) == (topo_adj_or_null == nullptr));
    // lanes per triangle (rs_tri_kernel), by the number of (image, triangle) pairs -- measured 1.9e5 pairs: 16.9 / 17.7 / 22.0 us with
    // 4 / 2 / 1 lanes, 7.7e5 pairs: 28.4 / 21.6 / 19.9
    const long long pairs = (long long)B * F;
    const int lpt = pairs <= 300000 ? 4 : (pairs <= 600000 ? 2 : 1);
    const int nb_tri = a3d_div_up(F, 256 / lpt), nb_screen = aa_screen_or_null ? a3d_div_up(V, 256) : 0;
    const int nb_opp = topo_opp_or_null ? a3d_div_up(a3d_div_up(3ll * F, 256), B) : 0;  // (per row of the grid)
    RsNormalsJob nj = {};
    A3D_CHECK_ARG(lists_stride >= 0);
    nj.stride = lists_stride;
    if (normals_v_a_or_null) {
        A3D_CHECK_ARG(normals_B_a > 0 && normals_B_b >= 0 && normals_off && normals_adj && normals_acc_a && normals_a);
        A3D_CHECK_ARG(normals_B_b == 0 || (normals_v_b_or_null && normals_acc_b && normals_b));
        nj.v_a = normals_v_a_or_null; nj.v_b = normals_v_b_or_null; nj.off = normals_off; nj.adj = normals_adj;
        nj.acc_a = normals_acc_a; nj.nrm_a = normals_a; nj.acc_b = normals_acc_b; nj.nrm_b = normals_b;
        nj.B_a = normals_B_a; nj.B_b = normals_B_b;
        nj.wg_per_row = a3d_div_up((long long)a3d_div_up(V, 256) * (normals_B_a + normals_B_b), B);
    }
#define RS_LAUNCH_TRI(LPT_) \
    hipLaunchKernelGGL(rs_tri_kernel<LPT_>, dim3(nb_tri + nb_screen + nb_opp + nj.wg_per_row, B), dim3(256), 0, s, \
                       (const float4*)clip, clip_batch, \
                       tri, V, F, H, W, keys, (const float4*)prev_rast_or_null, nb_tri, (float2*)aa_screen_or_null, aa_count_or_null, \
                       a3d_aa_shards(), cover_scratch_or_null ? (int*)cover_scratch_or_null + cover_nb : nullptr, cover_ng, nb_screen, \
                       topo_off_or_null, topo_adj_or_null, topo_opp_or_null, nb_opp, nj); \

    if (lpt == 4) { RS_LAUNCH_TRI(4) } else if (lpt == 2) { RS_LAUNCH_TRI(2) } else { RS_LAUNCH_TRI(1) }
#undef RS_LAUNCH_TRI
    A3D_LAUNCH_CHECK();
    if (defer) return A3D_OK;  // (the caller resolves: a3d_rast_resolve_gbuffer_fwd, or a3d_rast_resolve)
    if (cover_scratch_or_null)
        hipLaunchKernelGGL(rs_resolve_kernel<true>, dim3(a3d_div_up((long long)H * W, 256), B), dim3(256), 0, s, (const float4*)clip, clip_batch, tri,
                           V, H, W, keys, (float4*)rast, (int*)cover_scratch_or_null);
    else
        hipLaunchKernelGGL(rs_resolve_kernel<false>, dim3(a3d_div_up((long long)H * W, 256), B), dim3(256), 0, s, (const float4*)clip, clip_batch, tri,
                           V, H, W, keys, (float4*)rast, (int*)nullptr);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

// the second half of a3d_rast_fwd(defer_resolve = 1), stand-alone: the resolve launch (texels, block counts, group sums)
extern "C" int a3d_rast_resolve(const float* clip, int clip_batch, const int32_t* tri, int B, int V, int F, int H, int W, float* rast, void* scratch,
                                void* cover_scratch, a3d_stream_t stream) {
    A3D_CHECK_ARG(clip && tri && rast && scratch && cover_scratch && B > 0 && V > 0 && F > 0 && H > 0 && W > 0 && B <= 65535);
    A3D_CHECK_ARG((clip_batch == 1 || clip_batch == B) && H % 8 == 0 && W % 8 == 0 && ((long long)H * W) % 256 == 0 && (long long)B * H * W < 0x7fffffffll);
    hipLaunchKernelGGL(rs_resolve_kernel<true>, dim3(a3d_div_up((long long)H * W, 256), B), dim3(256), 0, (hipStream_t)stream, (const float4*)clip, clip_batch,
                       tri, V, H, W, (unsigned long long*)scratch, (float4*)rast, (int*)cover_scratch);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

// ... or fused with the covered-pixel list and its G-buffer rows (rs_resolve_cover_kernel)
extern "C" int a3d_rast_resolve_gbuffer_fwd(const float* clip, int clip_batch, const int32_t* tri, int B, int V, int F, int H, int W, float* rast,
                                            void* scratch, void* cover_scratch, int64_t p_cap, int64_t* pix, int32_t* inv_or_null,
                                            const float* v_pos, const float* v_nrm, const float* prior, int prior_batch, float* out,
                                            const float* extra_or_null, int E, float* extra_out_or_null, float* g_rows_to_clear_or_null,
                                            const a3d_gb_aux* aux_or_null, a3d_stream_t stream) {
    A3D_CHECK_ARG(!aux_or_null || (aux_or_null->size >= sizeof(a3d_gb_aux) && aux_or_null->rows >= p_cap && aux_or_null->pad_to >= 0));
    A3D_CHECK_ARG(clip && tri && rast && scratch && cover_scratch && B > 0 && V > 0 && F > 0 && H > 0 && W > 0 && B <= 65535 && p_cap >= 0);
    A3D_CHECK_ARG((clip_batch == 1 || clip_batch == B) && H % 8 == 0 && W % 8 == 0 && ((long long)H * W) % 256 == 0 && (long long)B * H * W < 0x7fffffffll);
    A3D_CHECK_ARG(prior_batch == 1 || prior_batch == B);
    A3D_CHECK_ARG(p_cap == 0 || (pix && v_pos && v_nrm && prior && out));
    A3D_CHECK_ARG(!extra_or_null || (E >= 1 && E <= 3 && (extra_out_or_null || p_cap == 0)));
    A3D_CHECK_ARG(!g_rows_to_clear_or_null || ((uintptr_t)g_rows_to_clear_or_null & 63) == 0);
    const int nb = (int)((long long)B * H * W / 256), ng = a3d_div_up(nb, A3D_COVER_GROUP);
    int* cs = (int*)cover_scratch;
    int* group_sum = cs + nb;
    int* blk_flag = group_sum + (size_t)ng * A3D_COVER_GROUP_STRIDE;
    const long long n_zero4 = g_rows_to_clear_or_null ? (long long)B * V * 4 : 0;  // (A3D_GBUFFER_GRAD_COLS / 4 float4 per (image, vertex))
    hipLaunchKernelGGL(rs_resolve_cover_kernel, dim3(a3d_div_up((long long)H * W, 256), B), dim3(256), 0, (hipStream_t)stream, (const float4*)clip, clip_batch,
                       tri, V, F, H, W, (unsigned long long*)scratch, (float4*)rast, cs, group_sum, blk_flag, blk_flag + nb, nb, (long long*)pix,
                       inv_or_null, (long long)p_cap, v_pos, v_nrm, prior, prior_batch, out, extra_or_null, E, extra_out_or_null,
                       (float4*)g_rows_to_clear_or_null, n_zero4, gb_aux_of(aux_or_null));
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

// ---- the property the look-back of rs_resolve_cover_kernel rests on, probed on THIS box / driver / partition mode before it is relied on
// (VERDICT r5 weak 3): work-groups are dispatched in the order of their linear index, so that a work-group that waits for the flag of a
// lower-numbered one never waits for a work-group that has no seat yet.  The probe is that very situation, made as hard as the launch
// allows: n work-groups (many times what the device seats at once), every one WAITS -- holding its seat -- for the flag of the
// work-group ``stride`` before it, with the resolve's own spin budget, then raises its own.  Were the order violated anywhere, a
// waiter would sit on a seat its predecessor needs and run out of budget: status != 0.  ~0.1 ms, once per process.
__global__ __launch_bounds__(64) void rs_dispatch_probe_kernel(int* flags, int n, int stride, int* status) {
    const int L = (int)blockIdx.x;
    if (threadIdx.x == 0) {
        if (L >= stride) {
            int timeout = 0;
            rs_await(flags + (L - stride), &timeout);
            if (timeout) atomicOr(status, 1);
        }
        __hip_atomic_fetch_add(flags + L, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (L == n - 1) atomicOr(status, 2);  // (the last work-group ran: the launch was not cut short)
    }
}

extern "C" int a3d_dispatch_order_probe(int n_workgroups, int stride, int32_t* scratch, a3d_stream_t stream) {
    A3D_CHECK_ARG(n_workgroups > 0 && stride > 0 && scratch);
    hipStream_t s = (hipStream_t)stream;
    A3D_HIP(hipMemsetAsync(scratch, 0, sizeof(int) * ((size_t)n_workgroups + 1), s));  // flags[n] | status
    hipLaunchKernelGGL(rs_dispatch_probe_kernel, dim3(n_workgroups), dim3(64), 0, s, scratch, n_workgroups, stride, scratch + n_workgroups);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_rast_bwd(const float* g_rast, const float* rast, const float* clip, int clip_batch, const int32_t* tri, int B, int V,
                            int F, int H, int W, float* g_clip, a3d_stream_t stream) {
    A3D_CHECK_ARG(g_rast && rast && clip && g_clip && B > 0 && V > 0 && F >= 0 && H > 0 && W > 0);
    A3D_CHECK_ARG(clip_batch == 1 || clip_batch == B);
    hipStream_t s = (hipStream_t)stream;
    A3D_HIP(hipMemsetAsync(g_clip, 0, sizeof(float) * 4 * (size_t)clip_batch * V, s));
    if (F == 0) return A3D_OK;
    const long long npix = (long long)B * H * W;
    A3D_CHECK_ARG(npix < 0x7fffffffll && B <= 65535 && (long long)clip_batch * V < 0x7fffffffll);
    const int tiles_x = a3d_div_up(W, TS_TILE), tiles_y = a3d_div_up(H, TS_TILE);
    hipLaunchKernelGGL(rs_bwd_kernel, dim3(tiles_x * tiles_y, B), dim3(256), TileScatter::lds_bytes(4), s, (const float4*)g_rast, (const float4*)rast,
                       (const float4*)clip, clip_batch, tri, V, F, H, W, tiles_x, g_clip);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

A3D_PROFILE_TU(raster)
