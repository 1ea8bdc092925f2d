// Shared helpers for the liba3d_hip kernels (gfx950 / CDNA4, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/a3d.h"

#define A3D_WAVE 64
// covered-pixel list (cover.hip; the rasteriser's resolve writes the same scratch): per-256-pixel block counts [nb] followed by the sums
// of groups of 64 consecutive blocks, one sum per 64-byte line [ceil(nb / 64) * 16 ints] (the sums are accumulated with device atomics:
// neighbours in one line serialise against each other in the L2's atomic unit)
#define A3D_COVER_GROUP 64
#define A3D_COVER_GROUP_STRIDE 16

void a3d_set_error(const char* fmt, ...);

#define A3D_CHECK_ARG(cond)                                                   \
    do {                                                                      \
        if (!(cond)) {                                                        \
            a3d_set_error("%s: invalid argument: %s", __func__, #cond);       \
            return A3D_EINVAL;                                                \
        }                                                                     \
    } while (0)

#define A3D_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            a3d_set_error("%s: %s failed: %s", __func__, #call, hipGetErrorString(e_));       \
            return A3D_EHIP;                                                                  \
        }                                                                                     \
    } while (0)

#define A3D_LAUNCH_CHECK() A3D_HIP(hipGetLastError())

static inline int a3d_div_up(long long a, long long b) { return (int)((a + b - 1) / b); }

#ifdef __HIPCC__
// ---- phase stamps inside kernels (tools/kernel_phases.py; the library proper is built WITHOUT them: build.py --profile makes a second,
// instrumented liba3d_hip_prof.so).  A3D_STAMP(kernel id within the TU, slot 0..7): thread 0 of every work-group writes the 100 MHz wall
// clock to buf[work-group][slot] when the TU's active kernel id is that one; A3D_STAMP_CLOCK the shader clock (for the frequency the
// launch ran at).  A3D_PROFILE_TU(name) defines the TU's setter a3d_profile_set_<name>(buf, kid).  What this is for: every hot-path
// kernel here is bound by dependent round trips, barriers or the instructions of its longest-lived work-group, not by bytes, and the
// counters say so only in aggregate -- the stamps say which phase of which work-group.
#ifdef A3D_PROFILE
static __device__ unsigned long long* a3d_prof_buf;
static __device__ int a3d_prof_kid = -1;
#define A3D_PROF_MAX_WG 65536
#define A3D_STAMP_(kid, slot, what)                                                                                              \
    do {                                                                                                                         \
        if (a3d_prof_kid == (kid) && threadIdx.x == 0 && threadIdx.y == 0 && threadIdx.z == 0) {                                 \
            const size_t wg_ = blockIdx.x + (size_t)gridDim.x * (blockIdx.y + (size_t)gridDim.y * blockIdx.z);                   \
            if (wg_ < A3D_PROF_MAX_WG) a3d_prof_buf[wg_ * 8 + (slot)] = what;                                                    \
        }                                                                                                                        \
    } while (0)
#define A3D_STAMP(kid, slot) A3D_STAMP_(kid, slot, wall_clock64())
#define A3D_STAMP_CLOCK(kid, slot) A3D_STAMP_(kid, slot, clock64())
#define A3D_PROFILE_TU(tu)                                                                                                       \
    extern "C" int a3d_profile_set_##tu(void* buf, int kid) {                                                                    \
        if (hipMemcpyToSymbol(HIP_SYMBOL(a3d_prof_buf), &buf, sizeof(buf)) != hipSuccess) return A3D_EHIP;                       \
        return hipMemcpyToSymbol(HIP_SYMBOL(a3d_prof_kid), &kid, sizeof(kid)) == hipSuccess ? A3D_OK : A3D_EHIP;                 \
    }
#else
#define A3D_STAMP(kid, slot) \
    do {                     \
    } while (0)
#define A3D_STAMP_CLOCK(kid, slot) \
    do {                           \
    } while (0)
#define A3D_PROFILE_TU(tu)
#endif

// lanes below me in the wave that have the bit set: ballot + mbcnt (wave64)
__device__ __forceinline__ int a3d_lane_id() { return (int)__lane_id(); }

__device__ __forceinline__ int a3d_wave_prefix(unsigned long long mask) {
    // number of set bits among lanes strictly below the calling lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// 16-byte load of data that is read exactly once (streamed): non-temporal, so it does not displace what the next kernels reuse
__device__ __forceinline__ float4 a3d_load_stream4(const float* p) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f a = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
    return make_float4(a.x, a.y, a.z, a.w);
}
__device__ __forceinline__ float a3d_load_stream(const float* p) { return __builtin_nontemporal_load(p); }

// Sum of a[lo, hi): eight independent loads in flight per step.  (A plain `for (i) s += a[i]` waits for every load before it
// issues the next one: ~1 us per element, 46 us for a 23-element run per thread in the single-work-group scans.)
__device__ __forceinline__ int a3d_run_sum(const int* __restrict__ a, int lo, int hi) {
    int s = 0, i = lo;
    for (; i + 8 <= hi; i += 8) {
        const int v0 = a[i], v1 = a[i + 1], v2 = a[i + 2], v3 = a[i + 3], v4 = a[i + 4], v5 = a[i + 5], v6 = a[i + 6], v7 = a[i + 7];
        s += ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7));
    }
    if (i + 4 <= hi) {
        const int v0 = a[i], v1 = a[i + 1], v2 = a[i + 2], v3 = a[i + 3];
        s += (v0 + v1) + (v2 + v3);
        i += 4;
    }
    if (i + 2 <= hi) {
        const int v0 = a[i], v1 = a[i + 1];
        s += v0 + v1;
        i += 2;
    }
    if (i < hi) s += a[i];
    return s;
}

// dst[i] = run + a[lo..i) for i in [lo, hi) (exclusive prefix of the run, starting from `run`), src optionally reset to `fill`; returns
// run + sum.  dst may alias a.  Eight loads in flight per step, as above.
template <bool RESET>
__device__ __forceinline__ int a3d_run_scan(int* a, int* dst, int lo, int hi, int run, int fill = 0) {
    int i = lo;
    for (; i + 8 <= hi; i += 8) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = a[i + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            dst[i + k] = run;
            if (RESET) a[i + k] = fill;
            run += v[k];
        }
    }
    if (i + 4 <= hi) {
        int v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = a[i + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dst[i + k] = run;
            if (RESET) a[i + k] = fill;
            run += v[k];
        }
        i += 4;
    }
    if (i + 2 <= hi) {
        const int v0 = a[i], v1 = a[i + 1];
        dst[i] = run; dst[i + 1] = run + v0;
        if (RESET) { a[i] = fill; a[i + 1] = fill; }
        run += v0 + v1;
        i += 2;
    }
    if (i < hi) {
        const int c = a[i];
        dst[i] = run;
        if (RESET) a[i] = fill;
        run += c;
    }
    return run;
}

// ---- cross-lane scans, sums and exchanges: the one copy of each idiom that several kernels share.  (Left where
// they are, each with one user: the quad broadcasts of skin.hip, the strided scan of rs_tri_kernel, the arg-min butterfly of bones.hip.)
// What all of them require: the lanes that exchange values reach the call TOGETHER -- the whole wave, in wave-uniform control flow,
// for everything built on DPP (the scans, a3d_lane_xor, the quad / row sums); the whole aligned group of WIDTH lanes for
// a3d_group_sum.  A lane that is switched off contributes nothing defined and the others read it all the same: the result is
// silently wrong, nothing faults.  The two a3d_block_* helpers contain barriers: EVERY thread of the work-group must arrive, or the
// work-group hangs.  They take work-groups of whole waves, numbered by threadIdx.x alone.

// DPP controls (the lane a value is read from), named once
enum {
    A3D_DPP_QUAD_XOR1 = 0xB1,        // quad_perm [1,0,3,2]: lane ^ 1
    A3D_DPP_QUAD_XOR2 = 0x4E,        // quad_perm [2,3,0,1]: lane ^ 2
    A3D_DPP_ROW_ROR8 = 0x128,        // row_ror:8: lane ^ 8
    A3D_DPP_ROW_HALF_MIRROR = 0x141, // row_half_mirror: lane ^ 7
    A3D_DPP_ROW_MIRROR = 0x140,      // row_mirror: lane ^ 15
    A3D_DPP_ROW_SHR = 0x110,         // + n: row_shr:n, lane - n of the same row of 16 (none: the destination keeps `old`)
    A3D_DPP_ROW_BCAST15 = 0x142,     // lane 15 of every row to the next row
    A3D_DPP_ROW_BCAST31 = 0x143      // lane 31 to rows 2 and 3
};
template <int CTRL>
__device__ __forceinline__ int a3d_dpp(int x) { return __builtin_amdgcn_mov_dpp(x, CTRL, 0xF, 0xF, true); }
template <int CTRL>
__device__ __forceinline__ float a3d_dpp(float x) { return __int_as_float(a3d_dpp<CTRL>(__float_as_int(x))); }

// the value of lane ^ M: a register move (DPP) where the pattern exists, ds_bpermute otherwise.  No barrier, no LDS words.
template <int M>
__device__ __forceinline__ int a3d_lane_xor(int x) {
    if (M == 1) return a3d_dpp<A3D_DPP_QUAD_XOR1>(x);
    if (M == 2) return a3d_dpp<A3D_DPP_QUAD_XOR2>(x);
    if (M == 8) return a3d_dpp<A3D_DPP_ROW_ROR8>(x);
    return __shfl_xor(x, M, 64);
}
template <int M>
__device__ __forceinline__ float a3d_lane_xor(float x) { return __int_as_float(a3d_lane_xor<M>(__float_as_int(x))); }

// sum / maximum over the aligned quad, sum over the aligned row of 16, in every lane of it: two / four DPP moves, in this order.  No
// barrier, no LDS words.
__device__ __forceinline__ float a3d_quad_sum(float r) {
    r += a3d_dpp<A3D_DPP_QUAD_XOR1>(r);
    r += a3d_dpp<A3D_DPP_QUAD_XOR2>(r);
    return r;
}
__device__ __forceinline__ float a3d_quad_max(float m) {
    m = fmaxf(m, a3d_dpp<A3D_DPP_QUAD_XOR1>(m));
    m = fmaxf(m, a3d_dpp<A3D_DPP_QUAD_XOR2>(m));
    return m;
}
__device__ __forceinline__ float a3d_row16_sum(float r) {
    r = a3d_quad_sum(r);
    r += a3d_dpp<A3D_DPP_ROW_HALF_MIRROR>(r);
    r += a3d_dpp<A3D_DPP_ROW_MIRROR>(r);
    return r;
}

// butterfly sum over every aligned group of WIDTH lanes (a power of two up to 64), in every lane of it; the offsets descend from WIDTH / 2,
// which fixes the order of a floating-point sum.  Only the group's own lanes must arrive together (the exchange is ds_bpermute): groups
// of one wave may sit in different trips of a loop.  No barrier, no LDS words.
template <int WIDTH = 64, typename T>
__device__ __forceinline__ T a3d_group_sum(T v) {
#pragma unroll
    for (int o = WIDTH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float a3d_wave_sum(float v) { return a3d_group_sum<64>(v); }

// minimum / maximum over the wave, in every lane of it (the same butterfly; neither depends on the order).  Floats go through
// a3d_ordered_key first: an unsigned key that orders like the float (negative values and -0 < +0 included), so that integer atomicMin /
// atomicMax can finish across waves what these start.  NaN is not ordered: callers keep it out.
__device__ __forceinline__ unsigned a3d_wave_min(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned a3d_wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned a3d_ordered_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float a3d_ordered_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// sum over the work-group, in every thread, in a fixed order: the butterfly per wave, then red[0] + red[1] + .. + red[WAVES-1] from the
// left.  (Starting from red[0] and not from zero: a sum whose terms are all -0 stays -0.)  Two barriers -- one BEFORE red is written,
// so the WAVES words of red may be handed to the next call right away, and one behind.
template <int WAVES, typename T>
__device__ __forceinline__ T a3d_block_sum(T v, T* red) {
    v = a3d_group_sum<64>(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) t += red[w];
    return t;
}

// inclusive prefix sum within rows of 16 lanes (row_shr 1, 2, 4, 8), and over the 64 lanes of a wave (plus row_bcast 15, 31): four / six
// DPP additions -- VALU only, no LDS crossbar (six ds_bpermute round trips in the __shfl_up form).  No barrier, no LDS words.
__device__ __forceinline__ int a3d_row16_incl_scan(int x) {
    x += __builtin_amdgcn_update_dpp(0, x, A3D_DPP_ROW_SHR + 1, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, A3D_DPP_ROW_SHR + 2, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, A3D_DPP_ROW_SHR + 4, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, A3D_DPP_ROW_SHR + 8, 0xf, 0xf, false);
    return x;
}
__device__ __forceinline__ int a3d_wave_incl_scan(int x) {
    x = a3d_row16_incl_scan(x);
    x += __builtin_amdgcn_update_dpp(0, x, A3D_DPP_ROW_BCAST15, 0xa, 0xf, false);  // -> rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, A3D_DPP_ROW_BCAST31, 0xc, 0xf, false);  // -> rows 2 and 3
    return x;
}

// exclusive prefix sum of `mine` over the work-group of WAVES waves (thread order); *total, when asked for: the sum over the whole
// work-group, in every thread.  ONE barrier, between the waves' totals going to s_wave[0..WAVES) and their being read: s_wave may be
// written again only behind a further barrier (or by a further call that itself comes behind one).  Pass `total` as a literal
// nullptr or the address of a local: the choice between the two loops below is then made when the call is inlined; a pointer only
// known at run time would keep both.
template <int WAVES>
__device__ __forceinline__ int a3d_block_excl_scan(int mine, int* s_wave, int* total = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = a3d_wave_incl_scan(mine);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int excl = incl - mine;
    if (total) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) excl += s_wave[w];
            t += s_wave[w];
        }
        *total = t;
    } else {
        for (int w = 0; w < wave; ++w) excl += s_wave[w];
    }
    return excl;
}

// eight ints into ascending order in registers: a 19-comparator network
__device__ __forceinline__ void a3d_sort8(int a[8]) {
#define A3D_CX(i, j) { const int x = min(a[i], a[j]), y = max(a[i], a[j]); a[i] = x; a[j] = y; }
    A3D_CX(0, 1) A3D_CX(2, 3) A3D_CX(4, 5) A3D_CX(6, 7)
    A3D_CX(0, 2) A3D_CX(1, 3) A3D_CX(4, 6) A3D_CX(5, 7)
    A3D_CX(1, 2) A3D_CX(5, 6) A3D_CX(0, 4) A3D_CX(3, 7)
    A3D_CX(1, 5) A3D_CX(2, 6)
    A3D_CX(1, 4) A3D_CX(3, 6)
    A3D_CX(2, 4) A3D_CX(3, 5)
    A3D_CX(3, 4)
#undef A3D_CX
}
#endif
