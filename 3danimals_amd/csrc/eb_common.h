// estimate_bones on the device: what the one-group kernel (bones.hip, eb_kernel) and the multi-group path (bones_wide.hip) share -- the
// monotone keys of the radix select, torch.quantile's rank arithmetic and torch.lerp, the bin search of one select pass, and the closed
// forms of phase D (spine joints, body bone ends, attachment joint, leg bone ends; reference skinning.py:118-141, :187-215) -- device code; and what the
// entry point needs of the other files: the launcher of the wide path, the resample tail and the launcher of the sampler (fps.hip).
#pragma once
#include <stddef.h>

#include "a3d_common.h"

// the launches of a call on the multi-work-group path (bones_wide.hip); a3d_estimate_bones (bones.hip) has validated ``args``
int eb_wide_launch(const a3d_estimate_bones_args* args, hipStream_t stream);

// The resample tail of a3d_estimate_bones (include/a3d.h describes it in words: the public struct stays as it is).  A caller that wants
// the clouds resampled first passes  size >= sizeof(a3d_estimate_bones_args) + A3D_FPS_TAIL_SIZE  and these bytes behind the public struct.
// (_lib.EbFpsTail mirrors it, registered on this header's entry of _lib.INTERNAL_SURFACES; no ``size`` of its own: it is no public struct.)
typedef struct a3d_eb_fps_tail {
    int32_t k;             /* points kept per cloud, 1 <= k <= V */
    int32_t sample_only;   /* non-zero: the sampler alone; bones, nearest, ok are not touched and may be null */
    const int64_t* start;  /* [N] on the device: each cloud's first pick (clamped into [0, V)) */
    float* sampled;        /* [N, k, 3]: the picked points, in the order picked */
    int64_t* idx;          /* [N, k]: their indices, or null */
} a3d_eb_fps_tail;
static_assert(sizeof(a3d_estimate_bones_args) % 8 == 0, "the tail follows the public struct without padding");
static_assert(sizeof(a3d_eb_fps_tail) == A3D_FPS_TAIL_SIZE, "include/a3d.h states the tail's size");
static_assert(offsetof(a3d_eb_fps_tail, k) == 0 && offsetof(a3d_eb_fps_tail, sample_only) == 4 && offsetof(a3d_eb_fps_tail, start) == 8 &&
              offsetof(a3d_eb_fps_tail, sampled) == 16 && offsetof(a3d_eb_fps_tail, idx) == 24, "include/a3d.h states the tail's byte layout");
// the sampler of a call with the tail (fps.hip); a3d_estimate_bones (bones.hip) has validated both
int eb_fps_launch(const a3d_estimate_bones_args* args, const a3d_eb_fps_tail* tail, hipStream_t stream);

#define EB_MAXSEL 12   // ranks looked for at once: 2 coordinates x 3 quantiles x the two neighbours a quantile interpolates between
#define EB_MAXGROUP 6  // ... of one coordinate

__device__ __forceinline__ unsigned eb_key(float f) {  // monotone float -> uint
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float eb_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ float eb_lerp(float a, float b, float w) { return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.f - w); }  // torch.lerp

// pos = q (n - 1) in float32, as torch.quantile computes it: the two 0-based ranks it interpolates between and the weight of the upper one
struct EbRanks { int lo, hi; float w; };
__device__ __forceinline__ EbRanks eb_ranks_of(float q, int n) {
    const float ps = q * (float)(n - 1), lo = floorf(ps), hi = ceilf(ps);
    EbRanks r;
    r.lo = max((int)lo, 0); r.hi = max((int)hi, 0); r.w = ps - lo;
    return r;
}

// One pass of the radix select for ONE target, by ONE WAVE (all 64 lanes arrive together): hist[256] = the counts of the pass's digit
// among the values that share the target's prefix (16-byte aligned: a lane reads four neighbouring bins), rank = the target's rank among
// them.  The lane whose four bins hold the rank returns true with the bin in *digit and the rank within that bin in *rest; at most one
// lane does (none when the histogram holds fewer than rank + 1 values).
__device__ __forceinline__ bool eb_find_bin(const int* hist, int rank, int* digit, int* rest) {
    const int ln = threadIdx.x & 63;
    const int4 c = reinterpret_cast<const int4*>(hist)[ln];
    const int s4 = c.x + c.y + c.z + c.w;
    const int incl = a3d_wave_incl_scan(s4), excl = incl - s4;
    if (rank < excl || rank >= incl) return false;
    int b = 4 * ln, base = excl;
    if (rank >= base + c.x) {
        base += c.x; ++b;
        if (rank >= base + c.y) {
            base += c.y; ++b;
            if (rank >= base + c.z) { base += c.z; ++b; }
        }
    }
    *digit = b; *rest = rank - base;
    return true;
}

// ---- phase D: every joint is a closed form of the two spine ends and the centroid of its instance
struct EbSpine {
    const float* p;      // the instance's vertices [V,3]
    int va, vb;          // the spine ends: arg-max / arg-min of z
    float cy, cz;        // centroid (x is snapped to 0)
    int n_body, n_leg;
    const float* blend;  // linspace(0, 1, ceil((n_body + 1) / 2))
};

__device__ __forceinline__ void eb_joint(const EbSpine& s, int j, float* o) {  // joints_a[:-1] ++ joints_b   (skinning.py:118-126)
    const int nb2 = (s.n_body + 2) / 2;
    const bool head = j < nb2 - 1;
    const int i = head ? j : j - (nb2 - 1), vi = head ? s.va : s.vb;
    const float e[3] = {0.f, s.p[3 * vi + 1], s.p[3 * vi + 2]}, mid[3] = {0.f, s.cy + (s.n_leg > 0 ? 0.5f : 0.f), s.cz};
    const float bl = s.blend[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = head ? e[c] * (1.f - bl) + mid[c] * bl : e[c] * bl + mid[c] * (1.f - bl);
}

// body bones: (i + 1, i) for the first half, then (i, i + 1) for i = n_body - 1 .. half   (skinning.py:128-141)
__device__ __forceinline__ void eb_body_end(const EbSpine& s, int bone, int e, float* o) {
    const int half = s.n_body / 2;
    const int i = bone < half ? bone : s.n_body - 1 - (bone - half);
    eb_joint(s, bone < half ? (e == 0 ? i + 1 : i) : (e == 0 ? i : i + 1), o);
}

// attachment joint of a leg: the body bone whose end is nearest in z to the foot, first index on ties   (skinning.py:187-192)
__device__ __forceinline__ int eb_nearest_body_bone(const EbSpine& s, float foot_z) {
    float bd = INFINITY;
    int att = 0;
    for (int k = 0; k < s.n_body; ++k) {
        float o[3];
        eb_body_end(s, k, 1, o);
        const float d = fabsf(o[2] - foot_z);
        if (d < bd) { bd = d; att = k; }
    }
    return att;
}

// end e of leg bone i = (joint i + 1, joint i) of the ramp foot -> attachment   (skinning.py:196-215)
__device__ __forceinline__ void eb_leg_end(const EbSpine& s, const float* __restrict__ foot, int attach, const float* ramp, int i, int e, float* o) {
    float anchor[3];
    eb_body_end(s, attach, 1, anchor);  // bones_pred[:, :, body_bone_idx, 1]
    const float rm = ramp[e == 0 ? i + 1 : i];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = foot[c] * (1.f - rm) + anchor[c] * rm;
}
