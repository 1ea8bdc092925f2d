// The camera-pose glue of the predictors on gfx950 (csrc/pose.h): what stands between the pose network and the
// first mesh operation in the reference.
//
// Heads (InstancePredictorBase.py:257-304), pick (:623-663; InstancePredictorFauna.py:37-77) with lookat_forward_to_rot_matrix
// (:706-714) and cameras (:606-620) are one device function each with its adjoint; the fused kernels compose them, the stand-alone
// camera kernels call the last one alone.  The work per image is a few hundred operations on at most 35 inputs: ONE THREAD PER IMAGE,
// 256-thread work-groups, everything in registers (the per-hypothesis arrays are indexed by unrolled loops only), no LDS, no barrier.
// The backward recomputes the forward from raw and the two permutations and writes every element of g_raw once: no memset, no
// atomics, the same bits on every run.
//
// Built with -ffp-contract=off: the arithmetic restates the torch statements of 3danimals_amd/pose.py operation by operation, rounding
// to float32 where torch rounds; only the transcendentals (tanh, exp, log1p, cos, sin) are taken in double and rounded once.  The
// products with the zeros of the up vector, of the projection and of the rotation about y are kept, so a non-finite input reaches the
// outputs it reaches in torch; maxima and clamps propagate a NaN as torch's do.
#include "pose.h"
#include "a3d_common.h"

namespace {

constexpr int PO_THREADS = 256;
constexpr int MAXH = A3D_POSE_MAX_HYPOS;
constexpr float SOFTPLUS_BETA = 1.3862943611198906f;  // ln 2 / 0.5
constexpr float NORM_EPS = 1e-12f;

struct V3 {
    float x, y, z;
};

struct Proj {
    float m[16];
};

struct PoseArgs {
    const float *raw, *signs, *max_trans;
    const long long *rand_perm, *best_perm;
    int N, H, oct, zeroy;
    float temp, naive_weight, one_minus_weight, offset_z;
    long long best_below;
    Proj P;
};

struct PoseOut {
    float *poses_raw, *pose_raw, *pose, *mvp, *w2c, *campos, *rot_prob, *rot_logit, *rots_probs;
    long long *rot_idx, *rand_flag;
};

struct PoseGrads {
    const float *poses_raw, *pose_raw, *pose, *mvp, *w2c, *campos, *rot_prob, *rot_logit, *rots_probs;
    float* g_raw;
};

__device__ __forceinline__ float opt(const float* p, long long i) { return p ? p[i] : 0.0f; }

__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// ---------------------------------------------------------------------------------------------------------------- F.normalize
// v / max(|v|, 1e-12); a NaN norm stays a NaN (clamp_min propagates it)
__device__ __forceinline__ float norm_of(V3 v) { return sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z); }
__device__ __forceinline__ float clamp_norm(float n) { return n < NORM_EPS ? NORM_EPS : n; }

__device__ __forceinline__ V3 normalize(V3 v) {
    const float d = clamp_norm(norm_of(v));
    return {v.x / d, v.y / d, v.z / d};
}

// autograd's chain for v / norm(v).clamp_min(eps): g / d, minus the part through d where the clamp lets it pass (n >= eps) and the norm
// has a slope (n != 0)
__device__ __forceinline__ V3 normalize_adj(V3 v, V3 g) {
    const float n = norm_of(v), d = clamp_norm(n);
    V3 gv = {g.x / d, g.y / d, g.z / d};
    if (n >= NORM_EPS) {
        const float dd = d * d;
        const float gd = -(((g.x * v.x) / dd + (g.y * v.y) / dd) + (g.z * v.z) / dd);
        const float s = gd / n;
        gv.x += v.x * s;
        gv.y += v.y * s;
        gv.z += v.z * s;
    }
    return gv;
}

// ---------------------------------------------------------------------------------------------------------------- heads
// F.softplus(x, beta): x itself where beta * x > 20
__device__ __forceinline__ float softplus(float x) {
    const float bx = x * SOFTPLUS_BETA;
    return bx > 20.0f ? x : (float)log1p(exp((double)bx)) / SOFTPLUS_BETA;
}

__device__ __forceinline__ float softplus_slope(float x) {
    const float bx = x * SOFTPLUS_BETA;
    if (bx > 20.0f) return 1.0f;
    const double z = exp((double)bx);
    return (float)(z / (z + 1.0));
}

// the forward vector of one hypothesis before its normalisation: (softplus(x), y', softplus(z)) * signs
__device__ __forceinline__ V3 head_vector(const float* __restrict__ r, const float* __restrict__ s, int oct, int zeroy) {
    float y = oct ? softplus(r[1]) : r[1];
    if (zeroy) y = y * 0.0f;
    return {softplus(r[0]) * s[0], y * s[1], softplus(r[2]) * s[2]};
}

__device__ __forceinline__ V3 head_adj(const float* __restrict__ r, const float* __restrict__ s, int oct, int zeroy, V3 g) {
    const V3 gv = normalize_adj(head_vector(r, s, oct, zeroy), g);
    float gy = gv.y * s[1];
    if (zeroy) gy = gy * 0.0f;
    if (oct) gy = gy * softplus_slope(r[1]);
    return {(gv.x * s[0]) * softplus_slope(r[0]), gy, (gv.z * s[2]) * softplus_slope(r[2])};
}

__device__ __forceinline__ float tanh32(float x) { return (float)tanh((double)x); }

// ---------------------------------------------------------------------------------------------------------------- look-at
// rows right = normalize(up x f), up' = normalize(f x right), f; up = (0, 1, 0)
__device__ __forceinline__ void lookat(V3 f, float* __restrict__ R) {
    const V3 up = {0.0f, 1.0f, 0.0f};
    const V3 r = normalize(cross(up, f));
    const V3 u = normalize(cross(f, r));
    R[0] = r.x, R[1] = r.y, R[2] = r.z;
    R[3] = u.x, R[4] = u.y, R[5] = u.z;
    R[6] = f.x, R[7] = f.y, R[8] = f.z;
}

// c = a x b:  g_a = b x g_c,  g_b = g_c x a
__device__ __forceinline__ V3 lookat_adj(V3 f, const float* __restrict__ gR) {
    const V3 up = {0.0f, 1.0f, 0.0f};
    const V3 c0 = cross(up, f);
    const V3 r = normalize(c0);
    const V3 c1 = cross(f, r);
    const V3 g_c1 = normalize_adj(c1, {gR[3], gR[4], gR[5]});
    const V3 a = cross(r, g_c1), b = cross(g_c1, f);
    const V3 g_r = {gR[0] + b.x, gR[1] + b.y, gR[2] + b.z};
    const V3 g_c0 = normalize_adj(c0, g_r);
    const V3 c = cross(g_c0, up);
    return {(gR[6] + a.x) + c.x, (gR[7] + a.y) + c.y, (gR[8] + a.z) + c.z};
}

// ---------------------------------------------------------------------------------------------------------------- cameras
__device__ __forceinline__ void mat4_mul(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            C[4 * i + j] = ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * B[12 + j];
}

// pose = (R row-major, t) -> w2c, mvp = P w2c, campos = -R (t + (0, 0, offset_z))
__device__ __forceinline__ void cameras(const float* __restrict__ pose, float offset_z, const Proj& P, float* __restrict__ w2c, float* __restrict__ mvp,
                                        float* __restrict__ campos) {
    const float T[3] = {pose[9] + 0.0f, pose[10] + 0.0f, pose[11] + offset_z};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) w2c[4 * i + j] = pose[3 * j + i];
        w2c[4 * i + 3] = T[i];
        campos[i] = -((pose[3 * i] * T[0] + pose[3 * i + 1] * T[1]) + pose[3 * i + 2] * T[2]);
    }
    w2c[12] = 0.0f, w2c[13] = 0.0f, w2c[14] = 0.0f, w2c[15] = 1.0f;
    mat4_mul(P.m, w2c, mvp);
}

// g_mvp, g_w2c [16], g_campos [3] (NULL: absent) of image n -> g_pose [12]
__device__ __forceinline__ void cameras_adj(const float* __restrict__ pose, float offset_z, const Proj& P, const float* g_mvp, const float* g_w2c,
                                            const float* g_campos, float* __restrict__ g_pose) {
    const float T[3] = {pose[9] + 0.0f, pose[10] + 0.0f, pose[11] + offset_z};
    float G[12];  // the gradient of the first three rows of w2c
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = opt(g_w2c, 4 * k + j);
            if (g_mvp) acc += ((P.m[k] * g_mvp[j] + P.m[4 + k] * g_mvp[4 + j]) + P.m[8 + k] * g_mvp[8 + j]) + P.m[12 + k] * g_mvp[12 + j];
            G[4 * k + j] = acc;
        }
    const float c[3] = {opt(g_campos, 0), opt(g_campos, 1), opt(g_campos, 2)};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) g_pose[3 * i + j] = G[4 * j + i] + (-c[i]) * T[j];
        g_pose[9 + i] = G[4 * i + 3] + -((pose[i] * c[0] + pose[3 + i] * c[1]) + pose[6 + i] * c[2]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- pick
// rots_probs of one image into q[], the softmax itself into s[] (h < H; the loops are unrolled so both stay in registers), and the
// argmax: the first NaN, else the lowest index among equal maxima
__device__ __forceinline__ int blended_probs(const float* __restrict__ r, const PoseArgs& a, float* q, float* s) {
    const int H = a.H;
    float z[MAXH], m = 0.0f;
#pragma unroll
    for (int h = 0; h < MAXH; ++h)
        if (h < H) {
            z[h] = -r[4 * h] / a.temp;
            if (h == 0 || (m == m && (z[h] > m || z[h] != z[h]))) m = z[h];  // (a NaN wins and stays)
        }
    float sum = 0.0f;
#pragma unroll
    for (int h = 0; h < MAXH; ++h)
        if (h < H) {
            s[h] = (float)exp((double)(z[h] - m));
            sum += s[h];
        }
    const float naive = 1.0f / (float)H;
    int best = 0;
    float bv = 0.0f;
#pragma unroll
    for (int h = 0; h < MAXH; ++h)
        if (h < H) {
            s[h] = s[h] / sum;
            q[h] = naive * a.naive_weight + s[h] * a.one_minus_weight;
            if (h == 0 || (bv == bv && (q[h] > bv || q[h] != q[h]))) best = h, bv = q[h];
        }
    return best;
}

__device__ __forceinline__ int picked(int best, int n, const PoseArgs& a, int* random) {
    *random = 0;
    if (a.best_perm == nullptr || a.best_perm[n] < a.best_below) return best;
    *random = 1;
    const long long m = a.rand_perm[n] % (long long)a.H;  // (torch's %: never negative, whatever the caller passed for a permutation)
    return (int)(m < 0 ? m + a.H : m);
}

__global__ __launch_bounds__(PO_THREADS) void pose_cameras_fwd_kernel(const PoseArgs a, const PoseOut o) {
    const int n = blockIdx.x * PO_THREADS + threadIdx.x;
    if (n >= a.N) return;
    const int H = a.H, W = 4 * H + 3;
    const float* r = a.raw + (long long)n * W;
    float* pr = o.poses_raw + (long long)n * W;
    float q[MAXH], s[MAXH];
    int random;
    const int idx = picked(blended_probs(r, a, q, s), n, a, &random);
    float t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pr[4 * H + i] = t[i] = tanh32(r[4 * H + i]) * a.max_trans[i];
    V3 f = {0.0f, 0.0f, 0.0f};
    float prob = 0.0f, logit = 0.0f;
#pragma unroll
    for (int h = 0; h < MAXH; ++h)
        if (h < H) {
            const V3 v = normalize(head_vector(r + 4 * h + 1, a.signs + 3 * h, a.oct, a.zeroy));
            pr[4 * h] = r[4 * h];
            pr[4 * h + 1] = v.x, pr[4 * h + 2] = v.y, pr[4 * h + 3] = v.z;
            o.rots_probs[(long long)n * H + h] = q[h];
            if (h == idx) f = v, prob = q[h], logit = r[4 * h];
        }
    o.rot_idx[n] = idx;
    o.rand_flag[n] = random;
    o.rot_prob[n] = prob;
    o.rot_logit[n] = logit;
    float* praw = o.pose_raw + (long long)n * 6;
    praw[0] = f.x, praw[1] = f.y, praw[2] = f.z, praw[3] = t[0], praw[4] = t[1], praw[5] = t[2];
    float pose[12], w2c[16], mvp[16], campos[3];
    lookat(f, pose);
    pose[9] = t[0], pose[10] = t[1], pose[11] = t[2];
    cameras(pose, a.offset_z, a.P, w2c, mvp, campos);
#pragma unroll
    for (int i = 0; i < 12; ++i) o.pose[(long long)n * 12 + i] = pose[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) o.w2c[(long long)n * 16 + i] = w2c[i], o.mvp[(long long)n * 16 + i] = mvp[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) o.campos[(long long)n * 3 + i] = campos[i];
}

__global__ __launch_bounds__(PO_THREADS) void pose_cameras_bwd_kernel(const PoseArgs a, const PoseGrads g) {
    const int n = blockIdx.x * PO_THREADS + threadIdx.x;
    if (n >= a.N) return;
    const int H = a.H, W = 4 * H + 3;
    const float* r = a.raw + (long long)n * W;
    float* gr = g.g_raw + (long long)n * W;
    const float* gpr = g.poses_raw ? g.poses_raw + (long long)n * W : nullptr;
    float q[MAXH], s[MAXH];
    int random;
    const int idx = picked(blended_probs(r, a, q, s), n, a, &random);
    // ---- the pose of the picked hypothesis again, and what arrives at it
    float t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tanh32(r[4 * H + i]) * a.max_trans[i];
    const V3 f = normalize(head_vector(r + 4 * idx + 1, a.signs + 3 * idx, a.oct, a.zeroy));
    float pose[12], g_pose[12];
    lookat(f, pose);
    pose[9] = t[0], pose[10] = t[1], pose[11] = t[2];
    const bool cams = g.mvp || g.w2c || g.campos;
    if (cams)
        cameras_adj(pose, a.offset_z, a.P, g.mvp ? g.mvp + (long long)n * 16 : nullptr, g.w2c ? g.w2c + (long long)n * 16 : nullptr,
                    g.campos ? g.campos + (long long)n * 3 : nullptr, g_pose);
#pragma unroll
    for (int i = 0; i < 12; ++i) g_pose[i] = opt(g.pose, (long long)n * 12 + i) + (cams ? g_pose[i] : 0.0f);
    const bool rotates = g.pose || cams;
    V3 g_f = {opt(g.pose_raw, (long long)n * 6), opt(g.pose_raw, (long long)n * 6 + 1), opt(g.pose_raw, (long long)n * 6 + 2)};
    if (rotates) {
        const V3 l = lookat_adj(f, g_pose);
        g_f.x += l.x, g_f.y += l.y, g_f.z += l.z;
    }
    const bool picked_fed = rotates || g.pose_raw;
    // ---- the translation: tanh(t) * max_trans
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float th = tanh32(r[4 * H + i]);
        const float up = (opt(gpr, 4 * H + i) + opt(g.pose_raw, (long long)n * 6 + 3 + i)) + g_pose[9 + i];
        gr[4 * H + i] = (up * a.max_trans[i]) * (1.0f - th * th);
    }
    // ---- the logits: straight through, the picked one's rot_logit, and the softmax under the blend
    const bool soft = g.rots_probs || g.rot_prob;
    float gs[MAXH], dot = 0.0f;
#pragma unroll
    for (int h = 0; h < MAXH; ++h)
        if (h < H) {
            gs[h] = (opt(g.rots_probs, (long long)n * H + h) + (h == idx ? opt(g.rot_prob, n) : 0.0f)) * a.one_minus_weight;
            dot += gs[h] * s[h];
        }
#pragma unroll
    for (int h = 0; h < MAXH; ++h)
        if (h < H) {
            float gl = opt(gpr, 4 * h) + (h == idx ? opt(g.rot_logit, n) : 0.0f);
            if (soft) gl += -((s[h] * (gs[h] - dot)) / a.temp);
            gr[4 * h] = gl;
            // ---- the forward vector: through poses_raw, and for the picked one through everything behind the pick
            const bool fed = gpr || (h == idx && picked_fed);
            V3 gv = {opt(gpr, 4 * h + 1), opt(gpr, 4 * h + 2), opt(gpr, 4 * h + 3)};
            if (h == idx) gv.x += g_f.x, gv.y += g_f.y, gv.z += g_f.z;
            const V3 out = fed ? head_adj(r + 4 * h + 1, a.signs + 3 * h, a.oct, a.zeroy, gv) : V3{0.0f, 0.0f, 0.0f};
            gr[4 * h + 1] = out.x, gr[4 * h + 2] = out.y, gr[4 * h + 3] = out.z;
        }
}

__global__ __launch_bounds__(PO_THREADS) void cameras_from_pose_fwd_kernel(const float* __restrict__ pose, int N, float offset_z, const Proj P,
                                                                           float* __restrict__ mvp_out, float* __restrict__ w2c_out,
                                                                           float* __restrict__ campos_out) {
    const int n = blockIdx.x * PO_THREADS + threadIdx.x;
    if (n >= N) return;
    float p[12], w2c[16], mvp[16], campos[3];
#pragma unroll
    for (int i = 0; i < 12; ++i) p[i] = pose[(long long)n * 12 + i];
    cameras(p, offset_z, P, w2c, mvp, campos);
#pragma unroll
    for (int i = 0; i < 16; ++i) w2c_out[(long long)n * 16 + i] = w2c[i], mvp_out[(long long)n * 16 + i] = mvp[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) campos_out[(long long)n * 3 + i] = campos[i];
}

__global__ __launch_bounds__(PO_THREADS) void cameras_from_pose_bwd_kernel(const float* __restrict__ pose, int N, float offset_z, const Proj P,
                                                                           const float* g_mvp, const float* g_w2c, const float* g_campos,
                                                                           float* __restrict__ g_pose_out) {
    const int n = blockIdx.x * PO_THREADS + threadIdx.x;
    if (n >= N) return;
    float p[12], g_pose[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) p[i] = pose[(long long)n * 12 + i];
    cameras_adj(p, offset_z, P, g_mvp ? g_mvp + (long long)n * 16 : nullptr, g_w2c ? g_w2c + (long long)n * 16 : nullptr,
                g_campos ? g_campos + (long long)n * 3 : nullptr, g_pose);
#pragma unroll
    for (int i = 0; i < 12; ++i) g_pose_out[(long long)n * 12 + i] = g_pose[i];
}

__global__ __launch_bounds__(PO_THREADS) void random_view_cameras_kernel(const float* __restrict__ w2c_pred, const long long* __restrict__ rand_degree,
                                                                         int b, float delta_angle, const Proj P, float* __restrict__ mvp_out,
                                                                         float* __restrict__ w2c_out, float* __restrict__ campos_out) {
    const int n = blockIdx.x * PO_THREADS + threadIdx.x;
    if (n >= b) return;
    const float angle = delta_angle * (float)rand_degree[n];
    const float c = (float)cos((double)angle), s = (float)sin((double)angle);
    const float D[16] = {c, 0.0f, s, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, -s, 0.0f, c, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float w2c[16] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float cp[3], pw[16], mvp[16];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        w2c[4 * i + 3] = w2c_pred[(long long)n * 16 + 4 * i + 3];
        cp[i] = -w2c[4 * i + 3];
    }
    mat4_mul(P.m, w2c, pw);
    mat4_mul(pw, D, mvp);
#pragma unroll
    for (int i = 0; i < 16; ++i) w2c_out[(long long)n * 16 + i] = w2c[i], mvp_out[(long long)n * 16 + i] = mvp[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) campos_out[(long long)n * 3 + i] = (D[i] * cp[0] + D[4 + i] * cp[1]) + D[8 + i] * cp[2];
}

Proj proj_of(const float* proj) {
    Proj P;
    for (int i = 0; i < 16; ++i) P.m[i] = proj[i];
    return P;
}

}  // namespace

#define PO_CHECK_IMAGES(N) A3D_CHECK_ARG((N) >= 1 && (N) <= A3D_POSE_MAX_IMAGES)
#define PO_CHECK_FUSED()                                                                                              \
    A3D_CHECK_ARG(H >= 1 && H <= A3D_POSE_MAX_HYPOS);                                                                 \
    PO_CHECK_IMAGES(N);                                                                                               \
    A3D_CHECK_ARG((long long)N * (4 * H + 3) < (1ll << 31));                                                          \
    A3D_CHECK_ARG(raw && orthant_signs && max_trans && proj && (rand_perm == nullptr) == (best_perm == nullptr));     \
    A3D_CHECK_ARG(best_below >= 0 && best_below <= N)

static PoseArgs pose_args(const float* raw, const float* orthant_signs, const float* max_trans, const int64_t* rand_perm, const int64_t* best_perm,
                          int N, int H, int oct, int zeroy, float temp, float naive_weight, float one_minus_weight, int64_t best_below,
                          float offset_z, const float* proj) {
    PoseArgs a;
    a.raw = raw, a.signs = orthant_signs, a.max_trans = max_trans;
    a.rand_perm = (const long long*)rand_perm, a.best_perm = (const long long*)best_perm;
    a.N = N, a.H = H, a.oct = oct, a.zeroy = zeroy;
    a.temp = temp, a.naive_weight = naive_weight, a.one_minus_weight = one_minus_weight, a.offset_z = offset_z;
    a.best_below = best_below;
    a.P = proj_of(proj);
    return a;
}

extern "C" int a3d_pose_cameras_fwd(const float* raw, const float* orthant_signs, const float* max_trans, const int64_t* rand_perm,
                                    const int64_t* best_perm, int N, int H, int oct, int zeroy, float temp, float naive_weight,
                                    float one_minus_weight, int64_t best_below, float offset_z, const float* proj, float* poses_raw, float* pose_raw,
                                    float* pose, float* mvp, float* w2c, float* campos, int64_t* rot_idx, float* rot_prob, float* rot_logit,
                                    float* rots_probs, int64_t* rand_flag, a3d_stream_t stream) {
    PO_CHECK_FUSED();
    A3D_CHECK_ARG(poses_raw && pose_raw && pose && mvp && w2c && campos && rot_idx && rot_prob && rot_logit && rots_probs && rand_flag);
    const PoseArgs a = pose_args(raw, orthant_signs, max_trans, rand_perm, best_perm, N, H, oct, zeroy, temp, naive_weight, one_minus_weight,
                                 best_below, offset_z, proj);
    PoseOut o;
    o.poses_raw = poses_raw, o.pose_raw = pose_raw, o.pose = pose, o.mvp = mvp, o.w2c = w2c, o.campos = campos;
    o.rot_prob = rot_prob, o.rot_logit = rot_logit, o.rots_probs = rots_probs;
    o.rot_idx = (long long*)rot_idx, o.rand_flag = (long long*)rand_flag;
    hipLaunchKernelGGL(pose_cameras_fwd_kernel, dim3(a3d_div_up(N, PO_THREADS)), dim3(PO_THREADS), 0, (hipStream_t)stream, a, o);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_pose_cameras_bwd(const float* raw, const float* orthant_signs, const float* max_trans, const int64_t* rand_perm,
                                    const int64_t* best_perm, int N, int H, int oct, int zeroy, float temp, float naive_weight,
                                    float one_minus_weight, int64_t best_below, float offset_z, const float* proj, const float* g_poses_raw,
                                    const float* g_pose_raw, const float* g_pose, const float* g_mvp, const float* g_w2c, const float* g_campos,
                                    const float* g_rot_prob, const float* g_rot_logit, const float* g_rots_probs, float* g_raw,
                                    a3d_stream_t stream) {
    PO_CHECK_FUSED();
    A3D_CHECK_ARG(g_raw);
    const PoseArgs a = pose_args(raw, orthant_signs, max_trans, rand_perm, best_perm, N, H, oct, zeroy, temp, naive_weight, one_minus_weight,
                                 best_below, offset_z, proj);
    PoseGrads g;
    g.poses_raw = g_poses_raw, g.pose_raw = g_pose_raw, g.pose = g_pose, g.mvp = g_mvp, g.w2c = g_w2c, g.campos = g_campos;
    g.rot_prob = g_rot_prob, g.rot_logit = g_rot_logit, g.rots_probs = g_rots_probs;
    g.g_raw = g_raw;
    hipLaunchKernelGGL(pose_cameras_bwd_kernel, dim3(a3d_div_up(N, PO_THREADS)), dim3(PO_THREADS), 0, (hipStream_t)stream, a, g);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_cameras_from_pose_fwd(const float* pose, int N, float offset_z, const float* proj, float* mvp, float* w2c, float* campos,
                                         a3d_stream_t stream) {
    PO_CHECK_IMAGES(N);
    A3D_CHECK_ARG(pose && proj && mvp && w2c && campos);
    hipLaunchKernelGGL(cameras_from_pose_fwd_kernel, dim3(a3d_div_up(N, PO_THREADS)), dim3(PO_THREADS), 0, (hipStream_t)stream, pose, N, offset_z,
                       proj_of(proj), mvp, w2c, campos);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_cameras_from_pose_bwd(const float* pose, int N, float offset_z, const float* proj, const float* g_mvp, const float* g_w2c,
                                         const float* g_campos, float* g_pose, a3d_stream_t stream) {
    PO_CHECK_IMAGES(N);
    A3D_CHECK_ARG(pose && proj && g_pose && (g_mvp || g_w2c || g_campos));
    hipLaunchKernelGGL(cameras_from_pose_bwd_kernel, dim3(a3d_div_up(N, PO_THREADS)), dim3(PO_THREADS), 0, (hipStream_t)stream, pose, N, offset_z,
                       proj_of(proj), g_mvp, g_w2c, g_campos, g_pose);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_random_view_cameras(const float* w2c_pred, const int64_t* rand_degree, int b, float delta_angle, const float* proj, float* mvp,
                                       float* w2c, float* campos, a3d_stream_t stream) {
    PO_CHECK_IMAGES(b);
    A3D_CHECK_ARG(w2c_pred && rand_degree && proj && mvp && w2c && campos);
    hipLaunchKernelGGL(random_view_cameras_kernel, dim3(a3d_div_up(b, PO_THREADS)), dim3(PO_THREADS), 0, (hipStream_t)stream, w2c_pred,
                       (const long long*)rand_degree, b, delta_angle, proj_of(proj), mvp, w2c, campos);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
