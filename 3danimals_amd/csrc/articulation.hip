// The articulation glue of the posing path on gfx950 (csrc/articulation.h): what stands between estimate_bones and
// skinning in the reference's predictors besides the network itself.
//
// Descriptors (InstancePredictorBase.py:337-382, 391-432; InstancePredictorFauna.py:102-147).  A work-group owns (image, chunk of
// A3D_ARTICULATION_CHUNK feature columns).  Forward: every work-group projects the K midpoints into LDS for itself (K <= 64: cheaper than
// a second launch or a trip through memory), the first chunk's work-group also writes the nine position columns; a chunk of global
// columns copies feat[n], a chunk of sampled columns evaluates grid_sample's bilinear rule, lanes on the columns (the output's unit
// stride).  Backward: the work-group of a chunk of sampled channels of image n owns EVERY pixel of those channels, so it zero-fills its
// slab itself, waits at a barrier and then stores the sums of the taps -- no memset of the whole gradient, no atomics.  The 4 K taps of
// the image are threaded into per-pixel chains in LDS (a tap's successor is the next tap, in the order k ascending then (y0,x0) (y0,x1)
// (y1,x0) (y1,x1), that hits the same pixel); the thread of (chain head, channel) adds its chain front to back and stores once, which
// is the sum "bone by bone in a fixed order" without a read-modify-write of memory.  The zero-fill puts its lanes on whichever of the
// channel and pixel strides is 1.
//
// Limits (:435-511, Fauna :149-213, :229-230; AnimalModel.py:313-314): S[k,c] * tanh(m x) and mean(angles^2), one work-group striding
// over the N K 3 elements, tanh in double (the backward recomputes it: S may be 0), the squares added with a3d_block_sum.
//
// Built with -ffp-contract=off: the pixel-coordinate arithmetic restates grid_sample's ((x + 1) * size - 1) / 2 and its four weights
// operation by operation.
#include "articulation.h"
#include "a3d_common.h"

namespace {

constexpr int AR_THREADS = 256;
constexpr int CH = A3D_ARTICULATION_CHUNK;
constexpr int AR_ROWS = AR_THREADS / CH;  // (bone | tap | pixel) rows a pass of the work-group covers with its lanes on the columns
constexpr int MAXK = A3D_ARTICULATION_MAX_BONES;
static_assert((CH & (CH - 1)) == 0 && CH <= AR_THREADS, "a chunk is a power of two of lanes");
static_assert(4 * MAXK <= AR_THREADS, "one thread per tap of an image");

constexpr int CA_THREADS = 1024;
constexpr int CA_WAVES = CA_THREADS / A3D_WAVE;

struct FwdArgs {
    const float *bones, *mvp, *w2c, *feat, *patch;
    float z_offset, spatial_scale;
    long long sn, sc, sh, sw;
    int bones_shared, K, D, C, h, w;
    float *bones_feat, *pos_in;
};

struct BwdArgs {
    const float *g, *pos_in;
    int K, D, C, h, w, chunks_d;
    float *g_feat, *g_patch;
    long long gn, gc, gh, gw;
};

// the four taps of one sample: tap (j, i) is pixel (yi[j], xi[i]) with weight wx[i] * wy[j], alive when yin[j] && xin[i]
struct Taps {
    int xi[2], yi[2];
    bool xin[2], yin[2];
    float wx[2], wy[2];
};

// grid_sample(mode bilinear, padding zeros, align_corners false) of one coordinate pair.  Inside / outside is decided on the floating-point
// floor, before any conversion to an integer (1e30, or a pixel coordinate that overflowed to infinity, is outside); a coordinate that is
// not finite has no tap at all.
__device__ __forceinline__ Taps taps_of(float x, float y, int h, int w) {
    Taps t;
    const bool finite = fabsf(x) < INFINITY && fabsf(y) < INFINITY;  // (false for a NaN)
    const float ix = ((x + 1.0f) * (float)w - 1.0f) / 2.0f;
    const float iy = ((y + 1.0f) * (float)h - 1.0f) / 2.0f;
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float x1 = x0 + 1.0f, y1 = y0 + 1.0f;
    t.wx[0] = x1 - ix;
    t.wx[1] = ix - x0;
    t.wy[0] = y1 - iy;
    t.wy[1] = iy - y0;
    const float xs[2] = {x0, x1}, ys[2] = {y0, y1};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        t.xin[i] = finite && xs[i] >= 0.0f && xs[i] <= (float)(w - 1);
        t.yin[i] = finite && ys[i] >= 0.0f && ys[i] <= (float)(h - 1);
        t.xi[i] = t.xin[i] ? (int)xs[i] : 0;
        t.yi[i] = t.yin[i] ? (int)ys[i] : 0;
    }
    return t;
}

// row r of a row-major 4x4 applied to (p, 1)
__device__ __forceinline__ float row_dot(const float* __restrict__ M, int r, float x, float y, float z) {
    return ((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3];
}

__global__ __launch_bounds__(AR_THREADS) void bone_inputs_fwd_kernel(const FwdArgs a) {
    __shared__ float s_x[MAXK], s_y[MAXK];
    const int n = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x, K = a.K;
    if (t < K) {
        const float* b = a.bones + (a.bones_shared ? 0ll : (long long)n * K * 6) + t * 6;
        const float* M = a.mvp + (long long)n * 16;
        const float mx = (b[0] + b[3]) / 2.0f, my = (b[1] + b[4]) / 2.0f, mz = (b[2] + b[5]) / 2.0f;
        const float cw = row_dot(M, 3, mx, my, mz);
        const float x = row_dot(M, 0, mx, my, mz) / cw, y = row_dot(M, 1, mx, my, mz) / cw;
        s_x[t] = x;
        s_y[t] = y;
        if (chunk == 0) {
            const float* V = a.w2c + (long long)n * 16;
            float* p = a.pos_in + ((long long)n * K + t) * 9;
            p[0] = x;
            p[1] = y;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float px = b[3 * e], py = b[3 * e + 1], pz = b[3 * e + 2];
                const float vw = row_dot(V, 3, px, py, pz);
                p[2 + 3 * e] = row_dot(V, 0, px, py, pz) / vw / a.spatial_scale * 2.0f;
                p[3 + 3 * e] = row_dot(V, 1, px, py, pz) / vw / a.spatial_scale * 2.0f;
                p[4 + 3 * e] = (row_dot(V, 2, px, py, pz) / vw + a.z_offset) / a.spatial_scale * 2.0f;
            }
            p[8] = ((float)t + 0.5f) / (float)K * 2.0f - 1.0f;
        }
    }
    const int Dt = a.D + a.C;
    if (Dt == 0) return;
    __syncthreads();
    const int chunks_d = (a.D + CH - 1) / CH;
    const int tc = t & (CH - 1), tr = t / CH;
    if (chunk < chunks_d) {  // global columns: feat[n] under every bone
        const int c = chunk * CH + tc;
        if (c >= a.D) return;
        const float v = a.feat[(long long)n * a.D + c];
        for (int k = tr; k < K; k += AR_ROWS) a.bones_feat[((long long)n * K + k) * Dt + c] = v;
        return;
    }
    const int c = (chunk - chunks_d) * CH + tc;
    if (c >= a.C) return;
    const float* src = a.patch + (long long)n * a.sn + (long long)c * a.sc;
    for (int k = tr; k < K; k += AR_ROWS) {
        const Taps tp = taps_of(s_x[k], s_y[k], a.h, a.w);
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (tp.yin[j] && tp.xin[i]) acc += src[(long long)tp.yi[j] * a.sh + (long long)tp.xi[i] * a.sw] * (tp.wx[i] * tp.wy[j]);
        a.bones_feat[((long long)n * K + k) * Dt + a.D + c] = acc;
    }
}

__device__ __forceinline__ long long pixel_offset(int p, int w, long long gh, long long gw, bool linear) {
    if (linear) return (long long)p * gw;
    const int y = p / w;
    return (long long)y * gh + (long long)(p - y * w) * gw;
}

__global__ __launch_bounds__(AR_THREADS) void bone_inputs_bwd_kernel(const BwdArgs a) {
    __shared__ int s_pix[4 * MAXK], s_next[4 * MAXK], s_head[4 * MAXK];
    __shared__ float s_wt[4 * MAXK];
    const int n = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x, K = a.K;
    const int Dt = a.D + a.C;
    const int tc = t & (CH - 1), tr = t / CH;
    const float* g = a.g + (long long)n * K * Dt;
    if (chunk < a.chunks_d) {  // the global columns: sum over the bones, k ascending
        const int c = chunk * CH + tc;
        if (tr != 0 || c >= a.D) return;
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) acc += g[(long long)k * Dt + c];
        a.g_feat[(long long)n * a.D + c] = acc;
        return;
    }
    // ---- the taps of this image, one per thread, then each tap's successor on the same pixel and whether it is the first there
    const int R = 4 * K;
    if (t < R) {
        const int k = t >> 2, j = (t >> 1) & 1, i = t & 1;
        const float* p = a.pos_in + ((long long)n * K + k) * 9;
        const Taps tp = taps_of(p[0], p[1], a.h, a.w);
        // (selects, not tp.yi[j]: a run-time index would move the struct out of registers)
        const bool alive = (j ? tp.yin[1] : tp.yin[0]) && (i ? tp.xin[1] : tp.xin[0]);
        s_pix[t] = alive ? (j ? tp.yi[1] : tp.yi[0]) * a.w + (i ? tp.xi[1] : tp.xi[0]) : -1;
        s_wt[t] = (i ? tp.wx[1] : tp.wx[0]) * (j ? tp.wy[1] : tp.wy[0]);
    }
    __syncthreads();
    if (t < R) {
        const int mine = s_pix[t];
        int head = mine >= 0, next = -1;
        for (int q = 0; q < t; ++q) head &= s_pix[q] != mine;
        for (int q = R - 1; q > t; --q) next = (s_pix[q] == mine) ? q : next;
        s_head[t] = head;
        s_next[t] = mine >= 0 ? next : -1;
    }
    // ---- zero-fill the slab this work-group owns: channels [c0, c0 + cn) of image n, every pixel
    const int c0 = (chunk - a.chunks_d) * CH, cn = min(CH, a.C - c0), hw = a.h * a.w;
    float* slab = a.g_patch + (long long)n * a.gn + (long long)c0 * a.gc;
    const bool linear = a.gh == (long long)a.w * a.gw;  // the pixels of a channel are one strided run (NCHW and NHWC both)
    if (a.gc == 1) {  // channels innermost: lanes on the channels
        if (tc < cn)
            for (int p = tr; p < hw; p += AR_ROWS) slab[tc + pixel_offset(p, a.w, a.gh, a.gw, linear)] = 0.0f;
    } else {  // lanes on the pixels
        for (int c = 0; c < cn; ++c)
            for (int p = t; p < hw; p += AR_THREADS) slab[(long long)c * a.gc + pixel_offset(p, a.w, a.gh, a.gw, linear)] = 0.0f;
    }
    __syncthreads();  // (the zeros of this work-group are ordered before its own stores below; nobody else touches the slab)
    // ---- every touched pixel once: its chain's sum, front to back
    if (tc >= cn) return;
    const float* gc = g + a.D + c0 + tc;
    for (int r = tr; r < R; r += AR_ROWS) {
        if (!s_head[r]) continue;
        float acc = 0.0f;
        for (int q = r; q >= 0; q = s_next[q]) acc += gc[(long long)(q >> 2) * Dt] * s_wt[q];
        slab[(long long)tc * a.gc + pixel_offset(s_pix[r], a.w, a.gh, a.gw, linear)] = acc;
    }
}

__global__ __launch_bounds__(CA_THREADS) void constrain_angles_fwd_kernel(const float* __restrict__ x, const float* __restrict__ S, float m, int count,
                                                                          int K3, float* __restrict__ angles, float* __restrict__ reg) {
    __shared__ double red[CA_WAVES];
    __shared__ float s_S[3 * MAXK];
    if ((int)threadIdx.x < K3) s_S[threadIdx.x] = S[threadIdx.x];
    __syncthreads();
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += CA_THREADS) {
        const float th = (float)tanh((double)(x[i] * m));
        const float v = s_S[i % K3] * th;
        angles[i] = v;
        acc += (double)v * (double)v;
    }
    if (reg == nullptr) return;
    const double total = a3d_block_sum<CA_WAVES>(acc, red);
    if (threadIdx.x == 0) reg[0] = (float)(total / (double)count);
}

__global__ __launch_bounds__(CA_THREADS) void constrain_angles_bwd_kernel(const float* __restrict__ g_angles, const float* __restrict__ g_reg,
                                                                          const float* __restrict__ x, const float* __restrict__ S, float m, int count,
                                                                          int K3, float* __restrict__ g_x) {
    __shared__ float s_S[3 * MAXK];
    if ((int)threadIdx.x < K3) s_S[threadIdx.x] = S[threadIdx.x];
    __syncthreads();
    const double per_square = g_reg ? (double)g_reg[0] * 2.0 / (double)count : 0.0;
    for (int i = threadIdx.x; i < count; i += CA_THREADS) {
        const double th = (double)(float)tanh((double)(x[i] * m));  // the forward's float32 tanh: +-1 once saturated, the slope then exactly 0
        const float s = s_S[i % K3];
        const float v = s * (float)th;
        const double up = (g_angles ? (double)g_angles[i] : 0.0) + per_square * (double)v;
        g_x[i] = (float)(up * (double)s * (double)m * (1.0 - th * th));
    }
}

}  // namespace

#define AR_CHECK_SHAPE()                                                                                                   \
    A3D_CHECK_ARG(K >= 1 && K <= A3D_ARTICULATION_MAX_BONES && N >= 0 && D >= 0 && C >= 0);                                \
    A3D_CHECK_ARG(C == 0 || (h >= 1 && h <= A3D_ARTICULATION_MAX_SIDE && w >= 1 && w <= A3D_ARTICULATION_MAX_SIDE));       \
    A3D_CHECK_ARG((long long)N * K * ((long long)D + C) < (1ll << 31) && (long long)N * K * 9 < (1ll << 31));              \
    A3D_CHECK_ARG((long long)N * D < (1ll << 31) && (long long)N * C < (1ll << 31) && N <= A3D_ARTICULATION_MAX_IMAGES)

extern "C" int a3d_bone_inputs_fwd(const float* bones, int bones_shared, const float* mvp, const float* w2c, float cam_pos_z_offset,
                                   float spatial_scale, const float* feat, const float* patch, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int N,
                                   int K, int D, int C, int h, int w, float* bones_feat, float* pos_in, a3d_stream_t stream) {
    AR_CHECK_SHAPE();
    A3D_CHECK_ARG(C == 0 || (sn >= 0 && sc >= 0 && sh >= 0 && sw >= 0));
    if (N == 0) return A3D_OK;
    A3D_CHECK_ARG(bones && mvp && w2c && pos_in);
    A3D_CHECK_ARG((D == 0 || feat) && (C == 0 || patch) && (D + C == 0 || bones_feat));
    const int chunks = max(1, a3d_div_up(D, CH) + a3d_div_up(C, CH));
    FwdArgs a;
    a.bones = bones, a.mvp = mvp, a.w2c = w2c, a.feat = feat, a.patch = patch;
    a.z_offset = cam_pos_z_offset, a.spatial_scale = spatial_scale;
    a.sn = sn, a.sc = sc, a.sh = sh, a.sw = sw;
    a.bones_shared = bones_shared, a.K = K, a.D = D, a.C = C, a.h = h, a.w = w;
    a.bones_feat = bones_feat, a.pos_in = pos_in;
    hipLaunchKernelGGL(bone_inputs_fwd_kernel, dim3(chunks, N), dim3(AR_THREADS), 0, (hipStream_t)stream, a);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_bone_inputs_bwd(const float* g_bones_feat, const float* pos_in, int N, int K, int D, int C, int h, int w, float* g_feat,
                                   float* g_patch, int64_t gn, int64_t gc, int64_t gh, int64_t gw, a3d_stream_t stream) {
    AR_CHECK_SHAPE();
    A3D_CHECK_ARG(D + C > 0 && (long long)N * C * h * w < (1ll << 31));
    A3D_CHECK_ARG(g_patch == nullptr || (C > 0 && gn >= 1 && gc >= 1 && gh >= 1 && gw >= 1));
    A3D_CHECK_ARG(g_feat == nullptr || D > 0);
    if (N == 0) return A3D_OK;
    A3D_CHECK_ARG(g_bones_feat && pos_in && (g_feat || g_patch));
    BwdArgs a;
    a.g = g_bones_feat, a.pos_in = pos_in;
    a.K = K, a.D = D, a.C = C, a.h = h, a.w = w;
    a.chunks_d = g_feat ? a3d_div_up(D, CH) : 0;
    a.g_feat = g_feat, a.g_patch = g_patch;
    a.gn = gn, a.gc = gc, a.gh = gh, a.gw = gw;
    const int chunks = a.chunks_d + (g_patch ? a3d_div_up(C, CH) : 0);
    hipLaunchKernelGGL(bone_inputs_bwd_kernel, dim3(chunks, N), dim3(AR_THREADS), 0, (hipStream_t)stream, a);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

#define CA_CHECK_SHAPE() \
    A3D_CHECK_ARG(K >= 1 && K <= A3D_ARTICULATION_MAX_BONES && N >= 0 && (long long)N * K * 3 <= A3D_ARTICULATION_MAX_ANGLES)

extern "C" int a3d_constrain_angles_fwd(const float* x, const float* S, float multiplier, int N, int K, float* angles, float* reg,
                                        a3d_stream_t stream) {
    CA_CHECK_SHAPE();
    if (N == 0) return A3D_OK;
    A3D_CHECK_ARG(x && S && angles);
    hipLaunchKernelGGL(constrain_angles_fwd_kernel, dim3(1), dim3(CA_THREADS), 0, (hipStream_t)stream, x, S, multiplier, N * K * 3, K * 3, angles,
                       reg);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_constrain_angles_bwd(const float* g_angles, const float* g_reg, const float* x, const float* S, float multiplier, int N, int K,
                                        float* g_x, a3d_stream_t stream) {
    CA_CHECK_SHAPE();
    if (N == 0) return A3D_OK;
    A3D_CHECK_ARG(x && S && g_x && (g_angles || g_reg));
    hipLaunchKernelGGL(constrain_angles_bwd_kernel, dim3(1), dim3(CA_THREADS), 0, (hipStream_t)stream, g_angles, g_reg, x, S, multiplier, N * K * 3,
                       K * 3, g_x);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
