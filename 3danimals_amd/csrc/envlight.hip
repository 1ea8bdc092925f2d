// Split-sum environment light on gfx950: the cube-map prefilters behind EnvironmentLight.build_mips (include/a3d.h "Environment light";
// the specification is written out in ops.py diffuse_cubemap() / specular_cubemap_raw()).
//
// One lane per output texel, forward and backward alike.  The backward is a GATHER: the pair weight is w(p, q) = f(p, q) * area(q) with f
// and the membership test symmetric in p and q, so g_in[q] = area(q) / 4 * sum over p in bounds(q) of g_out[p] * f(p, q) runs through the
// same bounds table and the same loop as the forward, writes every element once and is reproducible run to run -- no float atomics.
// Both passes build texel directions with env_dir() and dot them with env_dot() (a fixed fma chain whose products commute), so a pair is
// inside the cone in the backward exactly when it is in the forward.
// Specular: a wave is an 8 x 8 block of output texels (neighbouring lanes walk nearly the same windows: their loads share cache lines and
// their loops have nearly the same length); texel coordinates and the separable solid-angle factors (no atan in the loop) sit in LDS.
// Diffuse: every texel sees every texel (1536 x 1536 pairs at the size the light uses); the source map is staged through LDS in chunks as
// (direction, weight, colour) and read back by broadcast.
// Bounds: the exhaustive test, a row of source directions at a time through LDS -- a one-off per (N, cutoff), no culling to get wrong.
#include "a3d_common.h"

namespace {

constexpr int ENV_MAX_N = 4096;       // the specular filter keeps 2 N floats in LDS
constexpr int ENV_MAX_DIFFUSE_N = 256;  // the diffuse filter is all pairs (36 N^4): the light runs it at 16; 256 is 1.5e11 pairs, a fraction of a second
constexpr int ENV_MAX_BOUNDS_N = 32767;  // the table is int16
constexpr int ENV_DIFF_CHUNK = 1536;  // texels staged per round of the diffuse filter (7 floats each: 42 KiB)
constexpr int ENV_ROW_CHUNK = 1024;   // source texels of one row staged per round of the bounds search
constexpr float ENV_PI = 3.14159265358979323846f;

struct EnvK {
    int N;
    float a2, cutoff;
    const float* src;
    float* dst;
    int16_t* bounds;
    const float* area;
};

// centre of texel i on the -1..1 face axis
__device__ __forceinline__ float env_coord(int i, int N) { return (2.f * ((float)i + 0.5f)) / (float)N - 1.f; }

// unit direction of the texel centre (cx, cy) of a face: the reference's cube_to_dir (model/render/util.py:96-103), the convention
// texture.hip's cube_dir() inverts.  The squared length is summed in one order for every face.
__device__ __forceinline__ void env_dir(int face, float cx, float cy, float& x, float& y, float& z) {
    const float inv = rsqrtf(cx * cx + cy * cy + 1.f);
    const float u = cx * inv, v = cy * inv;
    switch (face) {
        case 0: x = inv; y = -v; z = -u; break;
        case 1: x = -inv; y = -v; z = u; break;
        case 2: x = u; y = inv; z = v; break;
        case 3: x = u; y = -inv; z = -v; break;
        case 4: x = u; y = -v; z = inv; break;
        default: x = -u; y = -v; z = -inv; break;
    }
}

// env_dot(a, b) == env_dot(b, a) bit for bit (every product commutes, the chain is fixed)
__device__ __forceinline__ float env_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(ax, bx, fmaf(ay, by, az * bz));
}

// face, x, y of texel i of a [6, N, N] map
__device__ __forceinline__ void env_texel(long long i, int N, int& face, int& x, int& y) {
    x = (int)(i % N);
    const long long r = i / N;
    y = (int)(r % N);
    face = (int)(r / N);
}

// ---- diffuse: out[p] = sum_q in[q] * clamp(dot, 0, 0.999) * area(q) / pi; backward: g_in[q] = area(q) / pi * sum_p g_out[p] * clamp(dot)
template <bool BWD>
__global__ __launch_bounds__(64) void env_diffuse_kernel(const EnvK k) {
    __shared__ float sd[ENV_DIFF_CHUNK * 3], sv[ENV_DIFF_CHUNK * 3], sw[ENV_DIFF_CHUNK];
    const int N = k.N, total = 6 * N * N;
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool valid = i < total;
    int face, px, py;
    env_texel(valid ? i : 0, N, face, px, py);
    float dx, dy, dz;
    env_dir(face, env_coord(px, N), env_coord(py, N), dx, dy, dz);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int base = 0; base < total; base += ENV_DIFF_CHUNK) {
        const int n = min(ENV_DIFF_CHUNK, total - base);
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += 64) {
            int f, x, y;
            env_texel(base + j, N, f, x, y);
            env_dir(f, env_coord(x, N), env_coord(y, N), sd[3 * j], sd[3 * j + 1], sd[3 * j + 2]);
            sw[j] = BWD ? 1.f : k.area[x] * k.area[y];
            const float* s = k.src + (long long)(base + j) * 3;
            sv[3 * j] = s[0]; sv[3 * j + 1] = s[1]; sv[3 * j + 2] = s[2];
        }
        __syncthreads();
        if (valid) {
            for (int j = 0; j < n; ++j) {
                const float d = env_dot(sd[3 * j], sd[3 * j + 1], sd[3 * j + 2], dx, dy, dz);
                const float w = fminf(fmaxf(d, 0.f), 0.999f) * sw[j];
                a0 = fmaf(w, sv[3 * j], a0);
                a1 = fmaf(w, sv[3 * j + 1], a1);
                a2 = fmaf(w, sv[3 * j + 2], a2);
            }
        }
    }
    if (!valid) return;
    const float scale = BWD ? k.area[px] * k.area[py] : 1.f;
    float* o = k.dst + (long long)i * 3;
    o[0] = a0 * scale / ENV_PI;
    o[1] = a1 * scale / ENV_PI;
    o[2] = a2 * scale / ENV_PI;
}

// ---- bounds: for (output texel p, source face s) the rectangle of the texels q of s with dot(d_q, d_p) >= cutoff; empty = (N-1, 0, N-1, 0)
__global__ __launch_bounds__(256) void env_bounds_kernel(const EnvK k) {
    __shared__ float4 row[ENV_ROW_CHUNK];
    const int N = k.N, s = blockIdx.y;
    const long long total = 6ll * N * N, i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < total;
    int face, px, py;
    env_texel(valid ? i : 0, N, face, px, py);
    float dx, dy, dz;
    env_dir(face, env_coord(px, N), env_coord(py, N), dx, dy, dz);
    int xmin = N - 1, xmax = 0, ymin = N - 1, ymax = 0;
    for (int y = 0; y < N; ++y) {
        const float cy = env_coord(y, N);
        for (int xb = 0; xb < N; xb += ENV_ROW_CHUNK) {
            const int n = min(ENV_ROW_CHUNK, N - xb);
            __syncthreads();
            for (int j = threadIdx.x; j < n; j += 256) {
                float4 q;
                env_dir(s, env_coord(xb + j, N), cy, q.x, q.y, q.z);
                q.w = 0.f;
                row[j] = q;
            }
            __syncthreads();
            for (int j = 0; j < n; ++j) {
                const float4 q = row[j];
                if (env_dot(q.x, q.y, q.z, dx, dy, dz) >= k.cutoff) {
                    xmin = min(xmin, xb + j);
                    xmax = max(xmax, xb + j);
                    ymin = min(ymin, y);
                    ymax = max(ymax, y);
                }
            }
        }
    }
    if (!valid) return;
    int16_t* b = k.bounds + (i * 6 + s) * 4;
    b[0] = (int16_t)xmin; b[1] = (int16_t)xmax; b[2] = (int16_t)ymin; b[3] = (int16_t)ymax;
}

// ---- specular.  Forward: out[p] = (sum_q w in[q], sum_q w) over the q inside the cone, w = max(dot, 0) * D * area(q) / 4,
// D = a2 / (pi ((t a2 - t) t + 1)^2), t = clamp(dot(d_p, h), 0, 1), h = normalize(d_q + d_p).
// Backward (the lane is q, the loop runs over p): g_in[q] = area(q) / 4 * sum_p g_out[p][0:3] * max(dot, 0) * D, the same D: t is taken
// with the LOOP texel's direction there, which is the forward's d_p.
template <bool BWD>
__global__ __launch_bounds__(64) void env_specular_kernel(const EnvK k) {
    extern __shared__ float lds[];
    const int N = k.N;
    float* coord = lds;
    float* area = lds + N;
    for (int j = threadIdx.x; j < N; j += 64) {
        coord[j] = env_coord(j, N);
        area[j] = k.area[j];
    }
    __syncthreads();
    const int lane = threadIdx.x;
    int face, px, py;
    bool valid;
    if (N >= 8) {
        const int tiles = (N + 7) / 8;
        const int t = blockIdx.x % (tiles * tiles);
        face = blockIdx.x / (tiles * tiles);
        px = (t % tiles) * 8 + (lane & 7);
        py = (t / tiles) * 8 + (lane >> 3);
        valid = px < N && py < N;
    } else {
        const int i = blockIdx.x * 64 + lane;
        valid = i < 6 * N * N;
        env_texel(valid ? i : 0, N, face, px, py);
    }
    if (!valid) return;
    float dx, dy, dz;
    env_dir(face, coord[px], coord[py], dx, dy, dz);
    const long long p = ((long long)face * N + py) * N + px;
    const int16_t* b = k.bounds + p * 24;
    constexpr int CH = BWD ? 4 : 3;  // floats per texel of src: g_out [.,4] / the map [.,3]
    const float a2 = k.a2;
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, ws = 0.f;
    for (int s = 0; s < 6; ++s) {
        // (clamped into the face: whatever table the caller hands in, nothing outside the map is read)
        const int xmin = max((int)b[4 * s], 0), xmax = min((int)b[4 * s + 1], N - 1);
        const int ymin = max((int)b[4 * s + 2], 0), ymax = min((int)b[4 * s + 3], N - 1);
        for (int y = ymin; y <= ymax; ++y) {
            const float cy = coord[y], ay = area[y];
            const float* srow = k.src + (((long long)s * N + y) * N) * CH;
            for (int x = xmin; x <= xmax; ++x) {
                float qx, qy, qz;
                env_dir(s, coord[x], cy, qx, qy, qz);
                const float d = env_dot(qx, qy, qz, dx, dy, dz);
                if (!(d >= k.cutoff) || !(d > 0.f)) continue;  // (d <= 0: weight 0, and h may be the zero vector)
                float hx = qx + dx, hy = qy + dy, hz = qz + dz;
                const float hinv = rsqrtf(hx * hx + hy * hy + hz * hz);
                hx *= hinv; hy *= hinv; hz *= hinv;
                float t = BWD ? env_dot(qx, qy, qz, hx, hy, hz) : env_dot(dx, dy, dz, hx, hy, hz);
                t = fminf(fmaxf(t, 0.f), 1.f);
                const float den = (t * a2 - t) * t + 1.f;
                const float D = a2 / (ENV_PI * den * den);
                const float w = BWD ? d * D : d * D * (area[x] * ay) * 0.25f;
                const float* v = srow + (long long)x * CH;
                c0 = fmaf(w, v[0], c0);
                c1 = fmaf(w, v[1], c1);
                c2 = fmaf(w, v[2], c2);
                ws += w;
            }
        }
    }
    if (BWD) {
        const float scale = area[px] * area[py] * 0.25f;
        float* o = k.dst + p * 3;
        o[0] = c0 * scale; o[1] = c1 * scale; o[2] = c2 * scale;
    } else {
        float* o = k.dst + p * 4;
        o[0] = c0; o[1] = c1; o[2] = c2; o[3] = ws;
    }
}

int env_check(const a3d_env_desc* d, EnvK& k, const char* fn, int max_n) {
    if (!d) {
        a3d_set_error("%s: invalid argument: desc", fn);
        return A3D_EINVAL;
    }
    if (d->size < sizeof(a3d_env_desc)) {  // (before any other field is read: a shorter struct does not have them)
        a3d_set_error("%s: invalid argument: desc->size %u < sizeof(a3d_env_desc) %zu (a caller built against an older header)", fn, d->size,
                      sizeof(a3d_env_desc));
        return A3D_EINVAL;
    }
    if (d->N < 1 || d->N > max_n) {
        a3d_set_error("%s: invalid argument: N = %d, must be 1 .. %d", fn, d->N, max_n);
        return A3D_EINVAL;
    }
    k.N = d->N;
    k.a2 = d->roughness * d->roughness * d->roughness * d->roughness;
    k.cutoff = d->costheta_cutoff;
    k.src = d->src;
    k.dst = d->dst;
    k.bounds = d->bounds;
    k.area = d->area;
    return A3D_OK;
}

template <bool BWD>
int env_diffuse(const a3d_env_desc* desc, a3d_stream_t stream, const char* fn) {
    EnvK k;
    const int rc = env_check(desc, k, fn, ENV_MAX_DIFFUSE_N);
    if (rc) return rc;
    if (!(k.src && k.dst && k.area)) {
        a3d_set_error("%s: invalid argument: src, dst and area must be set", fn);
        return A3D_EINVAL;
    }
    hipLaunchKernelGGL(env_diffuse_kernel<BWD>, dim3(a3d_div_up(6ll * k.N * k.N, 64)), dim3(64), 0, (hipStream_t)stream, k);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

template <bool BWD>
int env_specular(const a3d_env_desc* desc, a3d_stream_t stream, const char* fn) {
    EnvK k;
    const int rc = env_check(desc, k, fn, ENV_MAX_N);
    if (rc) return rc;
    if (!(k.src && k.dst && k.area && k.bounds) || !(desc->roughness > 0.f) || !(desc->costheta_cutoff >= -1.f && desc->costheta_cutoff <= 1.f)) {
        a3d_set_error("%s: invalid argument: src, dst, area and bounds must be set, roughness > 0, -1 <= costheta_cutoff <= 1", fn);
        return A3D_EINVAL;
    }
    const int N = k.N, tiles = (N + 7) / 8;
    const int waves = N >= 8 ? 6 * tiles * tiles : a3d_div_up(6ll * N * N, 64);
    hipLaunchKernelGGL(env_specular_kernel<BWD>, dim3(waves), dim3(64), 2 * N * sizeof(float), (hipStream_t)stream, k);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

}  // namespace

extern "C" int a3d_cubemap_diffuse_fwd(const a3d_env_desc* desc, a3d_stream_t stream) { return env_diffuse<false>(desc, stream, __func__); }
extern "C" int a3d_cubemap_diffuse_bwd(const a3d_env_desc* desc, a3d_stream_t stream) { return env_diffuse<true>(desc, stream, __func__); }
extern "C" int a3d_cubemap_specular_fwd(const a3d_env_desc* desc, a3d_stream_t stream) { return env_specular<false>(desc, stream, __func__); }
extern "C" int a3d_cubemap_specular_bwd(const a3d_env_desc* desc, a3d_stream_t stream) { return env_specular<true>(desc, stream, __func__); }

extern "C" int a3d_cubemap_specular_bounds(const a3d_env_desc* desc, a3d_stream_t stream) {
    EnvK k;
    const int rc = env_check(desc, k, __func__, ENV_MAX_BOUNDS_N);
    if (rc) return rc;
    A3D_CHECK_ARG(desc->bounds);
    A3D_CHECK_ARG(desc->costheta_cutoff >= -1.f && desc->costheta_cutoff <= 1.f);
    hipLaunchKernelGGL(env_bounds_kernel, dim3(a3d_div_up(6ll * k.N * k.N, 256), 6), dim3(256), 0, (hipStream_t)stream, k);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
