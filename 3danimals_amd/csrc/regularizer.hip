// The mesh regularisers on gfx950 (include/a3d_reg.h): laplace_regularizer_const, normal_consistency and avg_edge_length of the
// reference's model/render/regularizer.py, and the per-occurrence edge table they stand on (compute_edges /
// compute_edge_to_face_mapping, reference mesh.py:196-250, without torch.unique's sort and read-back).
//
// Everything is a gather, the idiom of normals.hip and tangent.hip over the same vertex -> (corner, face) lists: no atomics on floats.
// A unique edge is owned by one of its directed occurrences (its representative: the highest slot of the key), found by scanning the
// list of the key's lower vertex, which holds every face at the edge.  The losses are scalars: per-element terms and all sums are
// doubles, a work-group adds its 256 terms in a fixed tree and writes one partial, a finishing launch adds the partials in a fixed
// order and rounds once.  Per-vertex sums visit a list in ascending key order, so they do not depend on the order it was filled in.
#include "../../include/a3d_reg.h"
#include "a3d_common.h"
#include "topo_common.h"

namespace {

constexpr int RG_THREADS = 256;

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator*(D3 a, double s) { return D3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ D3 load3(const float* __restrict__ p, int i) { return D3{p[3ll * i], p[3ll * i + 1], p[3ll * i + 2]}; }
__device__ __forceinline__ D3 load3(const double* __restrict__ p, int i) { return D3{p[3ll * i], p[3ll * i + 1], p[3ll * i + 2]}; }

__device__ __forceinline__ void key_split(int key, int F, int& c, int& f) {
    c = key >= 2 * F ? 2 : (key >= F ? 1 : 0);
    f = key - c * F;
}

// fn(key) for every entry of a list in ascending key order, whatever order it is stored in: up to eight keys are sorted in registers,
// a longer list is re-read from memory for every entry
template <typename Fn>
__device__ __forceinline__ void rg_each_key(const int* __restrict__ adj, int lo, int cnt, Fn fn) {
    if (cnt <= 0) return;
    if (cnt <= 8) {
        int keys[8];
        nr_load_keys(adj, lo, cnt, keys);
        a3d_sort8(keys);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < cnt) fn(keys[e]);
        return;
    }
    int last = -1;
    for (int e = 0; e < cnt; ++e) {
        last = nr_next_key_mem(adj, lo, cnt, last);
        fn(last);
    }
}

// sum of v over the work-group in a fixed tree (every thread of the group calls this); sh: RG_THREADS doubles
__device__ __forceinline__ double rg_block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = RG_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// safe_normalize(cross(v1 - v0, v2 - v0)) of face f (render/util.py:28-32), with what its adjoint needs
struct FaceNormal {
    D3 n, e1, e2;
    double len, d;
};
__device__ __forceinline__ FaceNormal face_normal(const float* __restrict__ vp, const int* __restrict__ tri, int f) {
    FaceNormal r;
    const D3 p0 = load3(vp, tri[3 * f]);
    r.e1 = load3(vp, tri[3 * f + 1]) - p0;
    r.e2 = load3(vp, tri[3 * f + 2]) - p0;
    const D3 c = cross(r.e1, r.e2);
    r.d = dot(c, c);
    r.len = sqrt(r.d < 1e-20 ? 1e-20 : r.d);
    r.n = D3{c.x / r.len, c.y / r.len, c.z / r.len};
    return r;
}

// t = (1 - clamp(d, -1, 1)) 0.5 receives a gradient through |t| and the clamp: autograd's rule (clamp passes on [-1, 1] inclusive, abs gives 0 at 0)
__device__ __forceinline__ bool nc_live(double d) { return d >= -1.0 && d <= 1.0 && (1.0 - d) * 0.5 != 0.0; }

// ---------------------------------------------------------------------------------------------- edge table
__global__ __launch_bounds__(RG_THREADS) void edge_topology_kernel(const int* __restrict__ tri, int F, const int* __restrict__ off,
                                                                   const int* __restrict__ adj, int stride, int* __restrict__ table,
                                                                   int* __restrict__ num_edges) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    bool rep = false;
    if (s < 3 * F) {
        const int f = s / 3, c = s - 3 * f;
        const int i = tri[3 * f + c], j = tri[3 * f + (c + 1) % 3];
        const int lo = min(i, j), hi = max(i, j);
        int max_f = -1, max_b = -1;  // the highest forward / backward slot of the key
        int l0, n;
        vf_list(off, stride, lo, l0, n);
        for (int e = 0; e < n; ++e) {
            int cc, g;
            key_split(adj[l0 + e], F, cc, g);  // lo sits at corner cc of face g
            const int next = tri[3 * g + (cc + 1) % 3], prev = tri[3 * g + (cc + 2) % 3];
            if (next == hi) max_f = max(max_f, 3 * g + cc);  // runs lo -> hi: forward
            if (prev == hi) {  // runs hi -> lo: backward, unless it is a self edge
                const int slot = 3 * g + (cc + 2) % 3;
                if (hi > lo) max_b = max(max_b, slot);
                else max_f = max(max_f, slot);
            }
        }
        const bool fwd = i <= j;
        rep = s == max(max_f, max_b);
        const bool winner = s == (fwd ? max_f : max_b);
        const int other = fwd ? max_b : max_f;
        table[2ll * s] = (rep ? A3D_EDGE_REPRESENTATIVE : 0) | (winner ? A3D_EDGE_WINNER : 0) | (other < 0 ? A3D_EDGE_STAND_IN : 0);
        table[2ll * s + 1] = other < 0 ? 0 : other / 3;
    }
    const unsigned long long reps = __ballot(rep);
    if (a3d_lane_id() == 0 && reps) atomicAdd(num_edges, (int)__popcll(reps));  // (an integer count)
}

// ---------------------------------------------------------------------------------------------- forward: terms and partials
// one thread per (image, vertex): the umbrella term, its square to the group's partial, term / max(2 n, 1) kept for the backward
__global__ __launch_bounds__(RG_THREADS) void laplace_fwd_kernel(const float* __restrict__ v_pos, const int* __restrict__ tri,
                                                                 const int* __restrict__ off, const int* __restrict__ adj, int stride, int V, int F,
                                                                 double* __restrict__ scaled, double* __restrict__ partials) {
    __shared__ double sh[RG_THREADS];
    const int vi = blockIdx.x * blockDim.x + threadIdx.x;
    const long long b = blockIdx.y;
    double q = 0.0;
    if (vi < V) {
        const float* vp = v_pos + b * V * 3;
        int lo, cnt;
        vf_list(off, stride, vi, lo, cnt);
        const D3 p = load3(vp, vi);
        D3 s{0.0, 0.0, 0.0};
        rg_each_key(adj, lo, cnt, [&](int key) {
            int c, f;
            key_split(key, F, c, f);
            s = s + ((load3(vp, tri[3 * f + (c + 1) % 3]) - p) + (load3(vp, tri[3 * f + (c + 2) % 3]) - p));
        });
        const double nrm = cnt > 0 ? 2.0 * cnt : 1.0;
        const D3 t{s.x / nrm, s.y / nrm, s.z / nrm};
        q = t.x * t.x + t.y * t.y + t.z * t.z;
        double* o = scaled + (b * V + vi) * 3;
        o[0] = t.x / nrm; o[1] = t.y / nrm; o[2] = t.z / nrm;
    }
    const double tot = rg_block_sum(q, sh);
    if (threadIdx.x == 0) partials[b * gridDim.x + blockIdx.x] = tot;
}

// one thread per (image, occurrence); the representatives contribute.  NC: |t| and the stand-in sum (4 doubles per partial row);
// otherwise the edge's length (1 double per row)
template <bool NC>
__global__ __launch_bounds__(RG_THREADS) void edge_fwd_kernel(const float* __restrict__ v_pos, const int* __restrict__ tri,
                                                              const int* __restrict__ table, int V, int F, double* __restrict__ partials) {
    __shared__ double sh[RG_THREADS];
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const long long b = blockIdx.y;
    const float* vp = v_pos + b * V * 3;
    double q = 0.0;
    D3 w{0.0, 0.0, 0.0};
    if (s < 3 * F) {
        const int flags = table[2ll * s];
        if (flags & A3D_EDGE_REPRESENTATIVE) {
            const int f = s / 3, c = s - 3 * f;
            if (NC) {
                const D3 n = face_normal(vp, tri, f).n, m = face_normal(vp, tri, table[2ll * s + 1]).n;
                const double d = dot(n, m);
                const double cl = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d);
                q = fabs((1.0 - cl) * 0.5);
                if ((flags & A3D_EDGE_STAND_IN) && nc_live(d)) w = n;
            } else {
                const D3 e = load3(vp, tri[3 * f + c]) - load3(vp, tri[3 * f + (c + 1) % 3]);
                const double d = dot(e, e);
                q = sqrt(d < 1e-20 ? 1e-20 : d);
            }
        }
    }
    const long long row = b * gridDim.x + blockIdx.x;
    const double tot = rg_block_sum(q, sh);
    if (NC) {
        const double wx = rg_block_sum(w.x, sh), wy = rg_block_sum(w.y, sh), wz = rg_block_sum(w.z, sh);
        if (threadIdx.x == 0) { partials[4 * row] = tot; partials[4 * row + 1] = wx; partials[4 * row + 2] = wy; partials[4 * row + 3] = wz; }
    } else if (threadIdx.x == 0) partials[row] = tot;
}

// work-group 0: loss = sum of column 0 of all B * per_image rows / (count * num_edges[0]).  Work-group 1 + b (CH = 4 only): the
// stand-in sum of image b.  Each thread adds a strided share in ascending order, the group adds the shares in a fixed tree.
template <int CH>
__global__ __launch_bounds__(RG_THREADS) void finish_kernel(const double* __restrict__ partials, int per_image, int B, double count,
                                                            const int* __restrict__ num_edges, float* __restrict__ loss,
                                                            double* __restrict__ stand_in) {
    __shared__ double sh[RG_THREADS];
    if (blockIdx.x == 0) {
        const long long rows = (long long)B * per_image;
        double a = 0.0;
        for (long long r = threadIdx.x; r < rows; r += RG_THREADS) a += partials[CH * r];
        const double tot = rg_block_sum(a, sh);
        if (threadIdx.x == 0) loss[0] = (float)(tot / (count * (num_edges ? (double)num_edges[0] : 1.0)));
        return;
    }
    if (CH == 4) {
        const long long b = blockIdx.x - 1;
        for (int k = 0; k < 3; ++k) {
            double a = 0.0;
            for (int r = threadIdx.x; r < per_image; r += RG_THREADS) a += partials[CH * (b * per_image + r) + 1 + k];
            const double tot = rg_block_sum(a, sh);
            if (threadIdx.x == 0) stand_in[3 * b + k] = tot;
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(RG_THREADS) void laplace_bwd_kernel(const float* __restrict__ g_loss, const double* __restrict__ scaled,
                                                                 const int* __restrict__ tri, const int* __restrict__ off,
                                                                 const int* __restrict__ adj, int stride, int B, int V, int F,
                                                                 float* __restrict__ g_v) {
    const int vi = blockIdx.x * blockDim.x + threadIdx.x;
    if (vi >= V) return;
    const long long b = blockIdx.y;
    const double* sc = scaled + b * V * 3;
    int lo, cnt;
    vf_list(off, stride, vi, lo, cnt);
    D3 a = load3(sc, vi) * (-2.0 * cnt);
    rg_each_key(adj, lo, cnt, [&](int key) {
        int c, f;
        key_split(key, F, c, f);
        a = a + (load3(sc, tri[3 * f + (c + 1) % 3]) + load3(sc, tri[3 * f + (c + 2) % 3]));
    });
    const double k = 2.0 * (double)g_loss[0] / (3.0 * B * V);
    float* o = g_v + (b * V + vi) * 3;
    o[0] = (float)(a.x * k); o[1] = (float)(a.y * k); o[2] = (float)(a.z * k);
}

// one thread per (image, face): the adjoint of its normal from its winning occurrences (+ the stand-in sum for face 0), through the
// normalisation and the cross product -> the three corners' rows
__global__ __launch_bounds__(RG_THREADS) void nc_faces_bwd_kernel(const float* __restrict__ g_loss, const float* __restrict__ v_pos,
                                                                  const int* __restrict__ tri, const int* __restrict__ table,
                                                                  const int* __restrict__ num_edges, const double* __restrict__ stand_in, int B,
                                                                  int V, int F, double* __restrict__ face_scratch) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const long long b = blockIdx.y;
    const float* vp = v_pos + b * V * 3;
    const FaceNormal me = face_normal(vp, tri, f);
    D3 gn{0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long s = 3ll * f + c;
        if (table[2 * s] & A3D_EDGE_WINNER) {
            const D3 m = face_normal(vp, tri, table[2 * s + 1]).n;
            if (nc_live(dot(me.n, m))) gn = gn + m;
        }
    }
    if (f == 0) gn = gn + load3(stand_in, (int)b);
    gn = gn * (-0.5 * (double)g_loss[0] / ((double)B * (double)num_edges[0]));
    // n = c / len, len = sqrt(max(c . c, 1e-20)): the clamp passes the gradient where c . c >= 1e-20
    D3 gc{gn.x / me.len, gn.y / me.len, gn.z / me.len};
    if (me.d >= 1e-20) gc = gc - me.n * (dot(me.n, gn) / me.len);
    const D3 g1 = cross(me.e2, gc), g2 = cross(gc, me.e1);  // c = e1 x e2
    double* o = face_scratch + (b * F + f) * 9;
    o[0] = -(g1.x + g2.x); o[1] = -(g1.y + g2.y); o[2] = -(g1.z + g2.z);
    o[3] = g1.x; o[4] = g1.y; o[5] = g1.z;
    o[6] = g2.x; o[7] = g2.y; o[8] = g2.z;
}

__global__ __launch_bounds__(RG_THREADS) void nc_gather_bwd_kernel(const double* __restrict__ face_scratch, const int* __restrict__ off,
                                                                   const int* __restrict__ adj, int stride, int V, int F,
                                                                   float* __restrict__ g_v) {
    const int vi = blockIdx.x * blockDim.x + threadIdx.x;
    if (vi >= V) return;
    const long long b = blockIdx.y;
    int lo, cnt;
    vf_list(off, stride, vi, lo, cnt);
    D3 a{0.0, 0.0, 0.0};
    rg_each_key(adj, lo, cnt, [&](int key) {
        int c, f;
        key_split(key, F, c, f);
        const double* r = face_scratch + (b * F + f) * 9 + 3 * c;
        a = a + D3{r[0], r[1], r[2]};
    });
    float* o = g_v + (b * V + vi) * 3;
    o[0] = (float)a.x; o[1] = (float)a.y; o[2] = (float)a.z;
}

// one thread per (image, vertex): the two occurrences at each corner entry, (v -> next) and (prev -> v), where they represent their edge
__global__ __launch_bounds__(RG_THREADS) void edge_length_bwd_kernel(const float* __restrict__ g_loss, const float* __restrict__ v_pos,
                                                                     const int* __restrict__ tri, const int* __restrict__ table,
                                                                     const int* __restrict__ num_edges, const int* __restrict__ off,
                                                                     const int* __restrict__ adj, int stride, int B, int V, int F,
                                                                     float* __restrict__ g_v) {
    const int vi = blockIdx.x * blockDim.x + threadIdx.x;
    if (vi >= V) return;
    const long long b = blockIdx.y;
    const float* vp = v_pos + b * V * 3;
    int lo, cnt;
    vf_list(off, stride, vi, lo, cnt);
    const D3 p = load3(vp, vi);
    D3 a{0.0, 0.0, 0.0};
    auto add = [&](int slot, int other) {
        if (!(table[2ll * slot] & A3D_EDGE_REPRESENTATIVE)) return;
        const D3 e = p - load3(vp, other);
        const double d = dot(e, e);
        if (d >= 1e-20) {  // sqrt(max(d, 1e-20)): the clamp passes the gradient from 1e-20 on
            const double len = sqrt(d);
            a = a + D3{e.x / len, e.y / len, e.z / len};
        }
    };
    rg_each_key(adj, lo, cnt, [&](int key) {
        int c, f;
        key_split(key, F, c, f);
        add(3 * f + c, tri[3 * f + (c + 1) % 3]);
        add(3 * f + (c + 2) % 3, tri[3 * f + (c + 2) % 3]);
    });
    const double k = (double)g_loss[0] / ((double)B * (double)num_edges[0]);
    float* o = g_v + (b * V + vi) * 3;
    o[0] = (float)(a.x * k); o[1] = (float)(a.y * k); o[2] = (float)(a.z * k);
}

}  // namespace

#define RG_CHECK_SIZES() A3D_CHECK_ARG(B > 0 && B <= 65535 && V > 0 && F > 0 && (long long)3 * F < 0x7fffffffll)

extern "C" size_t a3d_reg_partials(int B, int n) {
    if (B <= 0 || n <= 0) return 0;
    return (size_t)4 * (size_t)B * (size_t)a3d_div_up(3ll * n, RG_THREADS);
}

extern "C" int a3d_edge_topology(const int32_t* t_pos_idx, int F, int V, const int32_t* off, const int32_t* adj, int lists_stride,
                                 int32_t* edge_table, int32_t* num_edges, a3d_stream_t stream) {
    A3D_CHECK_ARG(V > 0 && F > 0 && (long long)3 * F < 0x7fffffffll && lists_stride >= 0);
    A3D_CHECK_ARG(t_pos_idx && off && adj && edge_table && num_edges);
    hipStream_t s = (hipStream_t)stream;
    A3D_HIP(hipMemsetAsync(num_edges, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(edge_topology_kernel, dim3(a3d_div_up(3ll * F, RG_THREADS)), dim3(RG_THREADS), 0, s, t_pos_idx, F, off, adj, lists_stride,
                       edge_table, num_edges);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_laplace_fwd(const float* v_pos, const int32_t* t_pos_idx, const int32_t* off, const int32_t* adj, int lists_stride, int B,
                               int V, int F, double* scaled, double* partials, float* loss, a3d_stream_t stream) {
    RG_CHECK_SIZES();
    A3D_CHECK_ARG(lists_stride >= 0 && v_pos && t_pos_idx && off && adj && scaled && partials && loss);
    hipStream_t s = (hipStream_t)stream;
    const int gx = a3d_div_up(V, RG_THREADS);
    hipLaunchKernelGGL(laplace_fwd_kernel, dim3(gx, B), dim3(RG_THREADS), 0, s, v_pos, t_pos_idx, off, adj, lists_stride, V, F, scaled, partials);
    A3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(finish_kernel<1>, dim3(1), dim3(RG_THREADS), 0, s, (const double*)partials, gx, B, 3.0 * B * V, (const int*)nullptr, loss,
                       (double*)nullptr);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_laplace_bwd(const float* g_loss, const double* scaled, const int32_t* t_pos_idx, const int32_t* off, const int32_t* adj,
                               int lists_stride, int B, int V, int F, float* g_v_pos, a3d_stream_t stream) {
    RG_CHECK_SIZES();
    A3D_CHECK_ARG(lists_stride >= 0 && g_loss && scaled && t_pos_idx && off && adj && g_v_pos);
    hipLaunchKernelGGL(laplace_bwd_kernel, dim3(a3d_div_up(V, RG_THREADS), B), dim3(RG_THREADS), 0, (hipStream_t)stream, g_loss, scaled, t_pos_idx,
                       off, adj, lists_stride, B, V, F, g_v_pos);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_normal_consistency_fwd(const float* v_pos, const int32_t* t_pos_idx, const int32_t* edge_table, const int32_t* num_edges,
                                          int B, int V, int F, double* stand_in, double* partials, float* loss, a3d_stream_t stream) {
    RG_CHECK_SIZES();
    A3D_CHECK_ARG(v_pos && t_pos_idx && edge_table && num_edges && stand_in && partials && loss);
    hipStream_t s = (hipStream_t)stream;
    const int gx = a3d_div_up(3ll * F, RG_THREADS);
    hipLaunchKernelGGL(edge_fwd_kernel<true>, dim3(gx, B), dim3(RG_THREADS), 0, s, v_pos, t_pos_idx, edge_table, V, F, partials);
    A3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(finish_kernel<4>, dim3(1 + B), dim3(RG_THREADS), 0, s, (const double*)partials, gx, B, (double)B, num_edges, loss, stand_in);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_normal_consistency_bwd(const float* g_loss, const float* v_pos, const int32_t* t_pos_idx, const int32_t* edge_table,
                                          const int32_t* num_edges, const int32_t* off, const int32_t* adj, int lists_stride,
                                          const double* stand_in, int B, int V, int F, double* face_scratch, float* g_v_pos,
                                          a3d_stream_t stream) {
    RG_CHECK_SIZES();
    A3D_CHECK_ARG(lists_stride >= 0 && g_loss && v_pos && t_pos_idx && edge_table && num_edges && off && adj && stand_in && face_scratch && g_v_pos);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nc_faces_bwd_kernel, dim3(a3d_div_up(F, RG_THREADS), B), dim3(RG_THREADS), 0, s, g_loss, v_pos, t_pos_idx, edge_table,
                       num_edges, stand_in, B, V, F, face_scratch);
    A3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(nc_gather_bwd_kernel, dim3(a3d_div_up(V, RG_THREADS), B), dim3(RG_THREADS), 0, s, (const double*)face_scratch, off, adj,
                       lists_stride, V, F, g_v_pos);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_edge_length_fwd(const float* v_pos, const int32_t* t_pos_idx, const int32_t* edge_table, const int32_t* num_edges, int B,
                                   int V, int F, double* partials, float* loss, a3d_stream_t stream) {
    RG_CHECK_SIZES();
    A3D_CHECK_ARG(v_pos && t_pos_idx && edge_table && num_edges && partials && loss);
    hipStream_t s = (hipStream_t)stream;
    const int gx = a3d_div_up(3ll * F, RG_THREADS);
    hipLaunchKernelGGL(edge_fwd_kernel<false>, dim3(gx, B), dim3(RG_THREADS), 0, s, v_pos, t_pos_idx, edge_table, V, F, partials);
    A3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(finish_kernel<1>, dim3(1), dim3(RG_THREADS), 0, s, (const double*)partials, gx, B, (double)B, num_edges, loss,
                       (double*)nullptr);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}

extern "C" int a3d_edge_length_bwd(const float* g_loss, const float* v_pos, const int32_t* t_pos_idx, const int32_t* edge_table,
                                   const int32_t* num_edges, const int32_t* off, const int32_t* adj, int lists_stride, int B, int V, int F,
                                   float* g_v_pos, a3d_stream_t stream) {
    RG_CHECK_SIZES();
    A3D_CHECK_ARG(lists_stride >= 0 && g_loss && v_pos && t_pos_idx && edge_table && num_edges && off && adj && g_v_pos);
    hipLaunchKernelGGL(edge_length_bwd_kernel, dim3(a3d_div_up(V, RG_THREADS), B), dim3(RG_THREADS), 0, (hipStream_t)stream, g_loss, v_pos,
                       t_pos_idx, edge_table, num_edges, off, adj, lists_stride, B, V, F, g_v_pos);
    A3D_LAUNCH_CHECK();
    return A3D_OK;
}
