// Per-pixel arithmetic of the image-space derivatives (csrc/deriv.hip): rast_db = d(u, v) / d(X, Y) of the perspective-correct
// barycentrics of the stored triangle, and its adjoint w.r.t. the clip-space (x, y, w) of the three vertices.
//
// Forward, operation by operation what ops._rasterize_db_torch states (deriv.hip is compiled with -ffp-contract=off):
//   q_i = p_i.xy - f p_i.w,  a_i = q_j x q_k,  s = a_0 + a_1 + a_2          (j, k) = (i + 1, i + 2) mod 3
//   d a_i / d fx = -w_j qy_k + qy_j w_k,   d a_i / d fy = -qx_j w_k + w_j qx_k
//   du/dX = (d a_0/d fx * s - a_0 * d s/d fx) / (s * s) * (2 / W)   -- and likewise du/dY, dv/dX, dv/dY (a_1 for v, 2 / H for Y)
#pragma once

#define DV_HD __device__ __forceinline__

struct DvPixel {  // what both directions need of one pixel
    float qx[3], qy[3], w[3];
    float a[3], dax[3], day[3];
    float s, sx, sy;
};

// p[i] = (x, y, w) of vertex i; (fx, fy) = the pixel centre in NDC
DV_HD void dv_setup(const float (&px)[3], const float (&py)[3], const float (&pw)[3], float fx, float fy, DvPixel& d) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d.w[i] = pw[i];
        d.qx[i] = px[i] - fx * pw[i];
        d.qy[i] = py[i] - fy * pw[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        d.a[i] = d.qx[j] * d.qy[k] - d.qy[j] * d.qx[k];
        d.dax[i] = -d.w[j] * d.qy[k] + d.qy[j] * d.w[k];
        d.day[i] = -d.qx[j] * d.w[k] + d.w[j] * d.qx[k];
    }
    d.s = d.a[0] + d.a[1] + d.a[2];
    d.sx = d.dax[0] + d.dax[1] + d.dax[2];
    d.sy = d.day[0] + d.day[1] + d.day[2];
}

// (du/dX, du/dY, dv/dX, dv/dY); kx = 2 / W, ky = 2 / H.  d.s != 0.
DV_HD void dv_forward(const DvPixel& d, float kx, float ky, float (&out)[4]) {
    const float ss = d.s * d.s;
    out[0] = (d.dax[0] * d.s - d.a[0] * d.sx) / ss * kx;
    out[1] = (d.day[0] * d.s - d.a[0] * d.sy) / ss * ky;
    out[2] = (d.dax[1] * d.s - d.a[1] * d.sx) / ss * kx;
    out[3] = (d.day[1] * d.s - d.a[1] * d.sy) / ss * ky;
}

// Adjoint: g = d L / d (du/dX, du/dY, dv/dX, dv/dY) -> c[3 * i + (0, 1, 2)] = d L / d (x_i, y_i, w_i).  With h = g * (kx, ky, kx, ky)
// and L = N / s^2, N = h0 (dax0 s - a0 sx) + h1 (day0 s - a0 sy) + h2 (dax1 s - a1 sx) + h3 (day1 s - a1 sy):
//   dL/d dax0 = h0 / s, dL/d day0 = h1 / s, dL/d dax1 = h2 / s, dL/d day1 = h3 / s
//   dL/d sx = -(h0 a0 + h2 a1) / s^2,   dL/d sy = -(h1 a0 + h3 a1) / s^2        (sx, sy feed every dax_i, day_i)
//   dL/d a0 = -(h0 sx + h1 sy) / s^2,   dL/d a1 = -(h2 sx + h3 sy) / s^2
//   dL/d s  = (h0 dax0 + h1 day0 + h2 dax1 + h3 day1) / s^2 - 2 N / s^3           (s feeds every a_i)
// then the products a_i, dax_i, day_i back to (q, w), and q = p.xy - f p.w back to (x, y, w).  d.s != 0.
DV_HD void dv_backward(const DvPixel& d, float kx, float ky, float fx, float fy, const float (&g)[4], float (&c)[9]) {
    const float h0 = g[0] * kx, h1 = g[1] * ky, h2 = g[2] * kx, h3 = g[3] * ky;
    const float is = 1.f / d.s, is2 = is * is;
    const float n = h0 * (d.dax[0] * d.s - d.a[0] * d.sx) + h1 * (d.day[0] * d.s - d.a[0] * d.sy) + h2 * (d.dax[1] * d.s - d.a[1] * d.sx) +
                    h3 * (d.day[1] * d.s - d.a[1] * d.sy);
    const float gs = (h0 * d.dax[0] + h1 * d.day[0] + h2 * d.dax[1] + h3 * d.day[1]) * is2 - 2.f * n * is2 * is;
    const float gsx = -(h0 * d.a[0] + h2 * d.a[1]) * is2, gsy = -(h1 * d.a[0] + h3 * d.a[1]) * is2;
    const float ga[3] = {gs - (h0 * d.sx + h1 * d.sy) * is2, gs - (h2 * d.sx + h3 * d.sy) * is2, gs};
    const float gdx[3] = {gsx + h0 * is, gsx + h2 * is, gsx};
    const float gdy[3] = {gsy + h1 * is, gsy + h3 * is, gsy};
    float gqx[3] = {0.f, 0.f, 0.f}, gqy[3] = {0.f, 0.f, 0.f}, gw[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        // a_i = qx_j qy_k - qy_j qx_k
        gqx[j] += ga[i] * d.qy[k]; gqy[k] += ga[i] * d.qx[j];
        gqy[j] -= ga[i] * d.qx[k]; gqx[k] -= ga[i] * d.qy[j];
        // dax_i = -w_j qy_k + qy_j w_k
        gw[j] -= gdx[i] * d.qy[k]; gqy[k] -= gdx[i] * d.w[j];
        gqy[j] += gdx[i] * d.w[k]; gw[k] += gdx[i] * d.qy[j];
        // day_i = -qx_j w_k + w_j qx_k
        gqx[j] -= gdy[i] * d.w[k]; gw[k] -= gdy[i] * d.qx[j];
        gw[j] += gdy[i] * d.qx[k]; gqx[k] += gdy[i] * d.w[j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[3 * i] = gqx[i];
        c[3 * i + 1] = gqy[i];
        c[3 * i + 2] = gw[i] - fx * gqx[i] - fy * gqy[i];
    }
}
