// Per-pixel arithmetic of the shading BSDFs and the HDR image loss (reference renderutils/bsdf.py:57-151, loss.py:16-41), forward and
// hand-written backward, float32, operation by operation in the order of the torch twin (model/render/renderutils/ops.py).  Plain inline
// functions over registers: bsdf.hip wraps them with the loads, stores and reductions.  (Also compiles as host C++ -- nothing here is
// HIP -- so the derivatives can be checked against autograd on a CPU.)
//
// Subgradients at the kinks are torch's: clamp passes the gradient where the input lies inside or ON the bounds, where() passes none to
// the branch not taken, abs has gradient 0 at 0 (sign), normalize divides by max(|x|, 1e-12) and the norm has gradient 0 at 0.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define BSDF_FN __host__ __device__ __forceinline__
#else
#define BSDF_FN inline
#endif

namespace bsdf {

// Every function is a template over the scalar T the arithmetic is carried in: float (the forwards, the per-pixel backwards) or double
// (the backward of a call that reduces a gradient over pixels, bsdf.hip).  The clamp bounds are the float32 values in both.
constexpr float EPS = 1e-4f;                    // specular_epsilon (bsdf.py:94)
constexpr float ONE_M_EPS = (float)(1.0 - 1e-4);
constexpr double PI = 3.14159265358979323846;
constexpr float NORM_EPS = 1e-12f;              // F.normalize
constexpr float SRGB_T = 0.0031308f;

template <typename T>
struct V3T {
    T x, y, z;
};

template <typename T>
BSDF_FN V3T<T> v3(T x, T y, T z) { return V3T<T>{x, y, z}; }
template <typename T>
BSDF_FN V3T<T> operator+(V3T<T> a, V3T<T> b) { return V3T<T>{a.x + b.x, a.y + b.y, a.z + b.z}; }
template <typename T>
BSDF_FN V3T<T> operator-(V3T<T> a, V3T<T> b) { return V3T<T>{a.x - b.x, a.y - b.y, a.z - b.z}; }
template <typename T>
BSDF_FN V3T<T> operator*(V3T<T> a, V3T<T> b) { return V3T<T>{a.x * b.x, a.y * b.y, a.z * b.z}; }
template <typename T>
BSDF_FN V3T<T> operator*(V3T<T> a, T s) { return V3T<T>{a.x * s, a.y * s, a.z * s}; }
template <typename T>
BSDF_FN void operator+=(V3T<T>& a, V3T<T> b) { a.x += b.x; a.y += b.y; a.z += b.z; }
template <typename T>
BSDF_FN void operator-=(V3T<T>& a, V3T<T> b) { a.x -= b.x; a.y -= b.y; a.z -= b.z; }
template <typename T>
BSDF_FN T dot(V3T<T> a, V3T<T> b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
template <typename T>
BSDF_FN T hsum(V3T<T> a) { return a.x + a.y + a.z; }
// torch's clamp: a NaN stays a NaN (fminf / fmaxf would return the bound)
template <typename T>
BSDF_FN T maxf(T x, double lo_) {
    const T lo = (T)lo_;
    return x < lo ? lo : x;
}
template <typename T>
BSDF_FN T clampf(T x, double lo_, double hi_) {
    const T lo = (T)lo_, hi = (T)hi_;
    return x < lo ? lo : (x > hi ? hi : x);
}
template <typename T>
BSDF_FN T signf(T x) { return T(x > T(0.)) - T(x < T(0.)); }

template <typename T>
BSDF_FN V3T<T> normalize(V3T<T> v) {
    const T d = maxf(sqrt(dot(v, v)), NORM_EPS);
    return V3T<T>{v.x / d, v.y / d, v.z / d};
}

// gradient of normalize(v) w.r.t. v for the output gradient g: g / d - v (g . v) / (d^2 n) where the clamp passes (n >= eps)
template <typename T>
BSDF_FN V3T<T> normalize_bwd(V3T<T> v, V3T<T> g) {
    const T n = sqrt(dot(v, v));
    const T d = maxf(n, NORM_EPS);
    V3T<T> r = V3T<T>{g.x / d, g.y / d, g.z / d};
    if (n >= NORM_EPS) {
        const T s = dot(g, v) / (d * d) / n;
        r -= v * s;
    }
    return r;
}

// Schlick's (1 - clamp(c))^5 and its derivative w.r.t. c (0 outside the clamp)
template <typename T>
BSDF_FN void schlick_pow(T c, T& p, T& dp_dc) {
    const T cc = clampf(c, EPS, ONE_M_EPS);
    const T t = T(1.) - cc, t2 = t * t, t4 = t2 * t2;
    p = t4 * t;
    dp_dc = (c >= EPS && c <= ONE_M_EPS) ? -T(5.) * t4 : T(0.);
}

// D = a2 / (pi d^2), d = (c a2 - c) c + 1 with c clamped (bsdf.py:100-103)
template <typename T>
BSDF_FN T ndf_ggx(T a2, T c, T& dD_da2, T& dD_dc) {
    const T cc = clampf(c, EPS, ONE_M_EPS);
    const T e = cc * a2 - cc;
    const T d = e * cc + T(1.);
    const T q = d * d * T(PI);
    const T D = a2 / q;
    const T g_d = -(D / q) * (T(2.) * d * T(PI));
    dD_da2 = T(1.) / q + g_d * (cc * cc);
    dD_dc = (c >= EPS && c <= ONE_M_EPS) ? g_d * (e + cc * (a2 - T(1.))) : T(0.);
    return D;
}

// Lambda = (sqrt(1 + a2 tan^2) - 1) / 2 with c clamped (bsdf.py:105-110)
template <typename T>
BSDF_FN T lambda_ggx(T a2, T c, T& dL_da2, T& dL_dc) {
    const T cc = clampf(c, EPS, ONE_M_EPS);
    const T c2 = cc * cc;
    const T tan2 = (T(1.) - c2) / c2;
    const T s = sqrt(T(1.) + a2 * tan2);
    const T g_u = T(0.25) / s;  // d res / d (1 + a2 tan2)
    dL_da2 = g_u * tan2;
    dL_dc = (c >= EPS && c <= ONE_M_EPS) ? -(g_u * a2) / (c2 * c2) * (T(2.) * cc) : T(0.);
    return T(0.5) * (s - T(1.));
}

// ---- lambert (bsdf.py:57-58)
template <typename T>
BSDF_FN T lambert_fwd(V3T<T> nrm, V3T<T> wi) { return maxf(dot(nrm, wi), T(0.)) / T(PI); }

template <typename T>
BSDF_FN void lambert_bwd(V3T<T> nrm, V3T<T> wi, T g, V3T<T>& g_nrm, V3T<T>& g_wi) {
    const T g_dot = dot(nrm, wi) >= T(0.) ? g / T(PI) : T(0.);
    g_nrm += wi * g_dot;
    g_wi += nrm * g_dot;
}

// ---- frostbite diffuse (bsdf.py:64-79)
template <bool BWD, typename T>
BSDF_FN T frostbite(V3T<T> nrm, V3T<T> wi, V3T<T> wo, T lr, T g, V3T<T>& g_nrm, V3T<T>& g_wi, V3T<T>& g_wo, T& g_lr) {
    const T wiDotN = dot(wi, nrm), woDotN = dot(wo, nrm);
    const V3T<T> hs = wo + wi;
    const V3T<T> h = normalize(hs);
    const T wiDotH = dot(wi, h);
    const T bias = T(0.5) * lr;
    const T factor = T(1.) - T(0.51 / 1.51) * lr;
    const T f90 = bias + T(2.) * wiDotH * wiDotH * lr;
    T pi_, dpi, po, dpo;
    schlick_pow(wiDotN, pi_, dpi);
    schlick_pow(woDotN, po, dpo);
    const T wiS = T(1.) + (f90 - T(1.)) * pi_;
    const T woS = T(1.) + (f90 - T(1.)) * po;
    const bool lit = wiDotN > T(0.) && woDotN > T(0.);
    const T res = lit ? wiS * woS * factor : T(0.);
    if (BWD && lit) {
        const T g_wiS = g * woS * factor, g_woS = g * wiS * factor, g_factor = g * (wiS * woS);
        const T g_f90 = g_wiS * pi_ + g_woS * po;
        const T g_wiDotN = g_wiS * (f90 - T(1.)) * dpi;
        const T g_woDotN = g_woS * (f90 - T(1.)) * dpo;
        g_lr += g_factor * -T(0.51 / 1.51) + g_f90 * T(0.5) + g_f90 * (T(2.) * wiDotH * wiDotH);
        const T g_wiDotH = g_f90 * (T(4.) * wiDotH * lr);
        const V3T<T> g_h = wi * g_wiDotH;
        const V3T<T> g_hs = normalize_bwd(hs, g_h);
        g_wi += nrm * g_wiDotN + h * g_wiDotH + g_hs;
        g_wo += nrm * g_woDotN + g_hs;
        g_nrm += wi * g_wiDotN + wo * g_woDotN;
    }
    return res;
}

// ---- GGX specular (bsdf.py:117-134).  min_a = min_roughness^2
template <bool BWD, typename T>
BSDF_FN V3T<T> pbr_specular(V3T<T> col, V3T<T> nrm, V3T<T> wo, V3T<T> wi, T alpha, T min_a, V3T<T> g, V3T<T>& g_col, V3T<T>& g_nrm, V3T<T>& g_wo, V3T<T>& g_wi,
                        T& g_alpha) {
    const T al = clampf(alpha, min_a, T(1.));
    const T a2 = al * al;
    const V3T<T> hs = wo + wi;
    const V3T<T> h = normalize(hs);
    // (x . hs) / |hs| instead of x . (hs / |hs|): the same number with three roundings less -- nDotH feeds the GGX denominator
    // 1 - c^2 (1 - a2), which magnifies its rounding by up to 2 c / d (40 x at c = 0.96, alpha = 0.09)
    const T hd = maxf(sqrt(dot(hs, hs)), NORM_EPS);
    const T woDotN = dot(wo, nrm), wiDotN = dot(wi, nrm), woDotH = dot(wo, hs) / hd, nDotH = dot(nrm, hs) / hd;
    T dD_da2, dD_dc, dLi_da2, dLi_dc, dLo_da2, dLo_dc, p, dp;
    const T D = ndf_ggx(a2, nDotH, dD_da2, dD_dc);
    const T Li = lambda_ggx(a2, woDotN, dLi_da2, dLi_dc);
    const T Lo = lambda_ggx(a2, wiDotN, dLo_da2, dLo_dc);
    const T G = T(1.) / (T(1.) + Li + Lo);
    schlick_pow(woDotH, p, dp);
    const V3T<T> F = V3T<T>{col.x + (T(1.) - col.x) * p, col.y + (T(1.) - col.y) * p, col.z + (T(1.) - col.z) * p};
    const T m = maxf(woDotN, EPS);
    const bool front = woDotN > EPS && wiDotN > EPS;
    const V3T<T> w = V3T<T>{F.x * D * G * T(0.25) / m, F.y * D * G * T(0.25) / m, F.z * D * G * T(0.25) / m};
    if (BWD && front) {
        const T k = T(0.25) / m;
        const V3T<T> g_F = g * (D * G * k);
        const T gF = dot(g, F);
        const T g_D = gF * (G * k), g_G = gF * (D * k);
        const T g_m = -dot(g, w) / m;  // (front: woDotN > eps, the clamp passes)
        g_col += g_F * (T(1.) - p);
        const T g_woDotH = (g_F.x * (T(1.) - col.x) + g_F.y * (T(1.) - col.y) + g_F.z * (T(1.) - col.z)) * dp;
        const T g_L = -g_G * (G * G);
        const T g_a2 = g_D * dD_da2 + g_L * (dLi_da2 + dLo_da2);
        const T g_nDotH = g_D * dD_dc;
        const T g_woDotN = g_L * dLi_dc + g_m;
        const T g_wiDotN = g_L * dLo_dc;
        g_alpha += (alpha >= min_a && alpha <= T(1.)) ? g_a2 * (T(2.) * al) : T(0.);
        const V3T<T> g_h = wo * g_woDotH + nrm * g_nDotH;
        const V3T<T> g_hs = normalize_bwd(hs, g_h);
        g_wo += nrm * g_woDotN + h * g_woDotH + g_hs;
        g_wi += nrm * g_wiDotN + g_hs;
        g_nrm += wo * g_woDotN + wi * g_wiDotN + h * g_nDotH;
    }
    return front ? w : V3T<T>{T(0.), T(0.), T(0.)};
}

// ---- diffuse + specular of a point light (bsdf.py:136-151).  lobe: 0 lambert, 1 frostbite
template <bool BWD, typename T>
BSDF_FN V3T<T> pbr_bsdf(V3T<T> kd, V3T<T> arm, V3T<T> pos, V3T<T> nrm, V3T<T> view, V3T<T> light, T min_a, int lobe, V3T<T> g, V3T<T>& g_kd, V3T<T>& g_arm, V3T<T>& g_pos,
                    V3T<T>& g_nrm, V3T<T>& g_view, V3T<T>& g_light) {
    const V3T<T> vo = view - pos, vi = light - pos;
    const V3T<T> wo = normalize(vo), wi = normalize(vi);
    const T spec = arm.x, rough = arm.y, metal = arm.z;
    const T om = T(1.) - metal, os = T(1.) - spec;
    const V3T<T> u = V3T<T>{T(0.04) * om + kd.x * metal, T(0.04) * om + kd.y * metal, T(0.04) * om + kd.z * metal};
    const V3T<T> ks = u * os;
    const V3T<T> kdd = kd * om;
    V3T<T> g_wo = V3T<T>{T(0.), T(0.), T(0.)}, g_wi = g_wo, g_ks = g_wo, gn = g_wo;
    T g_rough = T(0.), g_alpha = T(0.);
    T dif;
    if (lobe == 0) {
        dif = lambert_fwd(nrm, wi);
        if (BWD) lambert_bwd(nrm, wi, dot(g, kdd), gn, g_wi);
    } else {
        dif = frostbite<BWD>(nrm, wi, wo, rough, BWD ? dot(g, kdd) : T(0.), gn, g_wi, g_wo, g_rough);
    }
    const V3T<T> sp = pbr_specular<BWD>(ks, nrm, wo, wi, rough * rough, min_a, g, g_ks, gn, g_wo, g_wi, g_alpha);
    if (BWD) {
        g_rough += g_alpha * (T(2.) * rough);
        const V3T<T> g_kdd = g * dif;
        const V3T<T> g_u = g_ks * os;
        g_kd += g_u * metal + g_kdd * om;
        g_arm += V3T<T>{-dot(g_ks, u), g_rough,
                    (g_u.x * kd.x + g_u.y * kd.y + g_u.z * kd.z) - T(0.04) * hsum(g_u) - dot(g_kdd, kd)};
        const V3T<T> g_vo = normalize_bwd(vo, g_wo), g_vi = normalize_bwd(vi, g_wi);
        g_view += g_vo;
        g_light += g_vi;
        g_pos -= g_vo + g_vi;
        g_nrm += gn;
    }
    return kdd * dif + sp;
}

// ---- HDR image loss, per element (loss.py:16-41).  loss: 0 l1, 1 mse, 2 smape, 3 relmse; tonemap: 0 none, 1 log_srgb
template <typename T>
BSDF_FN T tonemap(T x, T& d_dx) {
    const T xc = clampf(x, T(0.), T(65535.));
    const T f = log(xc + T(1.));
    T y, dy_df;
    if (f > SRGB_T) {
        const T fc = maxf(f, SRGB_T);
        const T pw = pow(fc, T(1.0 / 2.4));
        y = pw * T(1.055) - T(0.055);
        dy_df = T(1.055) * (T(1.0 / 2.4) * pw / fc);
    } else {
        y = T(12.92) * f;
        dy_df = T(12.92);
    }
    d_dx = (x >= T(0.) && x <= T(65535.)) ? dy_df / (xc + T(1.)) : T(0.);
    return y;
}

// value of one element; d_a, d_b: its derivatives w.r.t. img and target (before the 1 / N of the mean)
template <typename T>
BSDF_FN T image_loss(T a, T b, int loss, int tm, T& d_a, T& d_b) {
    T ta = T(1.), tb = T(1.);
    if (tm) {
        a = tonemap(a, ta);
        b = tonemap(b, tb);
    }
    const T diff = a - b;
    T v, ga, gb;
    if (loss == 1) {
        v = diff * diff;
        ga = T(2.) * diff;
        gb = -ga;
    } else if (loss == 2) {
        const T nom = fabs(diff), den = fabs(a) + fabs(b) + T(0.01);
        v = nom / den;
        const T g_den = -(v / den), s = signf(diff) / den;
        ga = s + g_den * signf(a);
        gb = -s + g_den * signf(b);
    } else if (loss == 3) {
        const T nom = diff * diff, den = a * a + b * b + T(0.1);
        v = nom / den;
        const T g_den = -(v / den), s = T(2.) * diff / den;
        ga = s + g_den * (T(2.) * a);
        gb = -s + g_den * (T(2.) * b);
    } else {
        v = fabs(diff);
        ga = signf(diff);
        gb = -ga;
    }
    d_a = ga * ta;
    d_b = gb * tb;
    return v;
}

}  // namespace bsdf
