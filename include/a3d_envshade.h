/* liba3d_hip: environment-lit shading (the sixth public header of the library; the core surface is a3d.h, the BSDFs are a3d_bsdf.h, the
 * image-space derivatives a3d_deriv.h, the tangent frame a3d_tangent.h, the mesh regularisers a3d_reg.h).
 *
 * Same conventions as a3d.h: flat C, device pointers + sizes + a3d_stream_t, int status (A3D_OK / A3D_EINVAL / A3D_EHIP) with the
 * message in a3d_last_error(), arguments validated before anything is launched, no allocation and no synchronisation inside a call.
 * The entry points live in the same liba3d_hip.so; they do not change a3d_version().
 *
 * EnvironmentLight.shade (reference model/render/light.py:90-128), the split-sum shade under an environment map, as ONE launch each way:
 *     wo = safe_normalize(view_pos - gb_pos),  refl = safe_normalize(2 dot(wo, n) n - wo),  safe_normalize(x) = x / sqrt(max(x.x, 1e-20))
 *     with mtx: refl and n are rotated by its 3 x 3 part (w = 0) for the lookups
 *     col = cube(diffuse, n) * diff_col                                  diff_col = kd (1 - ks.z) with the specular term, kd without
 *     with the specular term:
 *         ndv = max(dot(wo, n), 1e-4),  (A, B) = linear clamp lookup of the FG table at (ndv, ks.y)
 *         level = ks.y < hi ? (clamp(ks.y, lo, hi) - lo) / (hi - lo) * (L - 2) : (clamp(ks.y, hi, 1) - hi) / (1 - hi) + L - 2
 *         col += trilinear cube(specular stack, refl, level) * (((1 - ks.z) 0.04 + kd ks.z) A + B)
 *     out = col (1 - ks.x)
 * The three lookups are a3d_texture_fwd's own device code (cube face ties, edge walk, corner tap, a zero direction samples 0, the
 * level clamp); float32, operation by operation.
 */
#ifndef A3D_ENVSHADE_H
#define A3D_ENVSHADE_H

#include "a3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the per-pixel inputs of a3d_env_shade_desc, in EnvironmentLight.shade's argument order */
#define A3D_ENV_SHADE_POS 0
#define A3D_ENV_SHADE_NORMAL 1
#define A3D_ENV_SHADE_KD 2
#define A3D_ENV_SHADE_KS 3
#define A3D_ENV_SHADE_VIEW 4
#define A3D_ENV_SHADE_INPUTS 5

/* Set ``size`` to sizeof(a3d_env_shade_desc): a shorter struct (a caller built against an older header) is refused before any other
 * field is read.  Every map is float32 [6, S, S, 3] (texture batch 1); strides are in ELEMENTS. */
typedef struct a3d_env_shade_desc {
    uint32_t size;
    int32_t levels;          /* specular levels: 3 .. A3D_TEX_MAX_LEVELS, spec_size[l] = spec_size[l - 1] / 2 (the halving rule) */
    int32_t diffuse_size;    /* S of the diffuse irradiance map */
    int32_t fg_height, fg_width; /* the FG table [fg_height, fg_width, 2]: u = ndv along the width, v = roughness along the height */
    int32_t specular;        /* 0: out = cube(diffuse, n) kd (1 - ks.x); the specular stack, the FG table and the roughness constants are not read */
    int32_t mtx_batch;       /* 0: no lookup transform; 1: one [4,4]; B: one per image */
    int32_t B, H, W;         /* pixels; a wave takes an 8 x 8 tile when H >= 8 and W >= 8, 64 consecutive pixels otherwise (a point
                                list [1,1,P] uses every lane); a pixel's arithmetic does not depend on which */
    float min_roughness, max_roughness; /* lo, hi of the level rule */
    int32_t spec_size[A3D_TEX_MAX_LEVELS];
    const float* diffuse;
    const float* spec[A3D_TEX_MAX_LEVELS];
    const float* fg;
    const float* mtx;        /* [mtx_batch, 4, 4] row-major, contiguous; only rows / columns 0..2 are read */
    float* g_diffuse;        /* bwd: NULL = wants none; the callee ADDS into the buffer (hand it zeroed), as a3d_texture_bwd does */
    float* g_spec[A3D_TEX_MAX_LEVELS];
    const float* in[A3D_ENV_SHADE_INPUTS]; /* 3 adjacent floats per pixel at in[i] + b * image_stride[i] + (y * W + x) * pixel_stride[i] */
    int64_t pixel_stride[A3D_ENV_SHADE_INPUTS]; /* 0: constant over the image (view_pos [B,1,1,3]); 9: a slice of a [...,9] row */
    int64_t image_stride[A3D_ENV_SHADE_INPUTS];
    float* out;              /* fwd: [B*H*W, 3] */
    const float* g_out;      /* bwd: [B*H*W, 3], contiguous */
    float* g_in[4];          /* bwd: g_pos, g_normal, g_kd, g_ks, [B*H*W, 3] each, NULL = not wanted; stored once per pixel.  The
                                gradient of view_pos is exactly -g_pos per pixel and is not written */
} a3d_env_shade_desc;

/* fwd reads in[], the maps and mtx and writes out; one launch, one lane per pixel.
 * bwd reads in[], the maps, mtx and g_out, recomputes the forward (nothing else is saved) and writes the wanted g_in[] with plain stores
 * -- hand-written reverse mode through the three lookups, both normalisations, the reflection, the rotation (its transpose), the level
 * rule and the FG coordinates; two calls give the same bits -- and ADDS the texel gradients into g_diffuse / g_spec[]: maps of at most
 * 16 x 16 texels per face are summed in LDS per work-group and leave as one global atomic per non-zero float; larger levels merge
 * equal texels inside the wave first (a3d_texture_bwd's route).  The FG table and mtx receive no gradient.
 * Subgradients are autograd's: clamp(min) passes on >=, clamp(lo, hi) on the closed interval, where passes nothing to the branch not
 * taken, the level gradient reaches ks.y only where the level is not clamped to [0, L - 1], and the direction gradients of the cube
 * lookups treat the level as a constant. */
int a3d_env_shade_fwd(const a3d_env_shade_desc* desc, a3d_stream_t stream);
int a3d_env_shade_bwd(const a3d_env_shade_desc* desc, a3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
