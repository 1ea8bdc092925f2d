"""csrc/envshade.hip (ops.env_shade, EnvironmentLight.shade with HIP_ENV_SHADE on) against the hand-written float64 reverse mode of
tests/envshade_hard_ref.py, element by element, on the named hard cases of that module.

Bound, for every element of the values and of every gradient: |hip - x64| <= 2^-24 (4 MEASURED[case][quantity] magnitude + 4 |x64|),
MEASURED = what the float32 evaluation of the same restatement reaches on the CPU (tests/test_envshade_adversarial_cpu.py), the
magnitude = the chain with absolute values.  The factor 4 is for another summation order (LDS and memory atomics, the in-wave merge,
against a sequential scatter).  No case needed more.  No pixel and no element is left out; an element nothing feeds must be exactly 0.
Every case runs twice -- through EnvironmentLight.shade where its operand shapes take the fused path (all but the operand-form cases)
and through ops.env_shade --: values and per-pixel gradients bit-identical, map gradients inside the bound both times.

What the twelve gaps of the issue showed on an MI355X: nothing outside the bound.  Largest device figure / CPU float32 figure over all
cases and quantities: 1.51 (conc_frame_lds g_specular[1], 0.783 against 0.519 units); the allowance is 4.
   1 per-element bound: holds on all 48 cases; tests/test_envshade_adversarial_cpu.py shows that it rejects five broken reverse modes, two
     of which the per-tensor bound accepts.
   2 diffuse map on the merge route (light_d, conc_*_merge, geo_S32): did not show.
   3 levels of size 2 and 1 under larger ones, 6 and 16 levels, the LDS plan with 13 one-texel maps (light_e .. light_h, geo_S1): did not show.
   4 wanted gradients one by one (wanted_*): the library is handed no buffer for an unwanted gradient, the others are inside the bound;
     only view_pos wanting a gradient (needs[8] without needs[4]) gives g_view = -sum g_pos.  Did not show.
   5 concentrated scatter (conc_*: 1024 lanes on one quad, two quads on two faces, one quad per wave; LDS and merge): 0.3 - 9 units on
     the one-quad cases against 0.4 - 10 on the CPU.  Did not show.
   6 pixels exactly on a kink (kink_*, geo_*): the kernel stands where the float32 statements stand, and the zero pattern of its map
     gradients and of g_ks is the restatement's.  One float32 step below hi and below 1 the float32 level rounds onto the integer, so the
     level that float64 gives a weight of 1e-7 gets none: 2^24 units in the restatement and in the kernel alike, which makes the bound of
     kink_roughness_one_ulp_beside on g_specular[2..4] and g_ks empty; that case is held by the zero pattern.  Did not show.
   7 degenerate vectors against float64 (degenerate_vectors: zero normal, camera on the point, |view - pos| = 1e-11 and 1e-9 around the
     1e-20 clamp, |n| = 1e-3 and 1e3): did not show.
   8 transforms that are no rotations (xfm_*: zero -- every output exactly 0 --, reflection, shear, scales 1e-20 and 1e20, three
     matrices): did not show.
   9 a non-finite pixel (nonfinite_*): the NaN pattern is the float64 reference's, every other row and texel is inside the bound of the
     benign frame.  Did not show.
  10 frames around the tiling rule and the 256-lane work-group (frame_*): did not show.
  11 magnitudes (mag_*: texels at 1e30, 1e-30 and 0; g_out to 1e20; positions at 1e4, camera 1e-2 away): nothing overflows in the
     float32 restatement and nothing does in the kernel.  Did not show.
  12 operand forms (operands_*: kd [1,1,1,3], ks [B,1,1,3], gb_normal [1,H,W,3], expanded view_pos, gb_pos [B,H,1,3] on the copy path;
     through ops.env_shade, EnvironmentLight.shade sends such shapes to the statements): did not show.
No change to csrc/envshade.hip, csrc/tex_lookup.h or ops.py came out of this pass.

Measured on an MI355X, the largest figure over both runs of a case, in units of 2^-24 x magnitude, with the float32 restatement's
figure on the CPU (envshade_hard_ref.MEASURED, of which the bound is 4 x) in parentheses; g_specular lists the levels in order:
  light_a_8_4_2: values 19.6 (21.5); g_pos 1.76 (1.83); g_normal 2.39 (2.68); g_kd 17.5 (19.2); g_ks 8.21 (8.69); g_view 1.76 (1.83); g_diffuse 3.51 (3.85); g_specular[0..] 767 (767), 82 (82.3), 16 (16)
  light_b_64_32_16: values 231 (231); g_pos 11.1 (11); g_normal 16.5 (16.8); g_kd 44.2 (44.2); g_ks 45.7 (44.2); g_view 11.1 (11); g_diffuse 2.19e+03 (2.19e+03); g_specular[0..] 5.2e+03 (5.2e+03), 1.14e+04 (1.14e+04), 3.83e+03 (1.39e+04)
  light_c_64_to_4: values 91.6 (91.6); g_pos 5.43 (5.43); g_normal 10.5 (10.5); g_kd 41.5 (42.6); g_ks 29.8 (30.8); g_view 5.43 (5.43); g_diffuse 69.4 (69.4); g_specular[0..] 1.16e+03 (1.16e+03), 1.06e+04 (1.06e+04), 287 (287), 2.41e+03 (2.41e+03), 269 (269)
  light_d_64_32_16_dif32: values 188 (188); g_pos 11.1 (11); g_normal 16.4 (16.5); g_kd 42.2 (42.2); g_ks 44.6 (43.1); g_view 11.1 (11); g_diffuse 3.53e+03 (3.53e+03); g_specular[0..] 5.2e+03 (5.2e+03), 1.14e+04 (1.14e+04), 3.83e+03 (1.39e+04)
  light_e_4_2_1_dif1: values 4.72 (4.72); g_pos 1.01 (1.07); g_normal 1.65 (1.86); g_kd 4.2 (4.79); g_ks 3.94 (3.77); g_view 1.01 (1.07); g_diffuse 1.35 (1.78); g_specular[0..] 217 (217), 7.36 (7.36), 2.27 (2.78)
  light_f_2_1_1_dif2: values 6.45 (6.45); g_pos 1.21 (1.36); g_normal 1.12 (1.74); g_kd 4.35 (4.7); g_ks 2.76 (3.85); g_view 1.21 (1.36); g_diffuse 3.51 (3.85); g_specular[0..] 33.5 (33.5), 2.41 (2.26), 2.27 (2.78)
  light_g_16_to_1_1: values 24 (24); g_pos 1.78 (2); g_normal 4.02 (4.47); g_kd 38.3 (38.3); g_ks 10.2 (11); g_view 1.78 (2); g_diffuse 2.19e+03 (2.19e+03); g_specular[0..] 404 (404), 201 (201), 44.4 (44.4), 73.7 (73.7), 6.1 (7.32), 2.75 (2.34)
  light_h_16_levels: values 19.9 (19.9); g_pos 5.8 (5.82); g_normal 14.7 (16); g_kd 22.6 (21.3); g_ks 12.1 (11.7); g_view 5.8 (5.82); g_diffuse 4.58e+03 (4.58e+03); g_specular[0..] 773 (773), 88.6 (88.6), 477 (477), 18.7 (18.7), 7.7 (7.7), 10.5 (10.5), 711 (711), 25 (24.8), 29.1 (30.4), 68.7 (68.7), 92.2 (92.2), 63.4 (63.4), 64.5 (64.5), 63 (63), 12.6 (12.6), 11.1 (11.9)
  wanted_no_diffuse: values 40.2 (40.2); g_pos 9.61 (9.52); g_normal 12.9 (12.6); g_kd 28.1 (27); g_ks 34.2 (32.7); g_view 9.61 (9.52); g_specular[0..] 5.59e+04 (5.59e+04), 3.25e+03 (3.25e+03), 2.67e+03 (2.67e+03)
  wanted_no_level0: values 40.2 (40.2); g_pos 9.61 (9.52); g_normal 12.9 (12.6); g_kd 28.1 (27); g_ks 34.2 (32.7); g_view 9.61 (9.52); g_diffuse 739 (739); g_specular[0..] 3.25e+03 (3.25e+03), 2.67e+03 (2.67e+03)
  wanted_only_maps: values 40.2 (40.2); g_diffuse 739 (739); g_specular[0..] 5.59e+04 (5.59e+04), 3.25e+03 (3.25e+03), 2.67e+03 (2.67e+03)
  wanted_only_view: values 40.2 (40.2); g_view 9.61 (9.52)
  conc_list_lds: values 4.58 (4.58); g_pos 0.029 (0.053); g_normal 0.149 (0.309); g_kd 4.16 (4.95); g_ks 2.89 (3.44); g_view 0.029 (0.053); g_diffuse 0.587 (1.53); g_specular[0..] 0.379 (0.36), 0.428 (0.76), 0 (0)
  conc_list_merge: values 5.3 (5.3); g_pos 0.075 (0.179); g_normal 0.83 (0.939); g_kd 4.94 (4.53); g_ks 3.7 (3.24); g_view 0.075 (0.179); g_diffuse 1.59 (1.59); g_specular[0..] 4.67 (4.49), 0.312 (0.675), 0 (0)
  conc_frame_lds: values 4.83 (3.74); g_pos 0.031 (0.043); g_normal 0.11 (0.198); g_kd 3.55 (3.97); g_ks 3.08 (3.44); g_view 0.031 (0.043); g_diffuse 0.617 (0.756); g_specular[0..] 0.86 (1.29), 0.783 (0.519), 0 (0)
  conc_frame_merge: values 5.23 (5.24); g_pos 0.068 (0.19); g_normal 0.927 (1.13); g_kd 3.99 (4.84); g_ks 3.91 (3.67); g_view 0.068 (0.19); g_diffuse 1.7 (2.07); g_specular[0..] 8.96 (10.1), 0.778 (1.78), 0 (0)
  conc_two_quads: values 40.7 (41.4); g_pos 5.07 (5.11); g_normal 9.05 (9.01); g_kd 41.3 (39.4); g_ks 22.1 (21.6); g_view 5.07 (5.11); g_diffuse 12.4 (11.8); g_specular[0..] 74.9 (74.7), 11.6 (11.8), 0 (0)
  conc_quad_per_wave: values 78.7 (78.7); g_pos 15 (14.9); g_normal 25.9 (25.6); g_kd 116 (117); g_ks 41.7 (41.2); g_view 15 (14.9); g_diffuse 185 (184); g_specular[0..] 221 (218), 128 (126), 0 (0)
  geo_S1: values 4.45 (3.58); g_pos 0.833 (0.95); g_normal 1.13 (1.13); g_kd 3.73 (3.56); g_ks 2.57 (2.57); g_view 0.833 (0.95); g_diffuse 1.9 (1.9); g_specular[0..] 68.5 (68.5), 3.76 (3.92), 3.05 (3.05)
  geo_S2: values 5.13 (5.13); g_pos 0.657 (0.772); g_normal 0.91 (1.08); g_kd 3.6 (4.02); g_ks 3.08 (2.81); g_view 0.657 (0.772); g_diffuse 3.44 (3.44); g_specular[0..] 380 (380), 34.8 (34.8), 4.34 (3.98)
  geo_S16: values 27.2 (27.2); g_pos 4.39 (4.73); g_normal 5.18 (5.12); g_kd 25.1 (23.2); g_ks 21.1 (21.1); g_view 4.39 (4.73); g_diffuse 548 (548); g_specular[0..] 7.05e+03 (7.05e+03), 614 (614), 278 (278)
  geo_S32: values 29 (29); g_pos 4.39 (4.73); g_normal 6.83 (7.07); g_kd 31.4 (30.4); g_ks 22.7 (22.7); g_view 4.39 (4.73); g_diffuse 796 (796); g_specular[0..] 7.05e+03 (7.05e+03), 614 (614), 278 (278)
  kink_roughness: values 80.3 (80.3); g_pos 4.17 (4.15); g_normal 12.1 (11.5); g_kd 19.3 (17.7); g_ks 32.1 (32.1); g_view 4.17 (4.15); g_diffuse 122 (122); g_specular[0..] 2.19e+03 (2.19e+03), 363 (363), 304 (304), 609 (609), 142 (142)
  kink_roughness_one_ulp_beside: values 47.7 (50.8); g_pos 6.7 (6.7); g_normal 12.5 (12.5); g_kd 41.4 (43.1); g_ks 3.93e+04 (3.93e+04); g_view 6.7 (6.7); g_diffuse 122 (122); g_specular[0..] 2.19e+03 (2.19e+03), 363 (363), 2.08e+07 (2.08e+07), 1.68e+07 (1.68e+07), 1.68e+07 (1.68e+07)
  kink_n_dot_v: values 27.2 (27.2); g_pos 8.85 (8.68); g_normal 15.2 (14.8); g_kd 25.3 (26.4); g_ks 21.1 (21.1); g_view 8.85 (8.68); g_diffuse 562 (562); g_specular[0..] 7.05e+03 (7.05e+03), 614 (614), 278 (278)
  degenerate_vectors: values 108 (108); g_pos 17 (17); g_normal 22.4 (22.4); g_kd 66 (66); g_ks 74.3 (74.3); g_view 17 (17); g_diffuse 587 (587); g_specular[0..] 7.05e+03 (7.05e+03), 1.01e+03 (1.01e+03), 278 (278)
  xfm_zero: values 0 (0); g_pos 0 (0); g_normal 0 (0); g_kd 0 (0); g_ks 0 (0); g_view 0 (0); g_diffuse 0 (0); g_specular[0..] 0 (0), 0 (0), 0 (0)
  xfm_reflection: values 99.9 (99.9); g_pos 7.78 (7.78); g_normal 12.8 (13); g_kd 35.9 (34.1); g_ks 16.6 (16.7); g_view 7.78 (7.78); g_diffuse 2.3e+03 (2.3e+03); g_specular[0..] 1.79e+03 (1.79e+03), 1.65e+03 (1.65e+03), 2.47e+03 (2.47e+03)
  xfm_shear: values 57.1 (57.1); g_pos 3.74 (3.54); g_normal 6.67 (6.38); g_kd 53.6 (54.9); g_ks 21.9 (23); g_view 3.74 (3.54); g_diffuse 463 (463); g_specular[0..] 3.92e+03 (3.92e+03), 2.05e+03 (2.05e+03), 404 (404)
  xfm_scale_1e-20: values 30.6 (30.6); g_pos 5.2 (5.18); g_normal 7.2 (7.35); g_kd 31.6 (32.8); g_ks 21.1 (21.1); g_view 5.2 (5.18); g_diffuse 587 (587); g_specular[0..] 7.05e+03 (7.05e+03), 1.48e+03 (1.48e+03), 970 (970)
  xfm_scale_1e20: values 37.8 (30.2); g_pos 7.49 (7.77); g_normal 10.6 (11); g_kd 34 (26.4); g_ks 21.1 (21.4); g_view 7.49 (7.77); g_diffuse 368 (368); g_specular[0..] 7.05e+03 (7.05e+03), 1.44e+03 (1.44e+03), 970 (970)
  xfm_three: values 73.7 (73.7); g_pos 9.97 (9.78); g_normal 10.3 (10.3); g_kd 62.6 (62.6); g_ks 46.5 (46.5); g_view 9.97 (9.78); g_diffuse 817 (817); g_specular[0..] 1.25e+04 (1.25e+04), 6.93e+03 (6.93e+03), 476 (476)
  frame_1x8x8: values 176 (176); g_pos 5.28 (5.43); g_normal 11 (10.9); g_kd 30.5 (30.5); g_ks 17.1 (17.1); g_view 0.103 (0.09); g_diffuse 2.63e+03 (2.63e+03); g_specular[0..] 758 (758), 1.34e+03 (1.34e+03), 1.52e+03 (1.52e+03)
  frame_1x8x9: values 77.6 (118); g_pos 10 (9.83); g_normal 11 (10.6); g_kd 75.7 (117); g_ks 44.1 (53.2); g_view 0.328 (0.619); g_diffuse 732 (732); g_specular[0..] 1.81e+03 (1.81e+03), 2.98e+03 (2.98e+03), 668 (668)
  frame_1x7x64: values 250 (250); g_pos 12.2 (12.1); g_normal 21.5 (21.7); g_kd 241 (241); g_ks 85 (85); g_view 0.165 (0.168); g_diffuse 1.16e+04 (1.16e+04); g_specular[0..] 2.01e+05 (2.01e+05), 1.68e+04 (1.68e+04), 7.43e+03 (7.43e+03)
  frame_3x16x8: values 127 (127); g_pos 6.52 (6.39); g_normal 9.84 (9.76); g_kd 73.5 (74.7); g_ks 52.3 (51.9); g_view 0.3 (0.307); g_diffuse 8.91e+03 (8.91e+03); g_specular[0..] 1.88e+04 (1.88e+04), 1.67e+04 (1.67e+04), 1.4e+03 (1.4e+03)
  frame_list255: values 118 (118); g_pos 15.2 (15.2); g_normal 19.2 (19.2); g_kd 93.6 (94.9); g_ks 57.1 (57.1); g_view 0.295 (0.319); g_diffuse 2.04e+03 (2.04e+03); g_specular[0..] 4.91e+03 (4.91e+03), 1.9e+04 (1.9e+04), 1.34e+03 (1.34e+03)
  frame_list256: values 73.6 (73.6); g_pos 7.67 (7.67); g_normal 13.3 (13); g_kd 67.9 (67.9); g_ks 64 (64); g_view 0.124 (0.16); g_diffuse 4.84e+03 (4.84e+03); g_specular[0..] 1.57e+04 (1.57e+04), 1.72e+04 (1.72e+04), 7.07e+03 (7.07e+03)
  mag_hdr_maps: values 1.02e+03 (1.02e+03); g_pos 147 (147); g_normal 359 (359); g_kd 1.02e+03 (1.02e+03); g_ks 854 (854); g_view 147 (147); g_diffuse 4.27e+04 (4.27e+04); g_specular[0..] 6.24e+03 (6.24e+03), 4.62e+03 (4.62e+03), 675 (675)
  mag_g_out_1e20: values 103 (103); g_pos 9.52 (9.42); g_normal 19.5 (19.8); g_kd 36.4 (33.4); g_ks 42.9 (42.9); g_view 9.52 (9.42); g_diffuse 4.27e+04 (4.27e+04); g_specular[0..] 6.24e+03 (6.24e+03), 4.62e+03 (4.62e+03), 674 (674)
  mag_far_positions: values 93.8 (93.8); g_pos 18.4 (18.2); g_normal 23.3 (22.7); g_kd 93.8 (93.8); g_ks 56.2 (56.2); g_view 18.4 (18.2); g_diffuse 4.27e+04 (4.27e+04); g_specular[0..] 8.7e+03 (8.7e+03), 3.01e+04 (3.01e+04), 1.9e+03 (1.9e+03)
  operands_broadcast: values 61 (61); g_pos 11.7 (11.3); g_normal 11.7 (11.1); g_kd 1.02 (0.731); g_ks 0.817 (0.884); g_view 0.158 (0.126); g_diffuse 899 (899); g_specular[0..] 1.12e+04 (1.12e+04), 3.27e+04 (3.27e+04), 724 (724)
  operands_pos_BH13: values 70.9 (70.9); g_pos 2.25 (2.22); g_normal 15 (14.5); g_kd 55.5 (55.5); g_ks 33.2 (33.2); g_view 0.319 (0.369); g_diffuse 898 (898); g_specular[0..] 7.89e+03 (7.89e+03), 1.36e+05 (1.36e+05), 2.82e+03 (2.8e+03)
  hidden_under_the_largest: values 102 (102); g_pos 14 (13.9); g_normal 16 (16); g_kd 100 (99); g_ks 50.2 (49.1); g_view 14 (13.9); g_diffuse 4.07e+03 (4.07e+03); g_specular[0..] 8.45e+04 (8.45e+04), 3.27e+03 (3.27e+03), 2.69e+03 (2.69e+03)
  nonfinite_nan_normal: values 27.2 (27.2); g_pos 4.39 (4.73); g_normal 7.2 (7.35); g_kd 25.3 (26.4); g_ks 21.4 (21.4); g_view 4.39 (4.73); g_diffuse 587 (587); g_specular[0..] 7.05e+03 (7.05e+03), 614 (614), 970 (970)
  nonfinite_inf_pos: values 27.2 (27.2); g_pos 4.39 (4.73); g_normal 7.2 (7.35); g_kd 25.3 (26.4); g_ks 21.4 (21.4); g_view 4.39 (4.73); g_diffuse 587 (587); g_specular[0..] 7.05e+03 (7.05e+03), 614 (614), 970 (970)
  nonfinite_nan_kd: values 27.2 (27.2); g_pos 4.39 (4.73); g_normal 7.2 (7.35); g_kd 25.3 (26.4); g_ks 21.4 (21.4); g_view 4.39 (4.73); g_diffuse 587 (587); g_specular[0..] 7.05e+03 (7.05e+03), 614 (614), 970 (970)
  nonfinite_nan_g_out: values 27.2 (27.2); g_pos 4.39 (4.73); g_normal 7.2 (7.35); g_kd 25.3 (26.4); g_ks 21.4 (21.4); g_view 4.39 (4.73); g_diffuse 587 (587); g_specular[0..] 7.05e+03 (7.05e+03), 614 (614), 970 (970)
"""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import envshade_cases as C  # noqa: E402
import envshade_hard_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _mods():
    return (importlib.import_module("3danimals_amd.ops"), importlib.import_module("3danimals_amd.model.render.light"),
            importlib.import_module("3danimals_amd._lib"))


@pytest.fixture(autouse=True)
def _same_fg_table_and_switch():
    """The device light reads the table the float64 side reads (rounded to float32 once), and the switch is back at its default."""
    _, light, _ = _mods()
    key = str(torch.device("cuda", torch.cuda.current_device()))
    before, had = light._fg_cache.get(key), key in light._fg_cache
    light._fg_cache[key] = C.fg_table().float().cuda()
    try:
        yield
    finally:
        light.HIP_ENV_SHADE = True
        if had:
            light._fg_cache[key] = before
        else:
            light._fg_cache.pop(key, None)


def _keys(case):
    return M.quantities(len(case["spec"]))


def _run(case, through_light, record=None):
    """-> quantity -> tensor on the CPU (None: not wanted) of one forward and one backward of the kernel."""
    ops, light, L = _mods()
    keys = _keys(case)
    wants = set(keys[1:] if case["wants"] is None else case["wants"])
    dev = lambda t, k: t.float().cuda().requires_grad_(k in wants)
    leaves = [dev(t, k) for t, k in zip(case["leaves"], M.PIXEL_KEYS)]
    dif = dev(case["dif"], "g_diffuse")
    spec = [dev(t, f"g_specular[{l}]") for l, t in enumerate(case["spec"])]
    B, H, W = case["shape"]
    args = [t.expand(B, H, W, 3) if i in case.get("expanded", ()) else t for i, t in enumerate(leaves)]
    mtx = None if case["mtx"] is None else case["mtx"].float().cuda()
    light.HIP_ENV_SHADE = True
    with L.KernelTimer() as timer:
        if through_light:
            lgt = light.EnvironmentLight(torch.zeros(6, 2, 2, 3, device="cuda"))
            lgt.specular, lgt.diffuse = spec, dif
            lgt.xfm(mtx)
            assert lgt._fused_ok(*args)
            out = lgt.shade(*args)
        else:
            out = ops.env_shade(dif, spec, light._fg_lut("cuda"), *args, mtx=mtx)
        wrt = [t for t, k in zip(leaves + [dif] + spec, keys[1:]) if k in wants]
        seen = []
        real = ops.call

        def call(name, d, *rest):
            seen.append((name, d._obj))
            return real(name, d, *rest)

        ops.call = call
        try:
            grads = torch.autograd.grad((out * case["go"].float().cuda()).sum(), wrt)
        finally:
            ops.call = real
    assert {k: len(v) for k, v in timer.records.items()} == {"a3d_env_shade_fwd": 1, "a3d_env_shade_bwd": 1}  # the kernel, and nothing else
    if record is not None:
        record.extend(seen)
    res = dict.fromkeys(keys)
    res["values"] = out.detach().cpu()
    for k, g in zip([k for k in keys[1:] if k in wants], grads):
        res[k] = g.cpu()
    return res


def _fused_shapes(case):
    s = [tuple(t.shape) for t in case["leaves"]]
    return s[0] == s[1] == s[2] == s[3] and not case.get("expanded")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _same_non_finite(g, x32):
    """Where the float32 restatement is inf or NaN, the kernel gives the same inf or a NaN where it gives one."""
    over = ~torch.isfinite(x32)
    a, b = g[over], x32[over]
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a[~torch.isnan(a)], b[~torch.isnan(b)])


def _check(name, got, ref, mag, where=None, figure_of=None):
    """prints the units of every produced quantity -> the quantities with an element outside the bound."""
    bad = []
    for k, g in got.items():
        if g is None:
            continue
        fig = M.figure(figure_of or name, k)
        assert g.dtype == F32 and g.shape == ref[k].shape, k
        m = mag[k] if where is None else torch.where(where[k], mag[k], torch.full_like(mag[k], float("nan")))  # (NaN: not looked at)
        print(f"{name}: {k} {M.units(g, ref[k], m):.3f} units on the device (float32 on the CPU {fig})")
        v = M.violations(g, ref[k], mag[k], fig, None if where is None else where[k])
        if len(v):
            i = tuple(v[0].tolist())
            bad.append((k, len(v), i, float(g[i]), float(ref[k][i]), float(mag[k][i])))
    return bad


FINITE = tuple(n for n in M.CASES if n not in M.NONFINITE)


@pytest.mark.parametrize("name", FINITE)
def test_every_element_against_float64(name):
    case = M.build(name)
    ref, mag, _ = M.reference(name)
    x32, _ = M.evaluate(case, F32, magnitudes=False)
    assert all(bool(torch.isfinite(ref[k]).all()) for k in ref)
    record = []
    runs = [_run(case, False, record)] + ([_run(case, True, record)] if _fused_shapes(case) else [_run(case, False, record)])
    for got in runs:
        assert not _check(name, got, ref, mag)
        assert all(_same_non_finite(g, x32[k]) for k, g in got.items() if g is not None)
    for k in ("values",) + M.PIXEL_KEYS:
        if runs[0][k] is not None:
            assert _same_bits(runs[0][k], runs[1][k]), k
    if name.startswith("kink_"):  # on a kink the kernel stands where the float32 statements stand: the same texels fed, the same zeros in g_ks
        for got in runs:
            assert all(torch.equal(got[k] != 0, x32[k] != 0) for k in got if k == "g_ks" or k.startswith("g_diffuse") or k.startswith("g_specular"))
    if case["wants"] is not None:  # the unwanted gradients are not produced: the library is handed no buffer for them
        wants = set(case["wants"])
        for got in runs:
            assert all((g is not None) == (k in wants or k == "values") for k, g in got.items())
        descs = [d for n, d in record if n == "a3d_env_shade_bwd"]
        assert len(descs) == 2
        for d in descs:
            assert bool(d.g_diffuse) == ("g_diffuse" in wants)
            assert [bool(d.g_spec[l]) for l in range(len(case["spec"]))] == [f"g_specular[{l}]" in wants for l in range(len(case["spec"]))]
            assert [bool(d.g_in[j]) for j in range(4)] == ["g_pos" in wants or "g_view" in wants] + [k in wants for k in M.PIXEL_KEYS[1:4]]


@pytest.mark.parametrize("name", tuple(M.NONFINITE))
def test_a_non_finite_pixel_stays_in_its_own_rows_and_texels(name):
    """The NaN pattern of every output equals the float64 reference's (and the float32 restatement's); every finite element is inside
    the bound; and every row and texel the bad pixel does not feed is inside the bound of the same case with that pixel made benign."""
    case = M.build(name)
    ref, mag, f = M.reference(name)
    ben_ref, ben_mag, fb = M.reference(name + "_benign")
    x32, _ = M.evaluate(case, F32, magnitudes=False)
    where = {}
    for k in ref:
        if k in ("values",) + M.PIXEL_KEYS:
            w = torch.ones(ref[k].shape[:3], dtype=torch.bool)
            w[0, 0, M.BAD_PIXEL] = False
            where[k] = w[..., None].expand_as(ref[k])
        else:
            fed = torch.zeros(ref[k].numel() // 3, dtype=torch.bool)
            for fw in (f, fb):
                rows = fw.quads[k][M.BAD_PIXEL]
                fed[rows[rows >= 0]] = True
            where[k] = ~fed.reshape(ref[k].shape[:3])[..., None].expand_as(ref[k])
        assert bool(torch.isfinite(ref[k][where[k]]).all()) and bool(where[k].any())
    assert any(bool(torch.isnan(ref[k]).any()) for k in ref)
    runs = [_run(case, False), _run(case, True)]
    for got in runs:
        for k, g in got.items():
            assert torch.equal(torch.isnan(g), torch.isnan(ref[k])) and torch.equal(torch.isnan(g), torch.isnan(x32[k])), k
            assert not bool(torch.isinf(g).any()), k
        assert not _check(name, got, ref, mag)
        assert not _check(name + " (against the benign frame)", got, ben_ref, ben_mag, where, figure_of=name)
    for k in ("values",) + M.PIXEL_KEYS:
        assert _same_bits(runs[0][k], runs[1][k]), k
