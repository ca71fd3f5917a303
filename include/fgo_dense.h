/*
 * fgo_dense.h — dense, feature-free registration of key-frame pairs on the device: projective point-to-plane ICP on the depth
 * frames themselves.
 *
 * When the feature registration of a pair fails the reference has nothing to offer the graph: the g2o path adds fakeOdoNode's
 * identity edge with information 1e-3 I (g2o/g2o_graph.cpp:136-157, gtsam/gtsam_graph.cpp:697-722), the offline path writes
 * makeItVoid's record (information 10000 on the diagonal, gtsam/test/convert_vo2ba.cpp:424-436), which both checks then skip, and
 * add_vo_at_sparse_area.cpp repairs such records after the fact.  fgo_vro_ransac_batch reproduces the void record faithfully and
 * fgo_plane_propagate_batch bridges the gap only where an IMU pose exists.  The call below aligns the two DEPTH FRAMES of a pair and
 * returns exactly what the RANSAC returns -- pose_ij7 and info_ut21 -- so that a failed record can go on to the two checks, the
 * Mahalanobis gate and fgo_add_edge_se3 without a host loop.  An ICP is not part of the reference tree: the semantics below are
 * THIS PROJECT'S DEFINITION, pinned to the numpy restatement tests/depth_align_reference.py, itself pinned to a per-pixel brute
 * force by tests/test_depth_align_reference_cpu.py.
 *
 * Conventions: those of fgo_vro_ransac_batch.  p_i = R p_j + t, stored t(3) q_xyzw(4) with w >= 0; the tangent is [omega; v], the
 * perturbation T Exp(xi); info_ut21 is the upper triangle by rows, as fgo_add_edge_se3(..., FGO_TANGENT_GTSAM) takes it.  Frame i
 * is the TARGET (its depth is looked up), frame j the SOURCE (its pixels are moved).
 *
 * Arithmetic: f64; every product, quotient, sum and square root is rounded on its own (no contraction), sums of three terms are
 * (a + b) + c.  The stages:
 *   point       pixel (u, v) with the depth word d:  z = (double) d * z_scale, valid iff z_min < z < z_max (fgo_map_fuse_batch's
 *               test; a word 0 is never valid since z_min >= 0);  P = (((u - cx) * z) / fx, ((v - cy) * z) / fy, z).
 *   normal      of the TARGET at (u, v), s = normal_step: the centre and the four neighbours (u +- s, v), (u, v +- s) lie inside
 *               the image and are valid, and every neighbour's z is within normal_jump of the centre's (|dz| <= normal_jump).
 *               a = P(u + s, v) - P(u - s, v), b = P(u, v + s) - P(u, v - s), c = a x b, l = sqrt((c0^2 + c1^2) + c2^2); invalid
 *               unless l > 0; n = c / l, negated if n . P > 0 (the normal faces the camera).
 *   noise       sigma^2(n, P) = n^T Sigma(P) n with the pixel + depth model of fgo_vro_ransac_batch, in closed form:
 *               sigma_px^2 * (gx^2 + gy^2) + sz^2 * nr^2,  gx = (n0 * z) / fx, gy = (n1 * z) / fy, nr = (n0 * (x / z) + n1 * (y / z)) + n2,
 *               sz = sigma_z[0] + z * (sigma_z[1] + z * sigma_z[2]).
 *   evaluation  at the pose (q, t), R = the rotation matrix of q, on a level of stride k: every source pixel with u % k == 0 and
 *               v % k == 0 whose point p_j is valid, in pixel order (rows, then columns):
 *                 q_c = ((R[c][0] x + R[c][1] y) + R[c][2] z) + t_c;                     rejected unless q_2 > 0
 *                 u' = rint((fx * q_0) / q_2 + cx), v' = rint((fy * q_1) / q_2 + cy)     (ties to even); rejected outside the image
 *                 the target point p_i and normal n at (u', v');                         rejected if either is invalid
 *                 e = q - p_i;   rejected if sqrt((e0^2 + e1^2) + e2^2) > max_dist
 *                 rejected if |n . q| < min_cos * sqrt((q0^2 + q1^2) + q2^2)             (the surface is seen at a grazing angle)
 *               Otherwise, with m = R^T n:  r = n . e,  J = [p_j x m; m]  (= n^T [-R [p_j]x, R]),
 *               w = 1 / (sigma^2(n, p_i) + sigma^2(m, p_j)),  and with Jw = w J:
 *                 H += Jw J^T (upper triangle),  g += Jw r,  chi2 += (w r) r,  ss += r r,  count += 1.
 *   solve       a sum that is not finite: FGO_DA_NUM.  count < min_pairs: FGO_DA_TOO_FEW.  A diagonal entry of H that is not
 *               positive: FGO_DA_DEGENERATE with min_pivot 0.  s_k = 1 / sqrt(H_kk); Hs = ((H_rc s_r) s_c); Hs = L L^T by rows
 *               (d_j = Hs_jj - sum_k L_jk^2, one subtraction after the other); min_pivot = min_j d_j; min_pivot < the parameter
 *               min_pivot (or NaN): FGO_DA_DEGENERATE.  M = L^-1; delta = s * (M^T (M (s * g))).
 *   iteration   the levels l = 0 .. n_levels - 1 in this order (coarse to fine) with the stride skip[l]: at most iters[l] times
 *               evaluate, solve, T <- normalise(T Exp(-delta)) (Pose3's full exponential map); the level ends early after a step
 *               with |delta_omega| < eps_rot and |delta_v| < eps_trans.  iterations counts the steps of all levels, converged says
 *               that the LAST level ended early.
 *   result      one more evaluation and solve at the final pose with the stride of the last level: info = H (the Fisher
 *               information of the pose under the noise model), cov36 = ((M^T M)_rc s_r) s_c mirrored (exactly symmetric),
 *               rmse = sqrt(ss / count), chi2, n_pairs_used = count, min_pivot.  iters = {0} makes this the evaluation at the
 *               initial pose.
 *   failure     any status but FGO_DA_OK gives makeItVoid's record, as fgo_vro_ransac_batch does: pose identity, information
 *               10000 on the diagonal, covariance zero; n_pairs_used is the count of the evaluation that failed, iterations the
 *               steps done before it, rmse = chi2 = 0.
 * Reproducibility: a lane sums its own pixels in pixel order, the lanes of a wave are merged by a fixed butterfly and the waves in
 * wave order: no atomics, two calls are bit-identical, a pair's outputs do not depend on the rest of the batch, and the two kernel
 * forms give the same bits.  Stateless, host arrays in and out; FGO_ENODEV without a HIP device (no CPU fallback).
 */
#ifndef FGO_DENSE_H
#define FGO_DENSE_H
#include "fgo.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FGO_DA_OK 0
#define FGO_DA_TOO_FEW 1      /* fewer than min_pairs associations in an evaluation */
#define FGO_DA_DEGENERATE 2   /* the normal equations do not fix all six degrees of freedom */
#define FGO_DA_NUM 3          /* a sum is not finite */
#define FGO_DA_MAX_LEVELS 3
#define FGO_DA_MAX_PIXELS 16777216   /* width * height of one frame */

typedef struct {
  double fx, fy, cx, cy, z_scale, z_min, z_max;   /* as fgo_map_params: 250.5773 250.5773 90 70 0.001 0.1 5.0 */
  double sigma_px, sigma_z[3];                    /* as fgo_vro_params: 1.0, {0.014, 0, 0} */
  int n_levels;                                   /* 3 (1 .. FGO_DA_MAX_LEVELS) */
  int skip[3];                                    /* {4, 2, 2} */
  int iters[3];                                   /* {10, 10, 5} */
  int normal_step;                                /* 2 pixels */
  double normal_jump;                             /* 0.05 m */
  double max_dist;                                /* 0.10 m */
  double min_cos;                                 /* cos 80 deg */
  int min_pairs;                                  /* 500 */
  double eps_rot, eps_trans;                      /* 1e-6 rad, 1e-6 m */
  double min_pivot;                               /* 1e-6 */
} fgo_depth_align_params;
void fgo_depth_align_params_default(fgo_depth_align_params *p);   /* NULL tolerated */

typedef struct {
  int status;         /* FGO_DA_* */
  int n_pairs_used;
  int iterations;
  int converged;
  double rmse;
  double chi2;
  double min_pivot;   /* the smallest pivot of the scaled normal matrix in the last solve */
} fgo_depth_align_result;

/* All pairs in one launch, one workgroup per pair.  depth holds n_frames frames of height x width words, rows first; pair p aligns
 * frame_j[p] to frame_i[p] starting from pose_ij7_init[p] (normalised; NULL: the identity for every pair).  normal_eq_out, for tests
 * and diagnosis: per pair the 28 numbers H (upper 21), g (6), chi2 of the FIRST evaluation (every pair makes at least one).
 * FGO_EINVAL (before any HIP call): n_frames, n_pairs < 0; width, height < 1 or width * height > FGO_DA_MAX_PIXELS; fx, fy, z_scale
 * not positive and finite, cx, cy not finite; not 0 <= z_min < z_max; sigma_px <= 0; a negative sigma_z or all three zero; n_levels
 * outside [1, 3]; for a level in use skip < 1 or iters outside [0, 100]; normal_step outside [1, 64]; normal_jump <= 0;
 * max_dist <= 0; min_cos outside [0, 1]; min_pairs < 6; eps_rot, eps_trans < 0; min_pivot outside [0, 1) (NaN refused everywhere);
 * and with n_pairs > 0: a NULL depth, frame_i, frame_j, pose_ij7_out or result; a frame index outside [0, n_frames); an initial
 * quaternion that cannot be normalised or a translation that is not finite.  n_pairs == 0: FGO_OK, nothing is read or written. */
int fgo_depth_align_batch(int device, int64_t n_frames, int width, int height, const uint16_t *depth /* n_frames x H x W */,
                          int64_t n_pairs, const int64_t *frame_i, const int64_t *frame_j,
                          const double *pose_ij7_init /* n_pairs x 7, NULL = identity */,
                          const fgo_depth_align_params *params /* NULL = defaults */,
                          double *pose_ij7_out, double *info_ut21_out /* may be NULL */, double *cov36_out /* may be NULL */,
                          double *normal_eq_out /* n_pairs x 28, may be NULL: tests */, fgo_depth_align_result *result /* n_pairs */);
/* development: the kernel time of the last call by HIP events, ms; and the kernel form: 0 the default (the target frame's depth
 * words staged in LDS when a frame fits, 60 KB), 1 LDS (the same rule), 2 global memory always; returns the value in force */
double fgo_debug_depth_align_kernel_ms(void);
int fgo_debug_depth_align_form(int form);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FGO_DENSE_H */
