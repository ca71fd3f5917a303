// Batched two-view bundle adjustment on the MI355X (gfx950, f64): what CGraphGT::bundleAdjust builds and solves for ONE
// visual-odometry record (gtsam/gtsam_graph.cpp:500-610) -- two Pose3 (PriorFactor sigma 1e-7 on the first, :537), one Point3
// per match with a PriorFactor<Point3> (:574) and two GenericProjectionFactor<Pose3, Point3, Cal3DS2> (:539) --
// LevenbergMarquardtOptimizer::optimize(), then Marginals::marginalCovariance of the second pose and its inverse as the
// edge's information.  The reference's offline tools run it record after record (gtsam/test/convert_vo2ba.cpp:210-243); the
// records are independent, so fgo_two_view_ba_batch runs ONE WAVE PER PAIR and the whole LM run of a pair inside one launch.
//
// A pair has 12 + 3 N unknowns.  Per LM trial:
//   reduce   lanes stride the pair's points; a lane linearises its point (dev::reproj_factor<true> twice + the point prior),
//            factors H_pp + lambda I (3x3) and stages  Y = [W_i; W_j] L_pp^-T (12x3),  y = L_pp^-1 b_p  and the whitened pose
//            Jacobians / residuals in LDS, 64 points at a time.  The 78 + 12 entries of the reduced system
//              S = H_cc - sum_p Y_p Y_p^T,   g = b_c - sum_p Y_p y_p
//            are owned by lanes (one or two each); a lane sums its entries over the staged points in point order -- a fixed
//            order that depends on nothing but the pair, no floating-point atomics, two or three running sums per lane
//            instead of 90.
//   solve    every lane holds the 12x12 system (+ pose i's prior, + lambda I), factors and solves it redundantly: the step of
//            the poses is wave-uniform without a broadcast.
//   trial    lanes stride their points again: d_p = (H_pp + lambda I)^-1 (b_p - W^T d_c), the candidate point goes to the
//            work buffer, its two residuals are evaluated at the candidate poses; chi2' and d.(lambda d + b) are summed over
//            the wave by a butterfly whose result is bit-identical in every lane, so the accept / reject decision is uniform.
// The controller is the one of fgo_optimize_gtsam (csrc/fgo_lm.cpp).  After it stops, one more reduce pass with lambda = 0 gives
// the factor of the undamped reduced system; pose j is eliminated last, so the trailing 6x6 block L_jj of the factor carries
// its marginal:  information = L_jj L_jj^T,  covariance = L_jj^-T L_jj^-1.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include <cmath>
#include "../../include/fgo.h"
#include "device_plan.hpp"
#include "factors_device.hpp"
#include "small_dense_device.hpp"
#include "batch_call.hpp"

namespace fgo {
using namespace dev;

namespace {

constexpr int TV_LD = 65;       // staged rows hold 64 points + 1 double of padding: lanes that read different rows at one point hit different banks
constexpr int TV_ROWS = 39;     // round 1: pose Jacobians (24 rows) + residuals (4); round 2: Y (36) + y (3)
constexpr int TV_MAX_MATCHES = INT_MAX / 3;   // of one pair: the kernel indexes its points with int (3 k + 2)
constexpr int TV_SYS = 0, TV_RHS = 144, TV_GRAD = 156;   // after a reduce pass the staging area holds S (12x12), g (12), b_c (12)

// the call's constants: one record in device memory, read through a pointer
struct TvConst {
  CamCalib K;
  double w_pose, w_pt, s_pix;   // 1 / sigma^2 of the pose and point priors, 1 / sigma of a pixel
  int max_iters, min_matches;
};

// one match, whitened: the two projection factors and the point prior
struct PtLin {
  double A[12][2];     // rows 0-5: columns of (J_xi / sigma)^T, rows 6-11: of (J_xj / sigma)^T
  double P[4][3];      // rows 0-1: J_p / sigma of the factor on pose i, rows 2-3: on pose j
  double r[4];         // residuals / sigma
  double h[6], g[3];   // H_pp (upper triangle) and b_p, prior included
  double chi;
};

__device__ __forceinline__ void lin_point(const TvConst &C, const Pose &Xi, const Pose &Xj, V3 pt, V3 mean, const double *__restrict__ zi,
                                          const double *__restrict__ zj, PtLin &L) {
  double e[6];
  M6 Jx, Jp;
  reproj_factor<true>(Xi, pt, zi[0], zi[1], C.K, e, Jx, Jp);
#pragma unroll
  for (int c = 0; c < 6; ++c) { L.A[c][0] = C.s_pix * Jx.m[c]; L.A[c][1] = C.s_pix * Jx.m[6 + c]; }
#pragma unroll
  for (int c = 0; c < 3; ++c) { L.P[0][c] = C.s_pix * Jp.m[c]; L.P[1][c] = C.s_pix * Jp.m[6 + c]; }
  L.r[0] = C.s_pix * e[0]; L.r[1] = C.s_pix * e[1];
  reproj_factor<true>(Xj, pt, zj[0], zj[1], C.K, e, Jx, Jp);
#pragma unroll
  for (int c = 0; c < 6; ++c) { L.A[6 + c][0] = C.s_pix * Jx.m[c]; L.A[6 + c][1] = C.s_pix * Jx.m[6 + c]; }
#pragma unroll
  for (int c = 0; c < 3; ++c) { L.P[2][c] = C.s_pix * Jp.m[c]; L.P[3][c] = C.s_pix * Jp.m[6 + c]; }
  L.r[2] = C.s_pix * e[0]; L.r[3] = C.s_pix * e[1];
  const double d[3] = {pt.x - mean.x, pt.y - mean.y, pt.z - mean.z};
  int q = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) {
      double s = a == b ? C.w_pt : 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) s += L.P[k][a] * L.P[k][b];
      L.h[q++] = s;
    }
  double chi = C.w_pt * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
  for (int k = 0; k < 4; ++k) chi += L.r[k] * L.r[k];
  L.chi = chi;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double s = C.w_pt * d[a];
#pragma unroll
    for (int k = 0; k < 4; ++k) s += L.P[k][a] * L.r[k];
    L.g[a] = -s;
  }
}

// M = chol(H_pp + lambda I)^-1 (lower); false when a pivot is not positive
struct PtInv { double m00, m10, m11, m20, m21, m22; };
__device__ __forceinline__ bool pt_factor(const double h[6], double lambda, PtInv &M) {
  const double h00 = h[0] + lambda, h01 = h[1], h02 = h[2], h11 = h[3] + lambda, h12 = h[4], h22 = h[5] + lambda;
  bool ok = h00 > 0;
  const double l00 = sqrt(h00), i00 = 1.0 / l00;
  const double l10 = h01 * i00, l20 = h02 * i00;
  const double d11 = h11 - l10 * l10;
  ok = ok && d11 > 0;
  const double l11 = sqrt(d11), i11 = 1.0 / l11;
  const double l21 = (h12 - l20 * l10) * i11;
  const double d22 = h22 - l20 * l20 - l21 * l21;
  ok = ok && d22 > 0;
  const double i22 = 1.0 / sqrt(d22);
  M.m00 = i00; M.m10 = -l10 * i00 * i11; M.m11 = i11;
  M.m20 = -(l20 * M.m00 + l21 * M.m10) * i22; M.m21 = -l21 * M.m11 * i22; M.m22 = i22;
  return ok;
}

// what one entry of the reduced system sums: rows a2 / b2 of the staged Jacobians (2 consecutive rows each) with sign s2 (0: none),
// rows a1 / b1 of the staged Y (3 consecutive rows each)
struct TvOut { int a1, b1, a2, b2; double s2; };
__device__ __forceinline__ TvOut tv_out(int idx) {
  TvOut o = {0, 0, 0, 0, 0.0};
  if (idx < 78) {                                  // S(r, c), r <= c, row-major upper triangle
    int r = 0, left = idx;
    while (left >= 12 - r) { left -= 12 - r; ++r; }
    const int c = r + left;
    o.a1 = 3 * r; o.b1 = 3 * c; o.a2 = 2 * r; o.b2 = 2 * c;
    o.s2 = ((r < 6) == (c < 6)) ? 1.0 : 0.0;       // H_cc is block-diagonal per pose
  } else if (idx < 90) {                           // g(r) = b_c(r) - sum Y y,  b_c(r) = -sum A r
    const int r = idx - 78;
    o.a1 = 3 * r; o.b1 = 36; o.a2 = 2 * r; o.b2 = 24 + (r < 6 ? 0 : 2);
    o.s2 = -1.0;
  }
  return o;
}

// One linearisation of the pair at (Xi, Xj, pts) reduced onto the poses with damping lambda.  Leaves S (full, symmetric) at
// sm[TV_SYS], g at sm[TV_RHS] and the unreduced pose gradient b_c at sm[TV_GRAD] (the caller adds pose i's prior); returns
// the points' part of chi2 and whether a landmark block failed to factor.
__device__ __forceinline__ void tv_reduce(const TvConst *Cg, const Pose &Xi, const Pose &Xj, double lambda, int n, const double *__restrict__ pts,
                                          const double *__restrict__ mean, const double *__restrict__ zi, const double *__restrict__ zj,
                                          double *sm, int lane, double &chi_out, bool &fail_out) {
  const TvOut o0 = tv_out(lane), o1 = tv_out(64 + lane);
  double acc0 = 0, acc1 = 0, grad = 0, chi = 0;
  bool bad = false;
  for (int blk = 0; blk < n; blk += 64) {
    const int cnt = min(64, n - blk), k = blk + lane;
    double PM[4][3], y[3];                         // J_p M^T of the four residual rows, M b_p
    __syncthreads();                               // the readers of the previous contents are done
    if (k < n) {
      PtLin L;
      lin_point(*Cg, Xi, Xj, V3{pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]}, V3{mean[3 * k], mean[3 * k + 1], mean[3 * k + 2]}, zi + 2 * k, zj + 2 * k, L);
      chi += L.chi;
#pragma unroll
      for (int r = 0; r < 12; ++r) { sm[(2 * r) * TV_LD + lane] = L.A[r][0]; sm[(2 * r + 1) * TV_LD + lane] = L.A[r][1]; }
#pragma unroll
      for (int q = 0; q < 4; ++q) sm[(24 + q) * TV_LD + lane] = L.r[q];
      PtInv M;
      bad = bad || !pt_factor(L.h, lambda, M);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        PM[q][0] = L.P[q][0] * M.m00;
        PM[q][1] = L.P[q][0] * M.m10 + L.P[q][1] * M.m11;
        PM[q][2] = L.P[q][0] * M.m20 + L.P[q][1] * M.m21 + L.P[q][2] * M.m22;
      }
      y[0] = M.m00 * L.g[0];
      y[1] = M.m10 * L.g[0] + M.m11 * L.g[1];
      y[2] = M.m20 * L.g[0] + M.m21 * L.g[1] + M.m22 * L.g[2];
    }
    __syncthreads();
    // round 1: the pose Jacobians and residuals -> H_cc, b_c
#pragma unroll 2
    for (int q = 0; q < cnt; ++q) {
      double v0 = 0, v1 = 0;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        v0 += sm[(o0.a2 + c) * TV_LD + q] * sm[(o0.b2 + c) * TV_LD + q];
        v1 += sm[(o1.a2 + c) * TV_LD + q] * sm[(o1.b2 + c) * TV_LD + q];
      }
      if (o0.s2 != 0.0) acc0 += o0.s2 * v0;
      if (o1.s2 != 0.0) acc1 += o1.s2 * v1;
      if (o1.s2 < 0.0) grad -= v1;                 // (the right-hand sides are entries 78 .. 89: second slots of lanes 14 .. 25)
    }
    // round 2: a lane takes its Jacobians back (they need not stay in registers through round 1) and stages Y = [W_i; W_j] L_pp^-T, y
    double A[12][2];
    if (k < n) {
#pragma unroll
      for (int r = 0; r < 12; ++r) { A[r][0] = sm[(2 * r) * TV_LD + lane]; A[r][1] = sm[(2 * r + 1) * TV_LD + lane]; }
    }
    __syncthreads();
    if (k < n) {
#pragma unroll
      for (int r = 0; r < 12; ++r) {
        const int q = r < 6 ? 0 : 2;
#pragma unroll
        for (int c = 0; c < 3; ++c) sm[(3 * r + c) * TV_LD + lane] = A[r][0] * PM[q][c] + A[r][1] * PM[q + 1][c];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) sm[(36 + c) * TV_LD + lane] = y[c];
    }
    __syncthreads();
#pragma unroll 2
    for (int q = 0; q < cnt; ++q) {
      double v0 = 0, v1 = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v0 += sm[(o0.a1 + c) * TV_LD + q] * sm[(o0.b1 + c) * TV_LD + q];
        v1 += sm[(o1.a1 + c) * TV_LD + q] * sm[(o1.b1 + c) * TV_LD + q];
      }
      acc0 -= v0; acc1 -= v1;
    }
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int idx = lane + 64 * h;
    const double v = h ? acc1 : acc0;
    if (idx < 78) {
      int r = 0, left = idx;
      while (left >= 12 - r) { left -= 12 - r; ++r; }
      const int c = r + left;
      sm[TV_SYS + r * 12 + c] = v; sm[TV_SYS + c * 12 + r] = v;
    } else if (idx < 90) {
      sm[TV_RHS + idx - 78] = v; sm[TV_GRAD + idx - 78] = grad;
    }
  }
  __syncthreads();
  chi_out = wave_sum(chi);
  fail_out = __ballot(bad) != 0;
}

// the candidate of every point for the pose step d (12), and what the LM controller needs: chi2 of the points' factors at the
// candidate and the points' part of d.(lambda d + b).  Lanes own the same points as in tv_reduce, so a lane reads back only
// what it wrote itself.
__device__ __forceinline__ void tv_trial(const TvConst *Cg, const Pose &Xi, const Pose &Xj, const Pose &Yi, const Pose &Yj, const double d[12],
                                         double lambda, int n, const double *__restrict__ pts, double *__restrict__ cand,
                                         const double *__restrict__ mean, const double *__restrict__ zi, const double *__restrict__ zj, int lane,
                                         double &chi_out, double &scale_out) {
  double chi = 0, sc = 0;
  for (int k = lane; k < n; k += 64) {
    const V3 pt = {pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]}, mu = {mean[3 * k], mean[3 * k + 1], mean[3 * k + 2]};
    PtLin L;
    lin_point(*Cg, Xi, Xj, pt, mu, zi + 2 * k, zj + 2 * k, L);
    PtInv M;
    (void)pt_factor(L.h, lambda, M);                // (it factored in the reduce pass of this trial)
    double Ad[4] = {0, 0, 0, 0};                    // J_x d of the two factors
#pragma unroll
    for (int r = 0; r < 6; ++r) { Ad[0] += L.A[r][0] * d[r]; Ad[1] += L.A[r][1] * d[r]; Ad[2] += L.A[6 + r][0] * d[6 + r]; Ad[3] += L.A[6 + r][1] * d[6 + r]; }
    double t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = L.g[c] - (L.P[0][c] * Ad[0] + L.P[1][c] * Ad[1] + L.P[2][c] * Ad[2] + L.P[3][c] * Ad[3]);
    const double u0 = M.m00 * t[0], u1 = M.m10 * t[0] + M.m11 * t[1], u2 = M.m20 * t[0] + M.m21 * t[1] + M.m22 * t[2];
    const double dp[3] = {M.m00 * u0 + M.m10 * u1 + M.m20 * u2, M.m11 * u1 + M.m21 * u2, M.m22 * u2};
#pragma unroll
    for (int c = 0; c < 3; ++c) sc += dp[c] * (lambda * dp[c] + L.g[c]);
    const V3 pc = {pt.x + dp[0], pt.y + dp[1], pt.z + dp[2]};
    cand[3 * k] = pc.x; cand[3 * k + 1] = pc.y; cand[3 * k + 2] = pc.z;
    const TvConst &C = *Cg;
    double e[6];
    M6 J0, J1;
    reproj_factor<false>(Yi, pc, zi[2 * k], zi[2 * k + 1], C.K, e, J0, J1);
    chi += (C.s_pix * e[0]) * (C.s_pix * e[0]) + (C.s_pix * e[1]) * (C.s_pix * e[1]);
    reproj_factor<false>(Yj, pc, zj[2 * k], zj[2 * k + 1], C.K, e, J0, J1);
    chi += (C.s_pix * e[0]) * (C.s_pix * e[0]) + (C.s_pix * e[1]) * (C.s_pix * e[1]);
    const double q0 = pc.x - mu.x, q1 = pc.y - mu.y, q2 = pc.z - mu.z;
    chi += C.w_pt * (q0 * q0 + q1 * q1 + q2 * q2);
  }
  chi_out = wave_sum(chi);
  scale_out = wave_sum(sc);
}

// in place: the lower Cholesky factor of the symmetric 12x12 whose lower triangle a holds, packed by rows (lt)
__device__ __forceinline__ bool chol12(double a[78]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    double d = a[lt(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= a[lt(j, k)] * a[lt(j, k)];
    ok = ok && d > 0;
    const double l = sqrt(d), il = 1.0 / l;
    a[lt(j, j)] = l;
#pragma unroll
    for (int i = j + 1; i < 12; ++i) {
      double s = a[lt(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= a[lt(i, k)] * a[lt(j, k)];
      a[lt(i, j)] = s * il;
    }
  }
  return ok;
}

__device__ __forceinline__ Pose load_pose7(const double *__restrict__ p) { return {{p[0], p[1], p[2]}, {p[3], p[4], p[5], p[6]}}; }
__device__ __forceinline__ void store_pose7(double *__restrict__ p, const Pose &X) {
  p[0] = X.t.x; p[1] = X.t.y; p[2] = X.t.z; p[3] = X.q.x; p[4] = X.q.y; p[5] = X.q.z; p[6] = X.q.w;
}

__global__ __launch_bounds__(64) void k_two_view(int64_t n_pairs, const int64_t *__restrict__ match_ptr, const double *__restrict__ xyz,
                                                 const double *__restrict__ uv_i, const double *__restrict__ uv_j,
                                                 const double *__restrict__ pose_j0, const TvConst *__restrict__ Cg, double *__restrict__ work, int64_t n_matches,
                                                 double *__restrict__ pose_j_out, double *__restrict__ pose_i_out, double *__restrict__ cov_out,
                                                 double *__restrict__ info_out, fgo_two_view_result *__restrict__ res) {
  __shared__ double sm[TV_ROWS * TV_LD];
  const int64_t p = blockIdx.x;
  if (p >= n_pairs) return;
  const int lane = threadIdx.x;
  const int64_t m0 = match_ptr[p];
  const int n = (int)(match_ptr[p + 1] - m0);
  const Pose ident = {{0, 0, 0}, {0, 0, 0, 1}};
  Pose Xi = ident, Xj = pose_j0 ? load_pose7(pose_j0 + 7 * p) : ident;
  if (lane == 0) {                                    // zero unless the pair ends with FGO_TV_OK
    if (cov_out) for (int k = 0; k < 36; ++k) cov_out[36 * p + k] = 0;
    if (info_out) for (int k = 0; k < 21; ++k) info_out[21 * p + k] = 0;
  }
  fgo_two_view_result R;
  R.status = FGO_TV_TOO_FEW; R.iterations = 0; R.trials = 0; R.error_initial = 0; R.error_final = 0; R.lambda_final = 0;

  if (n >= Cg->min_matches) {
    const double *mean = xyz + 3 * m0, *zi = uv_i + 2 * m0, *zj = uv_j + 2 * m0;
    double *cur = work + 3 * m0, *cand = work + 3 * (n_matches + m0);
    for (int k = lane; k < n; k += 64) { cur[3 * k] = mean[3 * k]; cur[3 * k + 1] = mean[3 * k + 1]; cur[3 * k + 2] = mean[3 * k + 2]; }

    // LevenbergMarquardtOptimizer with GTSAM 4.0's defaults, as fgo_optimize_gtsam drives it
    const double lambdaFactor = 10.0, lambdaUpper = 1e5, minModelFidelity = 1e-3, relTol = 1e-5, absTol = 1e-5;
    double lambda = 1e-5, currentError = 0, errorBefore = 0;
    int iterations = 0, trials = 0;
    bool finishing = false;
    for (;;) {
      const double lam = finishing ? 0.0 : lambda;
      double chi_lin;
      bool failed;
      tv_reduce(Cg, Xi, Xj, lam, n, cur, mean, zi, zj, sm, lane, chi_lin, failed);
      // pose i's prior, PriorFactor<Pose3>(identity): every lane evaluates it, lane 0 adds it to the staged system -- the 12x12
      // factorisation below needs the registers
      {
        const double w_pose = Cg->w_pose;
        double pe[6];
        M6 PJ;
        prior_pose3<true>(Xi, ident, pe, PJ);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          chi_lin += w_pose * pe[r] * pe[r];
          double g = 0;
#pragma unroll
          for (int k = 0; k < 6; ++k) g += PJ.m[k * 6 + r] * pe[k];
          if (lane == 0) { sm[TV_RHS + r] -= w_pose * g; sm[TV_GRAD + r] -= w_pose * g; }
#pragma unroll
          for (int c = 0; c <= r; ++c) {
            double h = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k) h += PJ.m[k * 6 + r] * PJ.m[k * 6 + c];
            if (lane == 0) sm[TV_SYS + r * 12 + c] += w_pose * h;     // (the lower triangle is what is read below)
          }
        }
      }
      __syncthreads();
      double a[78];
#pragma unroll
      for (int r = 0; r < 12; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) a[lt(r, c)] = sm[TV_SYS + r * 12 + c];
      if (trials == 0 && !finishing) { currentError = 0.5 * chi_lin; R.error_initial = currentError; errorBefore = currentError; }
#pragma unroll
      for (int r = 0; r < 12; ++r) a[lt(r, r)] += lam;
      failed = !chol12(a) || failed;
      if (finishing) {
        R.status = (failed || !isfinite(currentError)) ? FGO_TV_NUM : FGO_TV_OK;
        if (R.status == FGO_TV_OK) {
          // L_jj = rows / columns 6 .. 11 of the factor: information = L_jj L_jj^T, covariance = L_jj^-T L_jj^-1 (the last two
          // steps of dev::inv6, kept here: see small_dense_device.hpp)
          double Mi[21];                              // L_jj^-1, lower, packed by rows
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            Mi[lt(c, c)] = 1.0 / a[lt(6 + c, 6 + c)];
#pragma unroll
            for (int r = c + 1; r < 6; ++r) {
              double s = 0;
#pragma unroll
              for (int k = c; k < r; ++k) s += a[lt(6 + r, 6 + k)] * Mi[lt(k, c)];
              Mi[lt(r, c)] = -s / a[lt(6 + r, 6 + r)];
            }
          }
          int q = 0;
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) {
              double s = 0, t = 0;
#pragma unroll
              for (int k = c; k < 6; ++k) s += Mi[lt(k, r)] * Mi[lt(k, c)];
#pragma unroll
              for (int k = 0; k <= r; ++k) t += a[lt(6 + r, 6 + k)] * a[lt(6 + c, 6 + k)];
              if (lane == 0 && cov_out) { cov_out[36 * p + r * 6 + c] = s; cov_out[36 * p + c * 6 + r] = s; }
              if (lane == 0 && info_out) info_out[21 * p + q] = t;
              ++q;
            }
        }
        R.iterations = iterations; R.trials = trials; R.error_final = currentError; R.lambda_final = lambda;
        break;
      }
      ++trials;
      bool step_ok = false, stop_search = false;
      double newError = currentError;
      Pose Yi = Xi, Yj = Xj;
      if (!failed) {
        double d[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) {                 // forward, then backward substitution
          double s = sm[TV_RHS + i];
#pragma unroll
          for (int k = 0; k < i; ++k) s -= a[lt(i, k)] * d[k];
          d[i] = s / a[lt(i, i)];
        }
#pragma unroll
        for (int i = 11; i >= 0; --i) {
          double s = d[i];
#pragma unroll
          for (int k = i + 1; k < 12; ++k) s -= a[lt(k, i)] * d[k];
          d[i] = s / a[lt(i, i)];
        }
        Yi = retract_pose3(Xi, d);
        Yj = retract_pose3(Xj, d + 6);
        double chi_cand, scale;
        tv_trial(Cg, Xi, Xj, Yi, Yj, d, lam, n, cur, cand, mean, zi, zj, lane, chi_cand, scale);
#pragma unroll
        for (int i = 0; i < 12; ++i) scale += d[i] * (lam * d[i] + sm[TV_GRAD + i]);
        double pe[6];
        M6 unused;
        prior_pose3<false>(Yi, ident, pe, unused);
#pragma unroll
        for (int r = 0; r < 6; ++r) chi_cand += Cg->w_pose * pe[r] * pe[r];
        if (isfinite(chi_cand)) {
          newError = 0.5 * chi_cand;
          const double linearizedCostChange = 0.5 * scale;    // b'd - d'Hd / 2 from the damped solve (csrc/fgo_lm.cpp)
          if (linearizedCostChange >= 0) {
            const double costChange = currentError - newError;
            if (linearizedCostChange > 1e-20 && costChange / linearizedCostChange > minModelFidelity) step_ok = true;
            if (fabs(costChange) < relTol * currentError) stop_search = true;
          }
        }
      }
      bool iteration_done = false;
      if (step_ok) {
        currentError = newError;
        Xi = Yi; Xj = Yj;
        double *t = cur; cur = cand; cand = t;
        lambda = fmax(0.0, lambda / lambdaFactor);
        iteration_done = true;
      } else if (stop_search) {
        iteration_done = true;
      } else {
        lambda *= lambdaFactor;
        if (lambda >= lambdaUpper) iteration_done = true;
      }
      if (iteration_done) {
        ++iterations;
        bool end = iterations >= Cg->max_iters || !isfinite(currentError) || currentError <= 0.0;
        if (!end) {
          const double absDec = errorBefore - currentError, relDec = absDec / errorBefore;
          end = relDec <= relTol || absDec <= absTol;
        }
        if (end) finishing = true;
        errorBefore = currentError;
      }
    }
  }
  if (lane == 0) {
    store_pose7(pose_j_out + 7 * p, Xj);
    if (pose_i_out) store_pose7(pose_i_out + 7 * p, Xi);
    res[p] = R;
  }
}

}  // namespace
}  // namespace fgo

extern "C" void fgo_two_view_params_default(fgo_two_view_params *p) {
  if (!p) return;
  p->pose_prior_sigma = 1e-7;
  p->point_sigma = 0.014;
  p->pixel_sigma = 1.0;
  p->max_iters = 100;
  p->min_matches = 5;
}

extern "C" int fgo_two_view_ba_batch(int device, int64_t n_pairs, const int64_t *match_ptr, const double *xyz_i, const double *uv_i,
                                     const double *uv_j, const double *pose_j0, const double calib9[9], const double body_P_sensor7[7],
                                     const fgo_two_view_params *params, double *pose_j_out, double *pose_i_out, double *cov36_out,
                                     double *info_ut21_out, fgo_two_view_result *result) {
  using namespace fgo;
  fgo_two_view_params P;
  fgo_two_view_params_default(&P);
  if (params) P = *params;
  if (n_pairs < 0 || n_pairs > INT_MAX || !(P.pose_prior_sigma > 0) || !(P.point_sigma > 0) || !(P.pixel_sigma > 0) || P.min_matches < 3) return FGO_EINVAL;
  if (n_pairs == 0) return FGO_OK;
  if (!match_ptr || !calib9 || !pose_j_out || !result || !csr_ptr_ok(match_ptr, n_pairs, TV_MAX_MATCHES)) return FGO_EINVAL;
  const int64_t M = match_ptr[n_pairs];
  if (M > 0 && (!xyz_i || !uv_i || !uv_j)) return FGO_EINVAL;
  TvConst C;
  if (!cam_calib_make(C.K, calib9, body_P_sensor7)) return FGO_EINVAL;       // zero quaternion
  C.w_pose = 1.0 / (P.pose_prior_sigma * P.pose_prior_sigma);
  C.w_pt = 1.0 / (P.point_sigma * P.point_sigma);
  C.s_pix = 1.0 / P.pixel_sigma;
  C.max_iters = P.max_iters <= 0 ? 100 : P.max_iters;
  C.min_matches = P.min_matches;
  if (int rc = select_device(device)) return rc;
  const size_t n = (size_t)n_pairs, m = (size_t)M, D = sizeof(double);
  // inputs, the work buffer (the current and the candidate points), then the outputs
  Staged S;
  const int h_ptr = S.in(match_ptr, (n + 1) * sizeof(int64_t)), h_xyz = S.in(xyz_i, 3 * m * D), h_uvi = S.in(uv_i, 2 * m * D), h_uvj = S.in(uv_j, 2 * m * D);
  const int h_p0 = S.in(pose_j0, 7 * n * D), h_const = S.in(&C, sizeof(TvConst));
  const int h_work = S.out(nullptr, 6 * m * D, true);
  const int h_pj = S.out(pose_j_out, 7 * n * D), h_pi = S.out(pose_i_out, 7 * n * D), h_cov = S.out(cov36_out, 36 * n * D), h_info = S.out(info_ut21_out, 21 * n * D);
  const int h_res = S.out(result, n * sizeof(fgo_two_view_result));
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  hipLaunchKernelGGL(k_two_view, dim3((unsigned)n_pairs), dim3(64), 0, 0, n_pairs, S.ptr<int64_t>(h_ptr), S.ptr<double>(h_xyz), S.ptr<double>(h_uvi),
                     S.ptr<double>(h_uvj), S.ptr<double>(h_p0), S.ptr<TvConst>(h_const), S.ptr<double>(h_work), M, S.ptr<double>(h_pj), S.ptr<double>(h_pi),
                     S.ptr<double>(h_cov), S.ptr<double>(h_info), S.ptr<fgo_two_view_result>(h_res));
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  return S.download();
}
