// RANSAC registration of visual-odometry records on the MI355X (gfx950, f64, wave64): the search, the rigid fit, its information
// and the void record of the reference's VRO step (m_ransac_iterations = 5000, gtsam/test/convert_vo2ba.cpp:448;
// getTransformFromMatches, gtsam/gtsam_graph.cpp:492; computeCovVRO, :256-277; makeItVoid, convert_vo2ba.cpp:424-436) for ONE pair
// of frames.  The VRO library's arithmetic is not in the reference; include/fgo.h states the semantics this file implements, and
// tests/vro_ransac_reference.py restates them in numpy.  The pairs are independent: fgo_vro_ransac_batch runs ONE WORKGROUP PER
// PAIR (W waves; W = 1 is the default, W = 4 the variant that lost the measurement) and all pairs in one launch.
//
//   score    ONE HYPOTHESIS PER LANE, 64 W at a time.  A lane draws its three matches from the counter-based hash, reads the six
//            points from global memory and builds R, t from the two triads.  The pair's matches are staged in LDS VR_CHUNK at a
//            time, 6 doubles per match; every lane reads the same match at the same time (a broadcast read) and tests
//            |p_i - (R p_j + t)|^2 <= max_dist^2.  Invalid hypotheses and the lanes past the last hypothesis skip the loop; the
//            barriers around the staging are outside every divergent branch, and their number is fixed by (K, M) before the
//            loop starts.  A pair that fits one chunk is staged once for all rounds.
//   winner   a lane keeps the best (count, h) of its own hypotheses (h rises, a later one has to be strictly better); the lanes
//            are merged by an integer butterfly (larger count, then lower h), the waves through LDS in wave order.
//   refine   wave 0 alone, the other waves are done: lanes stride the pair's matches in global memory.  A round = sums for the
//            centroids, sums for the cross-covariance, Horn's 4x4 eigenproblem by VR_SWEEPS cyclic Jacobi sweeps (wave-uniform,
//            redundantly in every lane), the new inlier mask.  The residual test is the same function the scoring uses.
//   info     a lane forms J^T S^-1 J of its inliers (3x3 Cholesky) and keeps 21 running sums; 6x6 Cholesky for the covariance.
// Every sum over matches is a per-lane sum in match order followed by a butterfly whose result is bit-identical in every lane: no
// atomics, no dependence on the rest of the batch, and every decision of phase two is wave-uniform without a broadcast.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include <cmath>
#include "../../include/fgo.h"
#include "small_dense_device.hpp"
#include "batch_call.hpp"

namespace fgo {
using namespace dev;

namespace {

constexpr int VR_CHUNK = 128;                 // matches staged in LDS at a time (6 KB)
constexpr int VR_SWEEPS = 8;                  // cyclic Jacobi sweeps of the 4x4 eigenproblem (quadratic convergence: 4 - 5 reach rounding)
constexpr int VR_MAX_MATCHES = INT_MAX / 3;   // of one pair: the kernel indexes its points with int (3 k + 2)
constexpr int VR_MAX_HYP = 1 << 20;
constexpr int VR_DEFAULT_WAVES = 1;             // measured against 4 on the bench tool: profiles/NOTES.md

struct VrArgs {
  int64_t n;
  const int64_t *ptr;
  const double *xi, *xj;
  int K, refine_rounds, min_inliers;
  uint64_t seed;
  double max_d2, min_side, min_area, rigid_tol, fx, fy, s_px2, sz0, sz1, sz2;
  double *pose, *info, *cov;                  // info / cov may be NULL
  uint8_t *mask;                              // always there: the refinement compares a round's set with the one before
  int32_t *hyp;                               // may be NULL
  fgo_vro_result *res;
};

struct Rt { double R[9], t[3]; };

__device__ __forceinline__ double norm3(const double v[3]) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
__device__ __forceinline__ void cross3(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// the orthonormal triad of three points as the columns of F (row-major), with the lengths the validity tests read
__device__ __forceinline__ void triad(const double *__restrict__ pa, const double *__restrict__ pb, const double *__restrict__ pc, double F[9],
                                      double &ab, double &ac, double &bc, double &area) {
  double d1[3], d2[3], d3[3], e1[3], e2[3], e3[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { d1[k] = pb[k] - pa[k]; d2[k] = pc[k] - pa[k]; d3[k] = pc[k] - pb[k]; }
  ab = norm3(d1); ac = norm3(d2); bc = norm3(d3);
  cross3(d1, d2, n);
  area = norm3(n);
#pragma unroll
  for (int k = 0; k < 3; ++k) e1[k] = d1[k] / ab;
  cross3(e1, d2, n);
  const double nn = norm3(n);
#pragma unroll
  for (int k = 0; k < 3; ++k) e3[k] = n[k] / nn;
  cross3(e3, e1, e2);
#pragma unroll
  for (int k = 0; k < 3; ++k) { F[3 * k] = e1[k]; F[3 * k + 1] = e2[k]; F[3 * k + 2] = e3[k]; }
}

// hypothesis h of a pair with M >= 3 matches at xi / xj; false if it is invalid
__device__ __forceinline__ bool hypothesis(const VrArgs &A, const double *__restrict__ xi, const double *__restrict__ xj, int h, int M, Rt &T) {
  int a, b, c;
  sample3(A.seed, (uint64_t)h, M, a, b, c);
  double Fi[9], Fj[9], abi, aci, bci, ari, abj, acj, bcj, arj;
  triad(xi + 3 * a, xi + 3 * b, xi + 3 * c, Fi, abi, aci, bci, ari);
  triad(xj + 3 * a, xj + 3 * b, xj + 3 * c, Fj, abj, acj, bcj, arj);
  const bool invalid = abi < A.min_side || abj < A.min_side || ari < A.min_area || arj < A.min_area || fabs(abi - abj) > A.rigid_tol ||
                       fabs(aci - acj) > A.rigid_tol || fabs(bci - bcj) > A.rigid_tol;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) T.R[3 * r + q] = Fi[3 * r] * Fj[3 * q] + Fi[3 * r + 1] * Fj[3 * q + 1] + Fi[3 * r + 2] * Fj[3 * q + 2];
  double mi[3], mj[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    mi[k] = (xi[3 * a + k] + xi[3 * b + k] + xi[3 * c + k]) / 3.0;
    mj[k] = (xj[3 * a + k] + xj[3 * b + k] + xj[3 * c + k]) / 3.0;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) T.t[r] = mi[r] - (T.R[3 * r] * mj[0] + T.R[3 * r + 1] * mj[1] + T.R[3 * r + 2] * mj[2]);
  return !invalid;
}

// |p_i - (R p_j + t)|^2 with the roundings spelled out: the scoring and the refinement have to agree on every match
__device__ __forceinline__ double resid2(const Rt &T, double ix, double iy, double iz, double jx, double jy, double jz) {
  const double rx = ix - fma(T.R[0], jx, fma(T.R[1], jy, fma(T.R[2], jz, T.t[0])));
  const double ry = iy - fma(T.R[3], jx, fma(T.R[4], jy, fma(T.R[5], jz, T.t[1])));
  const double rz = iz - fma(T.R[6], jx, fma(T.R[7], jy, fma(T.R[8], jz, T.t[2])));
  return fma(rx, rx, fma(ry, ry, rz * rz));
}

// the rotation maximising tr(R^T C), C = sum a b^T (a: centred p_i, b: centred p_j), as a quaternion x y z w with w >= 0: the
// eigenvector of the largest eigenvalue of Horn's N
__device__ __forceinline__ void horn(const double C[9], double q[4]) {
  // S = C^T = sum b a^T: Sxy = sum b_x a_y = C[3 * 1 + 0]
  const double Sxx = C[0], Sxy = C[3], Sxz = C[6], Syx = C[1], Syy = C[4], Syz = C[7], Szx = C[2], Szy = C[5], Szz = C[8];
  double a[16] = {Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx,
                  Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz,
                  Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy,
                  Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz};
  double v[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
#pragma unroll 1
  for (int sweep = 0; sweep < VR_SWEEPS; ++sweep) {
    jacobi_rot<4, 0, 1>(a, v); jacobi_rot<4, 0, 2>(a, v); jacobi_rot<4, 0, 3>(a, v);
    jacobi_rot<4, 1, 2>(a, v); jacobi_rot<4, 1, 3>(a, v); jacobi_rot<4, 2, 3>(a, v);
  }
  double best = a[0], e[4] = {v[0], v[4], v[8], v[12]};     // w x y z
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (a[5 * k] > best) { best = a[5 * k]; e[0] = v[k]; e[1] = v[4 + k]; e[2] = v[8 + k]; e[3] = v[12 + k]; }
  const double n = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]), sg = e[0] < 0 ? -1.0 : 1.0;
  q[0] = sg * e[1] / n; q[1] = sg * e[2] / n; q[2] = sg * e[3] / n; q[3] = sg * e[0] / n;
}

__device__ __forceinline__ void quat_to_R(const double q[4], double R[9]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = 1 - 2 * (x * x + y * y);
}

// the rotation matrix of a hypothesis as a quaternion x y z w, w >= 0 (refine_rounds = 0 reports the winner's own pose): the
// branch with the largest of the four squared components
__device__ __forceinline__ void R_to_quat(const double R[9], double q[4]) {
  const double tr = R[0] + R[4] + R[8];
  double x, y, z, w;
  if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
    w = 0.5 * sqrt(1 + tr); const double s = 0.25 / w;
    x = (R[7] - R[5]) * s; y = (R[2] - R[6]) * s; z = (R[3] - R[1]) * s;
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    x = 0.5 * sqrt(1 + R[0] - R[4] - R[8]); const double s = 0.25 / x;
    w = (R[7] - R[5]) * s; y = (R[1] + R[3]) * s; z = (R[2] + R[6]) * s;
  } else if (R[4] >= R[8]) {
    y = 0.5 * sqrt(1 - R[0] + R[4] - R[8]); const double s = 0.25 / y;
    w = (R[2] - R[6]) * s; x = (R[1] + R[3]) * s; z = (R[5] + R[7]) * s;
  } else {
    z = 0.5 * sqrt(1 - R[0] - R[4] + R[8]); const double s = 0.25 / z;
    w = (R[3] - R[1]) * s; x = (R[2] + R[6]) * s; y = (R[5] + R[7]) * s;
  }
  const double n = sqrt(x * x + y * y + z * z + w * w), sg = w < 0 ? -1.0 : 1.0;
  q[0] = sg * x / n; q[1] = sg * y / n; q[2] = sg * z / n; q[3] = sg * w / n;
}

// Sigma(p) = G diag(s_px2, s_px2, sigma_z(z)^2) G^T, upper triangle s00 s01 s02 s11 s12 s22
__device__ __forceinline__ void point_cov(const VrArgs &A, double x, double y, double z, double S[6]) {
  const double sz = A.sz0 + z * (A.sz1 + z * A.sz2), v = sz * sz, gx = z / A.fx, gy = z / A.fy, hx = x / z, hy = y / z;
  S[0] = gx * gx * A.s_px2 + hx * hx * v; S[1] = hx * hy * v; S[2] = hx * v;
  S[3] = gy * gy * A.s_px2 + hy * hy * v; S[4] = hy * v;
  S[5] = v;
}

template <int W>
__global__ __launch_bounds__(64 * W) void k_vro_ransac(VrArgs A) {
  __shared__ __attribute__((aligned(16))) double pts[VR_CHUNK * 6];     // a chunk of matches: p_i (3), p_j (3)
  __shared__ int w_cnt[W], w_h[W], w_valid[W];
  const int64_t pair = blockIdx.x;
  if (pair >= A.n) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = A.ptr[pair];
  const int M = (int)(A.ptr[pair + 1] - base), K = A.K;
  const double *__restrict__ xi = A.xi + 3 * base, *__restrict__ xj = A.xj + 3 * base;
  uint8_t *__restrict__ mask = A.mask + base;
  int32_t *__restrict__ hyp = A.hyp ? A.hyp + pair * (int64_t)K : nullptr;

  // ---- score: one hypothesis per lane
  int my_cnt = -1, my_h = INT_MAX, my_valid = 0;
  if (M >= 3) {                                    // uniform over the workgroup
    const int T = 64 * W, rounds = (K + T - 1) / T, chunks = (M + VR_CHUNK - 1) / VR_CHUNK;
    for (int r = 0; r < rounds; ++r) {
      const int h = r * T + tid;
      Rt H;
      const bool live = h < K && hypothesis(A, xi, xj, h, M, H);
      int cnt = live ? 0 : -1;
      for (int ch = 0; ch < chunks; ++ch) {
        const int m0 = ch * VR_CHUNK, mc = min(VR_CHUNK, M - m0);
        if (chunks > 1 || r == 0) {                // uniform: a pair of one chunk is staged once
          __syncthreads();
          for (int e = tid; e < 3 * mc; e += T) {
            const int m = e / 3, k = e - 3 * m;
            pts[6 * m + k] = xi[3 * m0 + e];
            pts[6 * m + 3 + k] = xj[3 * m0 + e];
          }
          __syncthreads();
        }
        if (live) {
#pragma unroll 8
          for (int m = 0; m < mc; ++m) {                  // unrolled: the LDS reads of eight matches are in flight at once
            const double *__restrict__ p = pts + 6 * m;
            cnt += resid2(H, p[0], p[1], p[2], p[3], p[4], p[5]) <= A.max_d2;
          }
        }
      }
      if (h < K) {
        if (hyp) hyp[h] = cnt;
        my_valid += live;
        if (cnt > my_cnt) { my_cnt = cnt; my_h = h; }
      }
    }
  } else if (hyp) {
    for (int h = tid; h < K; h += 64 * W) hyp[h] = -1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) better(my_cnt, my_h, __shfl_xor(my_cnt, o, 64), __shfl_xor(my_h, o, 64));
  my_valid = wave_sum(my_valid);
  if (lane == 0) { w_cnt[wave] = my_cnt; w_h[wave] = my_h; w_valid[wave] = my_valid; }
  __syncthreads();
  if (wave != 0) return;                           // the last barrier is behind: wave 0 goes on alone
  int best_cnt = w_cnt[0], best_h = w_h[0], n_valid = w_valid[0];
#pragma unroll
  for (int w = 1; w < W; ++w) { better(best_cnt, best_h, w_cnt[w], w_h[w]); n_valid += w_valid[w]; }
  if (best_cnt < 0) best_h = -1;

  // ---- refine: wave 0, lanes stride the matches; everything below that is not indexed by a match is wave-uniform
  int status = best_cnt < A.min_inliers ? FGO_VRO_TOO_FEW : FGO_VRO_OK, rounds_done = 0, n_in = 0;
  Rt P;
  double q[4] = {0, 0, 0, 1}, rmse = 0, info[21], cov[36];
  if (status == FGO_VRO_OK) {
    hypothesis(A, xi, xj, best_h, M, P);
    R_to_quat(P.R, q);
    for (int k = lane; k < M; k += 64) {
      const bool in = resid2(P, xi[3 * k], xi[3 * k + 1], xi[3 * k + 2], xj[3 * k], xj[3 * k + 1], xj[3 * k + 2]) <= A.max_d2;
      mask[k] = in;
      n_in += in;
    }
    n_in = wave_sum(n_in);
    for (int round = 0; round < A.refine_rounds; ++round) {
      double s[6] = {0, 0, 0, 0, 0, 0};
      for (int k = lane; k < M; k += 64)
        if (mask[k]) {
#pragma unroll
          for (int c = 0; c < 3; ++c) { s[c] += xi[3 * k + c]; s[3 + c] += xj[3 * k + c]; }
        }
#pragma unroll
      for (int c = 0; c < 6; ++c) s[c] = wave_sum(s[c]) / (double)n_in;
      double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int k = lane; k < M; k += 64)
        if (mask[k]) {
          const double a[3] = {xi[3 * k] - s[0], xi[3 * k + 1] - s[1], xi[3 * k + 2] - s[2]};
          const double b[3] = {xj[3 * k] - s[3], xj[3 * k + 1] - s[4], xj[3 * k + 2] - s[5]};
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) C[3 * r + c] += a[r] * b[c];
        }
#pragma unroll
      for (int c = 0; c < 9; ++c) C[c] = wave_sum(C[c]);
      horn(C, q);
      quat_to_R(q, P.R);
#pragma unroll
      for (int r = 0; r < 3; ++r) P.t[r] = s[r] - (P.R[3 * r] * s[3] + P.R[3 * r + 1] * s[4] + P.R[3 * r + 2] * s[5]);
      ++rounds_done;
      double chk = P.t[0] + P.t[1] + P.t[2];
#pragma unroll
      for (int c = 0; c < 9; ++c) chk += P.R[c];
      if (!(fabs(chk) < __builtin_huge_val())) { status = FGO_VRO_NUM; break; }     // a non-finite input reached the fit
      int changed = 0, n_new = 0;
      for (int k = lane; k < M; k += 64) {
        const bool in = resid2(P, xi[3 * k], xi[3 * k + 1], xi[3 * k + 2], xj[3 * k], xj[3 * k + 1], xj[3 * k + 2]) <= A.max_d2;
        changed += in != (mask[k] != 0);
        mask[k] = in;
        n_new += in;
      }
      n_in = wave_sum(n_new);
      changed = wave_sum(changed);
      if (n_in < A.min_inliers) { status = FGO_VRO_TOO_FEW; break; }
      if (changed == 0) break;
    }
  }

  // ---- information and rmse over the final inliers at the final pose
  if (status == FGO_VRO_OK) {
    double acc[21], ss = 0;
    int bad = 0;
#pragma unroll
    for (int c = 0; c < 21; ++c) acc[c] = 0;
    for (int k = lane; k < M; k += 64)
      if (mask[k]) {
        const double pi[3] = {xi[3 * k], xi[3 * k + 1], xi[3 * k + 2]}, pj[3] = {xj[3 * k], xj[3 * k + 1], xj[3 * k + 2]};
        ss += resid2(P, pi[0], pi[1], pi[2], pj[0], pj[1], pj[2]);
        if (!(pi[2] > 0) || !(pj[2] > 0)) { bad = 1; continue; }
        double Si[6], Sj[6], RS[9], S[6];
        point_cov(A, pi[0], pi[1], pi[2], Si);
        point_cov(A, pj[0], pj[1], pj[2], Sj);
        const double Sf[9] = {Sj[0], Sj[1], Sj[2], Sj[1], Sj[3], Sj[4], Sj[2], Sj[4], Sj[5]};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) RS[3 * r + c] = P.R[3 * r] * Sf[c] + P.R[3 * r + 1] * Sf[3 + c] + P.R[3 * r + 2] * Sf[6 + c];
        int o = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = r; c < 3; ++c, ++o) S[o] = Si[o] + (RS[3 * r] * P.R[3 * c] + RS[3 * r + 1] * P.R[3 * c + 1] + RS[3 * r + 2] * P.R[3 * c + 2]);
        // S = L L^T
        const bool ok0 = pivot_ok(S[0]);
        const double l00 = sqrt(ok0 ? S[0] : 1.0), l10 = S[1] / l00, l20 = S[2] / l00;
        const double d1 = S[3] - l10 * l10;
        const bool ok1 = pivot_ok(d1);
        const double l11 = sqrt(ok1 ? d1 : 1.0), l21 = (S[4] - l20 * l10) / l11;
        const double d2 = S[5] - l20 * l20 - l21 * l21;
        const bool ok2 = pivot_ok(d2);
        const double l22 = sqrt(ok2 ? d2 : 1.0);
        if (!(ok0 && ok1 && ok2)) { bad = 1; continue; }
        // J = [-R [p_j]x, R], W = L^-1 J
        double J[18], Wm[18];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double r0 = P.R[3 * r], r1 = P.R[3 * r + 1], r2 = P.R[3 * r + 2];
          J[6 * r] = -(r1 * pj[2] - r2 * pj[1]);
          J[6 * r + 1] = -(r2 * pj[0] - r0 * pj[2]);
          J[6 * r + 2] = -(r0 * pj[1] - r1 * pj[0]);
          J[6 * r + 3] = r0; J[6 * r + 4] = r1; J[6 * r + 5] = r2;
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          Wm[c] = J[c] / l00;
          Wm[6 + c] = (J[6 + c] - l10 * Wm[c]) / l11;
          Wm[12 + c] = (J[12 + c] - l20 * Wm[c] - l21 * Wm[6 + c]) / l22;
        }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int c = r; c < 6; ++c) acc[ut6(r, c)] += Wm[r] * Wm[c] + Wm[6 + r] * Wm[6 + c] + Wm[12 + r] * Wm[12 + c];
      }
    bad = wave_sum(bad);
    ss = wave_sum(ss);
#pragma unroll
    for (int c = 0; c < 21; ++c) info[c] = wave_sum(acc[c]);
    rmse = sqrt(ss / (double)n_in);
    // info = L L^T, cov = L^-T L^-1: the steps of dev::inv6 with the status seeded by `bad` and the full square as output (kept
    // here: see small_dense_device.hpp)
    double a[21];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c <= r; ++c) a[lt(r, c)] = info[ut6(c, r)];
    bool ok = bad == 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double d = a[lt(j, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) d -= a[lt(j, k)] * a[lt(j, k)];
      const bool okj = pivot_ok(d);
      ok = ok && okj;
      const double l = sqrt(okj ? d : 1.0);
      a[lt(j, j)] = l;
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double t = a[lt(i, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) t -= a[lt(i, k)] * a[lt(j, k)];
        a[lt(i, j)] = t / l;
      }
    }
    double Mi[21];                                 // L^-1, lower, packed by rows
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      Mi[lt(c, c)] = 1.0 / a[lt(c, c)];
#pragma unroll
      for (int r = c + 1; r < 6; ++r) {
        double t = 0;
#pragma unroll
        for (int k = c; k < r; ++k) t += a[lt(r, k)] * Mi[lt(k, c)];
        Mi[lt(r, c)] = -t / a[lt(r, r)];
      }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) {
        double t = 0;
#pragma unroll
        for (int k = c; k < 6; ++k) t += Mi[lt(k, r)] * Mi[lt(k, c)];
        cov[6 * r + c] = t;
        cov[6 * c + r] = t;
      }
    if (!ok) status = FGO_VRO_NUM;
  }

  // ---- the void record of a failed pair
  if (status != FGO_VRO_OK) {
    for (int k = lane; k < M; k += 64) mask[k] = 0;
    n_in = 0; rmse = 0;
    P.t[0] = P.t[1] = P.t[2] = 0;
    q[0] = q[1] = q[2] = 0; q[3] = 1;
#pragma unroll
    for (int c = 0; c < 21; ++c) info[c] = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) info[ut6(r, r)] = 10000.0;
#pragma unroll
    for (int c = 0; c < 36; ++c) cov[c] = 0;
  }
  if (lane != 0) return;
  A.res[pair] = {status, n_in, best_h, best_cnt, n_valid, rounds_done, rmse};
  double *po = A.pose + 7 * pair;
  po[0] = P.t[0]; po[1] = P.t[1]; po[2] = P.t[2]; po[3] = q[0]; po[4] = q[1]; po[5] = q[2]; po[6] = q[3];
  if (A.info) {
#pragma unroll
    for (int c = 0; c < 21; ++c) A.info[21 * pair + c] = info[c];
  }
  if (A.cov) {
#pragma unroll
    for (int c = 0; c < 36; ++c) A.cov[36 * pair + c] = cov[c];
  }
}

int g_waves = VR_DEFAULT_WAVES;
double g_kernel_ms = 0.0;

}  // namespace
}  // namespace fgo

extern "C" int fgo_debug_vro_waves(int waves) {
  if (waves == 0) fgo::g_waves = fgo::VR_DEFAULT_WAVES;
  else if (waves == 1 || waves == 4) fgo::g_waves = waves;
  return fgo::g_waves;
}
extern "C" double fgo_debug_vro_kernel_ms(void) { return fgo::g_kernel_ms; }

extern "C" void fgo_vro_params_default(fgo_vro_params *p) {
  if (!p) return;
  p->hypotheses = 5000;
  p->seed = 0;
  p->max_dist = 0.03;
  p->min_side = 0.05;
  p->rigid_tol = 0.03;
  p->refine_rounds = 3;
  p->min_inliers = 8;
  p->fx = p->fy = 250.5773;
  p->sigma_px = 1.0;
  p->sigma_z[0] = 0.014; p->sigma_z[1] = 0.0; p->sigma_z[2] = 0.0;
}

extern "C" int fgo_vro_ransac_batch(int device, int64_t n_pairs, const int64_t *match_ptr, const double *xyz_i, const double *xyz_j,
                                    const fgo_vro_params *params, double *pose_ij7_out, double *info_ut21_out, double *cov36_out,
                                    uint8_t *inlier_out, int32_t *hyp_count_out, fgo_vro_result *result) {
  using namespace fgo;
  fgo_vro_params P;
  fgo_vro_params_default(&P);
  if (params) P = *params;
  if (n_pairs < 0 || n_pairs > INT_MAX) return FGO_EINVAL;
  if (P.hypotheses < 1 || P.hypotheses > VR_MAX_HYP || !(P.max_dist > 0) || !(P.min_side > 0) || !(P.fx > 0) || !(P.fy > 0) ||
      !(P.sigma_px > 0) || !(P.rigid_tol >= 0) || P.refine_rounds < 0 || P.refine_rounds > 10 || P.min_inliers < 3)
    return FGO_EINVAL;
  if (!(P.sigma_z[0] >= 0) || !(P.sigma_z[1] >= 0) || !(P.sigma_z[2] >= 0) || !(P.sigma_z[0] + P.sigma_z[1] + P.sigma_z[2] > 0)) return FGO_EINVAL;
  if (n_pairs == 0) return FGO_OK;
  if (!match_ptr || !xyz_i || !xyz_j || !pose_ij7_out || !result) return FGO_EINVAL;
  if (!csr_ptr_ok(match_ptr, n_pairs, VR_MAX_MATCHES)) return FGO_EINVAL;
  const int64_t m_total = match_ptr[n_pairs];
  if ((uint64_t)m_total > SIZE_MAX / (3 * sizeof(double))) return FGO_EINVAL;
  if (int rc = select_device(device)) return rc;
  const size_t n = (size_t)n_pairs, m = (size_t)m_total, D = sizeof(double), K = (size_t)P.hypotheses;
  // inputs, then the outputs (the mask is always there: the kernel works in it)
  Staged S;
  const int h_ptr = S.in(match_ptr, (n + 1) * sizeof(int64_t)), h_xi = S.in(xyz_i, 3 * m * D), h_xj = S.in(xyz_j, 3 * m * D);
  const int h_pose = S.out(pose_ij7_out, 7 * n * D), h_info = S.out(info_ut21_out, 21 * n * D), h_cov = S.out(cov36_out, 36 * n * D);
  const int h_mask = S.out(inlier_out, m, true), h_hyp = S.out(hyp_count_out, n * K * sizeof(int32_t));
  const int h_res = S.out(result, n * sizeof(fgo_vro_result));
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  VrArgs A;
  A.n = n_pairs;
  A.ptr = S.ptr<int64_t>(h_ptr); A.xi = S.ptr<double>(h_xi); A.xj = S.ptr<double>(h_xj);
  A.K = P.hypotheses; A.refine_rounds = P.refine_rounds; A.min_inliers = P.min_inliers;
  A.seed = P.seed;
  A.max_d2 = P.max_dist * P.max_dist; A.min_side = P.min_side; A.min_area = P.min_side * P.min_side; A.rigid_tol = P.rigid_tol;
  A.fx = P.fx; A.fy = P.fy; A.s_px2 = P.sigma_px * P.sigma_px;
  A.sz0 = P.sigma_z[0]; A.sz1 = P.sigma_z[1]; A.sz2 = P.sigma_z[2];
  A.pose = S.ptr<double>(h_pose); A.info = S.ptr<double>(h_info); A.cov = S.ptr<double>(h_cov);
  A.mask = S.ptr<uint8_t>(h_mask);
  A.hyp = S.ptr<int32_t>(h_hyp);
  A.res = S.ptr<fgo_vro_result>(h_res);
  KernelTimer timer;
  if (!timer.start()) return FGO_ENUM;
  if (g_waves == 1) hipLaunchKernelGGL(k_vro_ransac<1>, dim3((unsigned)n_pairs), dim3(64), 0, 0, A);
  else hipLaunchKernelGGL(k_vro_ransac<4>, dim3((unsigned)n_pairs), dim3(256), 0, 0, A);
  timer.stop();
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  g_kernel_ms = timer.ms();
  return S.download();
}
