// IMU check of visual-odometry records on the MI355X (gfx950, f64, wave64): the chi-square test the chi2_for_vro switch turns on in
// the reference's drivers (gtsam/test_vro_imu_graph.cpp:679-778) for ONE record -- the record's rotation against the rotation the
// IMU preintegrated between the same two key frames.  The records are independent, so fgo_imu_check_vro_batch runs ONE WAVE PER
// RECORD and all records in one launch.
//
//   dR_imu = dR Exp(J_R_bg (bg_i - bhat_g))   (:708-710, corrected as fgo_preint_predict corrects it)
//   dR_vro = R_uc R(q_ij) R_uc^T              (:692-698)
//   dRw = dR_imu^T dR_vro, dw = Log(dRw), D = Dlog(dw), J_imu = -D dRw^T (:714-717), J_vro = D (commented out in the reference)
//   calibrated   S = J_imu Sth J_imu^T + D (R_uc Sij[0:3, 0:3] R_uc^T) D^T, Sth = Sigma15[0:3, 0:3], d2 = dw^T S^-1 dw (3x3 Cholesky)
//   reference    Lth = (Sigma15^-1)[0:3, 0:3], d2_ref = dw^T J_imu Lth J_imu^T dw (:724-743)
//
// The 15x15 inverse is never formed.  Sigma15 is staged in LDS with the theta block ordered LAST (p v ba bg theta) and factored
// there, Sigma15 = L L^T; the trailing block of the inverse is then (L_tt L_tt^T)^-1 with L_tt the factor's trailing 3x3 triangle,
// so d2_ref = |L_tt^-1 J_imu^T dw|^2: one 3x3 forward substitution.
//
// Schedule of a wave: the small work (the 6x6 inverse of the record's information, the logarithm, the Jacobians, the 3x3 Cholesky)
// is wave-uniform and runs redundantly in every lane, so the record's status needs no broadcast; lane 0 writes the results.  The
// right-looking Cholesky of the 15x15 runs across the lanes: the column steps are wave-uniform, the scaling of a column and the
// rank-1 update of the trailing block are spread over the lanes, one entry of the lower triangle per lane and pass.  An entry is
// updated by the column steps in their order, whoever owns it: no atomics, every sum in a fixed order that depends on nothing but
// the record, so results are bit-identical from call to call and do not depend on what else is in the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include <cmath>
#include "../../include/fgo.h"
#include "pose3_device.hpp"
#include "small_dense_device.hpp"
#include "batch_call.hpp"

namespace fgo {
using namespace dev;

namespace {

struct IcArgs {
  int64_t n;
  const double *pose, *info, *cov, *bias;
  const fgo_preint *preint;
  const int64_t *index;
  double q_uc[4];
  double d2_gate, d2_ref_gate, failed00;
  fgo_imu_check_result *res;
  double *dw, *cov_dw;                             // may be NULL
};

// the LDS traffic of one wave: orders this wave's LDS accesses around the point for the compiler and the hardware
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the leading 3x3 block (s00 s01 s02 s11 s12 s22) of A^-1 for the symmetric 6x6 A given by its upper triangle; false if a pivot is
// <= 0 or not finite.  The part of inv6 that these six entries do not need is never computed.
__device__ __forceinline__ bool inv6_lead3(const double *__restrict__ a_ut, double S[6]) {
  double Si[21];
  const bool ok = inv6(a_ut, Si);
  S[0] = Si[ut6(0, 0)]; S[1] = Si[ut6(0, 1)]; S[2] = Si[ut6(0, 2)]; S[3] = Si[ut6(1, 1)]; S[4] = Si[ut6(1, 2)]; S[5] = Si[ut6(2, 2)];
  return ok;
}

// J A J^T of a symmetric A: the upper triangle is computed and mirrored, so the result is exactly symmetric
__device__ __forceinline__ M3 congr3(const M3 &J, const M3 &A) {
  const M3 T = mm(J, A);
  M3 C;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = r; c < 3; ++c) {
      const double s = T.m[r * 3] * J.m[c * 3] + T.m[r * 3 + 1] * J.m[c * 3 + 1] + T.m[r * 3 + 2] * J.m[c * 3 + 2];
      C.m[r * 3 + c] = s;
      C.m[c * 3 + r] = s;
    }
  return C;
}

__device__ __forceinline__ Q4 qunit(Q4 q) {
  const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return {q.x / n, q.y / n, q.z / n, q.w / n};
}
__device__ __forceinline__ Q4 qunit(const double *__restrict__ q) { return qunit(Q4{q[0], q[1], q[2], q[3]}); }

__global__ __launch_bounds__(64) void k_imu_check(IcArgs A) {
  __shared__ double L[225];                        // Sigma15 in the order p v ba bg theta, then its Cholesky factor (lower triangle)
  const int64_t rec = blockIdx.x;
  if (rec >= A.n) return;
  const int lane = threadIdx.x;
  const fgo_preint *__restrict__ pm = A.preint + A.index[rec];

  // Sij[0:3, 0:3] (s00 s01 s02 s11 s12 s22), in every lane
  double sw[6];
  int status = FGO_IC_OK;
  if (A.cov) {
    const double *__restrict__ c = A.cov + 36 * rec;
    sw[0] = c[0]; sw[1] = c[1]; sw[2] = c[2]; sw[3] = c[7]; sw[4] = c[8]; sw[5] = c[14];
  } else {
    const double *__restrict__ a = A.info + 21 * rec;
    if (A.failed00 > 0 && a[0] == A.failed00) status = FGO_IC_SKIPPED;     // the failed-VO sentinel
    else if (!inv6_lead3(a, sw)) status = FGO_IC_NUM;
  }

  // Sigma15 = L L^T in LDS, theta last: entry (r, c) of the staged matrix is entry ((r + 3) % 15, (c + 3) % 15) of preintMeasCov
  if (status == FGO_IC_OK) {                       // wave-uniform
    for (int e = lane; e < 225; e += 64) {
      const int r = e / 15, c = e - 15 * r, pr = r < 12 ? r + 3 : r - 12, pc = c < 12 ? c + 3 : c - 12;
      L[e] = 0.5 * (pm->cov[pr * 15 + pc] + pm->cov[pc * 15 + pr]);
    }
    wave_sync();
    bool ok = true;
    for (int j = 0; j < 15; ++j) {
      const double d = L[j * 16];                  // every lane reads the pivot before lane j replaces it: ok stays wave-uniform
      const bool okj = pivot_ok(d);
      ok = ok && okj;
      const double l = sqrt(okj ? d : 1.0);
      wave_sync();
      if (lane == j) L[j * 16] = l;
      if (lane > j && lane < 15) L[lane * 15 + j] /= l;
      wave_sync();
      for (int e = lane; e < 225; e += 64) {       // the trailing block's lower triangle: (r, c) with j < c <= r
        const int r = e / 15, c = e - 15 * r;
        if (c > j && c <= r) L[e] -= L[r * 15 + j] * L[c * 15 + j];
      }
      wave_sync();
    }
    if (!ok) status = FGO_IC_NUM;
  }

  M3 S = mzero();
  V3 dw = {0, 0, 0};
  double d2 = 0, d2_ref = 0, angle = 0;
  if (status == FGO_IC_OK) {
    // dR_imu, dR_vro as unit quaternions
    Q4 q_imu = qunit(pm->dR);
    if (A.bias) {
      const double *__restrict__ b = A.bias + 6 * rec;
      const V3 dbg = {b[3] - pm->bhat[3], b[4] - pm->bhat[4], b[5] - pm->bhat[5]};
      const M3 J = {{pm->J_R_bg[0], pm->J_R_bg[1], pm->J_R_bg[2], pm->J_R_bg[3], pm->J_R_bg[4], pm->J_R_bg[5], pm->J_R_bg[6],
                     pm->J_R_bg[7], pm->J_R_bg[8]}};
      q_imu = qunit(qmul(q_imu, so3_exp(mv(J, dbg))));
    }
    const Q4 q_uc = qunit(A.q_uc), q_ij = qunit(A.pose + 7 * rec + 3);
    const Q4 q_vro = qmul(qmul(q_uc, q_ij), qconj(q_uc));
    const Q4 q_w = qunit(qmul(qconj(q_imu), q_vro));
    dw = so3_log(q_w);
    angle = sqrt(dot3(dw, dw));
    const M3 D = so3_dlog(dw), J_imu = mscale(mm(D, mtrans(qmat(q_w))), -1.0), R_uc = qmat(q_uc);
    M3 Sigma_th;                                   // from the payload: the factor has overwritten the staged block
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) Sigma_th.m[r * 3 + c] = 0.5 * (pm->cov[r * 15 + c] + pm->cov[c * 15 + r]);
    const M3 Sww = {{sw[0], sw[1], sw[2], sw[1], sw[3], sw[4], sw[2], sw[4], sw[5]}};
    const M3 S_imu = congr3(J_imu, Sigma_th), S_vro = congr3(D, congr3(R_uc, Sww));
#pragma unroll
    for (int k = 0; k < 9; ++k) S.m[k] = S_imu.m[k] + S_vro.m[k];
    // d2 = dw^T S^-1 dw
    {
      const double a00 = S.m[0], a10 = S.m[3], a11 = S.m[4], a20 = S.m[6], a21 = S.m[7], a22 = S.m[8];
      const bool ok0 = pivot_ok(a00);
      const double l00 = sqrt(ok0 ? a00 : 1.0), l10 = a10 / l00, l20 = a20 / l00;
      const double s1 = a11 - l10 * l10;
      const bool ok1 = pivot_ok(s1);
      const double l11 = sqrt(ok1 ? s1 : 1.0), l21 = (a21 - l20 * l10) / l11;
      const double s2 = a22 - l20 * l20 - l21 * l21;
      const bool ok2 = pivot_ok(s2);
      const double l22 = sqrt(ok2 ? s2 : 1.0);
      const double y0 = dw.x / l00, y1 = (dw.y - l10 * y0) / l11, y2 = (dw.z - l20 * y0 - l21 * y1) / l22;
      d2 = y0 * y0 + y1 * y1 + y2 * y2;
      if (!(ok0 && ok1 && ok2)) status = FGO_IC_NUM;
    }
    // d2_ref = |L_tt^-1 J_imu^T dw|^2
    {
      const V3 u = mtv(J_imu, dw);
      const double y0 = u.x / L[12 * 16], y1 = (u.y - L[13 * 15 + 12] * y0) / L[13 * 16];
      const double y2 = (u.z - L[14 * 15 + 12] * y0 - L[14 * 15 + 13] * y1) / L[14 * 16];
      d2_ref = y0 * y0 + y1 * y1 + y2 * y2;
    }
  }
  if (lane != 0) return;
  if (status != FGO_IC_OK) { S = mzero(); dw = {0, 0, 0}; d2 = d2_ref = angle = 0; }
  const int reject = status != FGO_IC_OK ? 0 : (d2 > A.d2_gate ? 1 : 0) | (d2_ref > A.d2_ref_gate ? 2 : 0);
  A.res[rec] = {status, reject, d2, d2_ref, angle};
  if (A.dw) { double *o = A.dw + 3 * rec; o[0] = dw.x; o[1] = dw.y; o[2] = dw.z; }
  if (A.cov_dw) {
    double *o = A.cov_dw + 9 * rec;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = S.m[k];
  }
}

}  // namespace
}  // namespace fgo

extern "C" void fgo_imu_check_params_default(fgo_imu_check_params *p) {
  if (!p) return;
  p->d2_gate = fgo_chi2_quantile(3, 0.95);
  p->d2_ref_gate = 40000.0;
  p->failed_info00 = 10000.0;
}

extern "C" int fgo_imu_check_vro_batch(int device, int64_t n_records, const double *pose_ij7, const double *info_ut21, const double *cov36,
                                       int64_t n_preint, const fgo_preint *preint, const int64_t *preint_index, const double *bias_i6,
                                       const double imu_q_cam4[4], const fgo_imu_check_params *params, fgo_imu_check_result *result,
                                       double *dw_out, double *cov_dw9_out) {
  using namespace fgo;
  fgo_imu_check_params P;
  fgo_imu_check_params_default(&P);
  if (params) P = *params;
  if (n_records < 0 || n_records > INT_MAX || !(P.d2_gate > 0) || !(P.d2_ref_gate > 0)) return FGO_EINVAL;
  if (imu_q_cam4 && !quat_ok(imu_q_cam4)) return FGO_EINVAL;
  if (n_records == 0) return FGO_OK;
  if (!pose_ij7 || !preint || !preint_index || !result || (info_ut21 != nullptr) == (cov36 != nullptr)) return FGO_EINVAL;
  if (n_preint < 1 || (uint64_t)n_preint > SIZE_MAX / sizeof(fgo_preint)) return FGO_EINVAL;
  for (int64_t r = 0; r < n_records; ++r)
    if (preint_index[r] < 0 || preint_index[r] >= n_preint || !quat_ok(pose_ij7 + 7 * r + 3)) return FGO_EINVAL;
  if (int rc = select_device(device)) return rc;
  const size_t n = (size_t)n_records, D = sizeof(double);
  // inputs, then the result records, then the outputs that were asked for
  Staged S;
  const int h_pose = S.in(pose_ij7, 7 * n * D), h_info = S.in(info_ut21, 21 * n * D), h_cov = S.in(cov36, 36 * n * D);
  const int h_preint = S.in(preint, (size_t)n_preint * sizeof(fgo_preint)), h_index = S.in(preint_index, n * sizeof(int64_t));
  const int h_bias = S.in(bias_i6, 6 * n * D);
  const int h_res = S.out(result, n * sizeof(fgo_imu_check_result)), h_dw = S.out(dw_out, 3 * n * D), h_cov_dw = S.out(cov_dw9_out, 9 * n * D);
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  IcArgs A;
  A.n = n_records;
  A.pose = S.ptr<double>(h_pose); A.info = S.ptr<double>(h_info); A.cov = S.ptr<double>(h_cov);
  A.preint = S.ptr<fgo_preint>(h_preint);
  A.index = S.ptr<int64_t>(h_index);
  A.bias = S.ptr<double>(h_bias);
  for (int k = 0; k < 4; ++k) A.q_uc[k] = imu_q_cam4 ? imu_q_cam4[k] : (k == 3 ? 1.0 : 0.0);
  A.d2_gate = P.d2_gate; A.d2_ref_gate = P.d2_ref_gate; A.failed00 = P.failed_info00;
  A.res = S.ptr<fgo_imu_check_result>(h_res);
  A.dw = S.ptr<double>(h_dw); A.cov_dw = S.ptr<double>(h_cov_dw);
  hipLaunchKernelGGL(k_imu_check, dim3((unsigned)n_records), dim3(64), 0, 0, A);
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  return S.download();
}
