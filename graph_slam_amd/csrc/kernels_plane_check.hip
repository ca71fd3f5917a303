// Plane check of visual-odometry records on the MI355X (gfx950, f64, wave64): what gtsam/test_plane_check_vo.cpp does for ONE record
// (computePlaneNodeDis :328-379, computePlaneDis :383-445) -- the planes seen in frame i are carried through the record's relative
// pose Tij into frame j, paired with the planes seen there, every pair gets a Mahalanobis distance that accounts for the
// uncertainty of the pose (Sij = information^-1, :167) and of both plane fits, and the record keeps the largest distance;
// gtsam/test/delete_vo_by_plane_check.cpp then drops the records whose distance is too large.  The records are independent, so
// fgo_plane_check_vro_batch runs ONE WAVE PER RECORD and all records in one launch.
//
//   plane i      PE = Pi.transform(Tij): n' = R^T n, d' = n.t + d, with D_pose (3x6, tangent [omega; v]) and D_plane (3x3) as
//                dev::plane_factor<true> forms them;  S_Pi = diag(B(n)^T S_n B(n), S_d);
//                S_PE = D_pose Sij D_pose^T + D_plane S_Pi D_plane^T;   sdj = S_d + n^T S_t n + g^T S_n g, g = (I - n n^T) t
//                (CGraphGT::computeSdj, gtsam/gtsam_graph.cpp:725-748)
//   matching     plane i takes the first j, in order, with |n'.n_j| >= cos_min and |d' - d_j| <= d_max (:338-362)
//   pair         e = PE.errorVector(Pj) = [B(n')^T n_j; d' - d_j], raw = e.e, S_e = H1 S_PE H1^T + H2 S_Pj H2^T, d2 = e^T S_e^-1 e
//                (3x3 Cholesky); H2 = diag(B(n')^T B(n_j), -1), H1 = diag(Hp, 1) with Hp the derivative of B(n')^T n_j along
//                n' -> retract(n', v), taken through the basis rule with its axis held fixed (GTSAM 4.0's Unit3::errorVector)
//   record       err = the largest d2 over the matched planes i (strict >, in order of i), err_raw = that pair's raw
//
// Schedule of a wave: every lane inverts the record's information redundantly (6x6 Cholesky in registers), so Sij and the
// record's status are wave-uniform without a broadcast.  The planes i are then taken 64 at a time: lane l transforms plane l of the
// block and stages n', d', S_PE in LDS; the block's candidate pairs (i, j), i-major, are owned by lanes in chunks of 64; the first
// matching j of an i is the lowest set bit of the chunk's ballot among that i's lanes, and whether the i that straddles a chunk
// boundary has matched already is carried (wave-uniform) into the next chunk; only the selected pairs do the Jacobian and Cholesky
// work, and leave d2 / raw / j in the LDS slot of their i; lane l folds plane l into its running maximum.  One ordered butterfly
// at the end gives the record's maximum (ties to the smaller i).  LDS holds one block of 64 planes, so the number of planes per
// frame is not capped.  Every small loop is unrolled with compile-time indices, no atomics, every sum in a fixed order that
// depends on nothing but the record: results are bit-identical from call to call and do not depend on what else is in the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include <cmath>
#include "../../include/fgo.h"
#include "device_plan.hpp"
#include "factors_device.hpp"
#include "small_dense_device.hpp"
#include "plane_fit_device.hpp"
#include "batch_call.hpp"

namespace fgo {
using namespace dev;

namespace {

// LDS rows of 64 doubles, one column per plane i of the block
constexpr int PC_N = 0, PC_D = 3, PC_S = 4, PC_D2 = 10, PC_RAW = 11, PC_ROWS = 12;

struct PcArgs {
  int64_t n;
  const double *pose, *info, *cov;
  const int64_t *pi_ptr, *pj_ptr;
  const double *pi_abcd, *pi_cov, *pj_abcd, *pj_cov;
  double cos_min, d_max, failed00;
  fgo_plane_check_result *res;
  int64_t *match;                                  // the per-plane outputs may be NULL
  double *d2, *raw, *pred, *pred_cov, *sdj;
};

// B^T S B (u00 u01 u11) of a symmetric 3x3 S
__device__ __forceinline__ void tangent_cov(const Basis &B, const M3 &S, double u[3]) {
  const V3 s1 = mv(S, B.b1), s2 = mv(S, B.b2);
  u[0] = dot3(B.b1, s1); u[1] = dot3(B.b1, s2); u[2] = dot3(B.b2, s2);
}

// Q U Q^T (m00 m01 m11) of a 2x2 Q (q00 q01 q10 q11) and a symmetric 2x2 U (u00 u01 u11)
__device__ __forceinline__ void congr2(const double q[4], const double u[3], double m[3]) {
  const double a00 = q[0] * u[0] + q[1] * u[1], a01 = q[0] * u[1] + q[1] * u[2];
  const double a10 = q[2] * u[0] + q[3] * u[1], a11 = q[2] * u[1] + q[3] * u[2];
  m[0] = a00 * q[0] + a01 * q[1];
  m[1] = a00 * q[2] + a01 * q[3];
  m[2] = a10 * q[2] + a11 * q[3];
}

// Unit3::basis() with the axis it chose (the coordinate axis of the smallest |n_i|; ties: x, then y, then z) and |n x axis|
__device__ __forceinline__ Basis unit3_basis_axis(V3 n, V3 &ax, double &nc) {
  const double mx = fabs(n.x), my = fabs(n.y), mz = fabs(n.z);
  ax = {0, 0, 1};
  if (mx <= my && mx <= mz) ax = {1, 0, 0};
  else if (my <= mx && my <= mz) ax = {0, 1, 0};
  V3 b1 = cross(n, ax);
  nc = sqrt(dot3(b1, b1));
  b1 = {b1.x / nc, b1.y / nc, b1.z / nc};
  return {b1, cross(n, b1)};
}

// The pair (PE, Pj): d2 and raw; false when S_e is not positive definite.  PE = (np, dp) with its covariance pe (upper triangle
// p00 p01 p02 p11 p12 p22 in the tangent of PE).
__device__ __forceinline__ bool pair_distance(V3 np, double dp, const double pe[6], const PlaneIn &Pj, double &d2, double &raw) {
  V3 ax;
  double nc;
  const Basis Bp = unit3_basis_axis(np, ax, nc), Bj = unit3_basis(Pj.n);
  const double e0 = dot3(Bp.b1, Pj.n), e1 = dot3(Bp.b2, Pj.n), e2 = dp - Pj.d;
  raw = e0 * e0 + e1 * e1 + e2 * e2;
  // H2 S_Pj H2^T, H2 = diag(B(n')^T B(n_j), -1)
  const double h[4] = {dot3(Bp.b1, Bj.b1), dot3(Bp.b1, Bj.b2), dot3(Bp.b2, Bj.b1), dot3(Bp.b2, Bj.b2)};
  double uj[3], m2[3];
  tangent_cov(Bj, Pj.Sn, uj);
  congr2(h, uj, m2);
  // Hp: column k is the derivative along dn = b_k;  c = n' x axis, b1 = c / |c|, b2 = n' x b1
  double hp[4];
  {
    const V3 dn[2] = {Bp.b1, Bp.b2};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const V3 dc = cross(dn[k], ax);
      const double pr = dot3(Bp.b1, dc);
      const V3 db1 = {(dc.x - Bp.b1.x * pr) / nc, (dc.y - Bp.b1.y * pr) / nc, (dc.z - Bp.b1.z * pr) / nc};
      const V3 db2 = cross(dn[k], Bp.b1) + cross(np, db1);
      hp[k] = dot3(Pj.n, db1);
      hp[2 + k] = dot3(Pj.n, db2);
    }
  }
  // H1 S_PE H1^T, H1 = diag(Hp, 1)
  const double u1[3] = {pe[0], pe[1], pe[3]};
  double m1[3];
  congr2(hp, u1, m1);
  const double w0 = hp[0] * pe[2] + hp[1] * pe[4], w1 = hp[2] * pe[2] + hp[3] * pe[4];
  double l[6];
  const bool pd = chol3(m1[0] + m2[0], m1[1] + m2[1], m1[2] + m2[2], w0, w1, pe[5] + Pj.Sd, l);
  d2 = solve3_sq(l, e0, e1, e2);
  return pd;
}

__global__ __launch_bounds__(64) void k_plane_check(PcArgs A) {
  __shared__ double sm[PC_ROWS * 64];
  __shared__ int sj[64], sbad[64];
  const int64_t rec = blockIdx.x;
  if (rec >= A.n) return;
  const int lane = threadIdx.x;
  const int64_t gi0 = A.pi_ptr[rec], gj0 = A.pj_ptr[rec];
  const int ni = (int)(A.pi_ptr[rec + 1] - gi0), nj = (int)(A.pj_ptr[rec + 1] - gj0);

  // Sij, in every lane
  double S[21];
  int status = FGO_PC_OK;
  if (A.cov) {
    const double *__restrict__ c = A.cov + 36 * rec;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int k = r; k < 6; ++k) S[ut6(r, k)] = c[r * 6 + k];
  } else {
    const double *__restrict__ a = A.info + 21 * rec;
    if (A.failed00 > 0 && a[0] == A.failed00) status = FGO_PC_SKIPPED;     // the failed-VO sentinel (:171)
    else if (!inv6(a, S)) status = FGO_PC_NUM;
  }
  if (status != FGO_PC_OK) {
    for (int i = lane; i < ni; i += 64) {
      const int64_t g = gi0 + i;
      if (A.match) A.match[g] = -1;
      if (A.d2) A.d2[g] = 0;
      if (A.raw) A.raw[g] = 0;
      if (A.sdj) A.sdj[g] = 0;
      if (A.pred) for (int k = 0; k < 4; ++k) A.pred[4 * g + k] = 0;
      if (A.pred_cov) for (int k = 0; k < 9; ++k) A.pred_cov[9 * g + k] = 0;
    }
    if (lane == 0) A.res[rec] = {status, 0, 0, -1, -1, 0, 0.0, 0.0};
    return;
  }

  const double *__restrict__ ps = A.pose + 7 * rec;
  const V3 t = {ps[0], ps[1], ps[2]};
  const double qn = sqrt(ps[3] * ps[3] + ps[4] * ps[4] + ps[5] * ps[5] + ps[6] * ps[6]);
  const M3 R = qmat(Q4{ps[3] / qn, ps[4] / qn, ps[5] / qn, ps[6] / qn});
  const M3 Sww = block3(S, 0, 0), Swv = block3(S, 0, 3), Svv = block3(S, 3, 3);

  double best = 0, best_raw = 0;                   // this lane's planes, in order of i
  int best_i = -1, best_j = -1, n_matched = 0, n_bad = 0;

  for (int ib = 0; ib < ni; ib += 64) {
    const int cnt = min(64, ni - ib);
    __syncthreads();                               // the readers of the previous block are done
    if (lane < cnt) {
      const int64_t g = gi0 + ib + lane;
      const PlaneIn P = load_plane(A.pi_abcd + 4 * g, A.pi_cov + 16 * g);
      const V3 np = mtv(R, P.n);
      const double dp = dot3(P.n, t) + P.d;
      const Basis Bp = unit3_basis(np), B = unit3_basis(P.n);
      // D_pose = [[r1^T, 0], [r2^T, 0], [0, n'^T]],  r_a = b'_a x n'
      const V3 r1 = cross(Bp.b1, np), r2 = cross(Bp.b2, np);
      const V3 w1 = mv(Sww, r1), w2 = mv(Sww, r2), x = mv(Swv, np);
      double pe[6] = {dot3(r1, w1), dot3(r1, w2), dot3(r1, x), dot3(r2, w2), dot3(r2, x), dot3(np, mv(Svv, np))};
      // D_plane = [[Q, 0], [tb^T, 1]],  Q = B'^T R^T B, tb = B^T t;  S_Pi = diag(U, S_d)
      const V3 Rb1 = mtv(R, B.b1), Rb2 = mtv(R, B.b2);
      const double q[4] = {dot3(Bp.b1, Rb1), dot3(Bp.b1, Rb2), dot3(Bp.b2, Rb1), dot3(Bp.b2, Rb2)};
      const double tb0 = dot3(B.b1, t), tb1 = dot3(B.b2, t);
      double u[3], m[3];
      tangent_cov(B, P.Sn, u);
      congr2(q, u, m);
      const double ut0 = u[0] * tb0 + u[1] * tb1, ut1 = u[1] * tb0 + u[2] * tb1;       // U tb
      pe[0] += m[0]; pe[1] += m[1]; pe[3] += m[2];
      pe[2] += q[0] * ut0 + q[1] * ut1;
      pe[4] += q[2] * ut0 + q[3] * ut1;
      pe[5] += tb0 * ut0 + tb1 * ut1 + P.Sd;
      sm[(PC_N + 0) * 64 + lane] = np.x; sm[(PC_N + 1) * 64 + lane] = np.y; sm[(PC_N + 2) * 64 + lane] = np.z;
      sm[PC_D * 64 + lane] = dp;
#pragma unroll
      for (int k = 0; k < 6; ++k) sm[(PC_S + k) * 64 + lane] = pe[k];
      sm[PC_D2 * 64 + lane] = 0; sm[PC_RAW * 64 + lane] = 0;
      sj[lane] = -1; sbad[lane] = 0;
      if (A.pred) { double *o = A.pred + 4 * g; o[0] = np.x; o[1] = np.y; o[2] = np.z; o[3] = dp; }
      if (A.pred_cov) {
        double *o = A.pred_cov + 9 * g;
        o[0] = pe[0]; o[1] = pe[1]; o[2] = pe[2]; o[3] = pe[1]; o[4] = pe[3]; o[5] = pe[4]; o[6] = pe[2]; o[7] = pe[4]; o[8] = pe[5];
      }
      if (A.sdj) A.sdj[g] = predicted_sdj(P, t, Svv);
    }
    __syncthreads();

    // the block's candidate pairs, i-major, 64 at a time
    const int64_t npairs = (int64_t)cnt * nj;
    int64_t carry_i = -1;                          // the last i of the previous chunk, and whether it has matched (wave-uniform)
    bool carry_m = false;
    for (int64_t base = 0; base < npairs; base += 64) {
      const int64_t p = base + lane;
      const bool valid = p < npairs;
      const int64_t il = valid ? p / nj : 0;
      const int j = (int)(p - il * nj);
      bool cond = false;
      V3 np = {0, 0, 0};
      double dp = 0;
      PlaneIn Pj;
      if (valid) {
        np = {sm[(PC_N + 0) * 64 + il], sm[(PC_N + 1) * 64 + il], sm[(PC_N + 2) * 64 + il]};
        dp = sm[PC_D * 64 + il];
        Pj = load_plane(A.pj_abcd + 4 * (gj0 + j), A.pj_cov + 16 * (gj0 + j));
        cond = fabs(dot3(np, Pj.n)) >= A.cos_min && fabs(dp - Pj.d) <= A.d_max;
      }
      const unsigned long long mask = __ballot(cond);
      const int64_t s = il * nj - base;            // the chunk's lanes of this i begin at lo
      const int lo = s > 0 ? (int)s : 0;
      const unsigned long long mine = mask & ((1ull << lane) - 1) & ~((1ull << lo) - 1);
      const bool sel = cond && mine == 0 && !(il == carry_i && carry_m);
      const int64_t last_p = (base + 63 < npairs ? base + 63 : npairs - 1), last_i = last_p / nj, sl = last_i * nj - base;
      const bool any_last = (mask >> (sl > 0 ? (int)sl : 0)) != 0;
      carry_m = (last_i == carry_i && carry_m) || any_last;
      carry_i = last_i;
      if (sel) {
        double pe[6], d2, raw;
#pragma unroll
        for (int k = 0; k < 6; ++k) pe[k] = sm[(PC_S + k) * 64 + il];
        const bool pd = pair_distance(np, dp, pe, Pj, d2, raw);
        sm[PC_D2 * 64 + il] = pd ? d2 : __builtin_huge_val();
        sm[PC_RAW * 64 + il] = pd ? raw : __builtin_huge_val();
        sj[il] = j; sbad[il] = pd ? 0 : 1;
      }
    }
    __syncthreads();
    if (lane < cnt) {
      const int64_t g = gi0 + ib + lane;
      const int mj = sj[lane];
      const double d2 = sm[PC_D2 * 64 + lane], raw = sm[PC_RAW * 64 + lane];
      if (A.match) A.match[g] = mj;
      if (A.d2) A.d2[g] = d2;
      if (A.raw) A.raw[g] = raw;
      if (mj >= 0) {
        ++n_matched;
        if (sbad[lane]) ++n_bad;
        else if (d2 > best) { best = d2; best_raw = raw; best_i = ib + lane; best_j = mj; }
      }
    }
  }

  // the record's maximum: the larger d2, a tie to the smaller i -- what strict > in order of i keeps.  Both sides of a step
  // compare the same two candidates, so every lane ends with the same record.
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, 64), oraw = __shfl_xor(best_raw, o, 64);
    const int oi = __shfl_xor(best_i, o, 64), oj = __shfl_xor(best_j, o, 64);
    n_matched += __shfl_xor(n_matched, o, 64);
    n_bad += __shfl_xor(n_bad, o, 64);
    if (ob > best || (ob == best && oi >= 0 && oi < best_i)) { best = ob; best_raw = oraw; best_i = oi; best_j = oj; }
  }
  if (lane == 0) A.res[rec] = {FGO_PC_OK, n_matched, n_bad, best_i, best_j, 0, best, best_raw};
}

bool normals_ok(const double *abcd, int64_t first, int64_t last) {
  for (int64_t k = first; k < last; ++k) {
    const double *a = abcd + 4 * k, nn = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    if (!(nn > 0) || !std::isfinite(nn)) return false;
  }
  return true;
}

}  // namespace
}  // namespace fgo

extern "C" void fgo_plane_check_params_default(fgo_plane_check_params *p) {
  if (!p) return;
  p->cos_min = cos(10. * M_PI / 180.);
  p->d_max = 0.2;
  p->failed_info00 = 10000.0;
}

extern "C" int fgo_plane_check_vro_batch(int device, int64_t n_records, const double *pose_ij7, const double *info_ut21, const double *cov36,
                                         const int64_t *pi_ptr, const double *pi_abcd, const double *pi_cov16, const int64_t *pj_ptr,
                                         const double *pj_abcd, const double *pj_cov16, const fgo_plane_check_params *params,
                                         fgo_plane_check_result *result, int64_t *match_out, double *d2_out, double *raw_out,
                                         double *pred_abcd_out, double *pred_cov9_out, double *sdj_out) {
  using namespace fgo;
  fgo_plane_check_params P;
  fgo_plane_check_params_default(&P);
  if (params) P = *params;
  if (n_records < 0 || n_records > INT_MAX || !(P.cos_min >= -1 && P.cos_min <= 1) || !(P.d_max >= 0)) return FGO_EINVAL;
  if (n_records == 0) return FGO_OK;
  if (!pose_ij7 || !pi_ptr || !pj_ptr || !result || (info_ut21 != nullptr) == (cov36 != nullptr)) return FGO_EINVAL;
  if (!csr_ptr_ok(pi_ptr, n_records, INT_MAX) || !csr_ptr_ok(pj_ptr, n_records, INT_MAX)) return FGO_EINVAL;   // an int counts a record's planes
  const int64_t Mi = pi_ptr[n_records], Mj = pj_ptr[n_records];
  if ((Mi > 0 && (!pi_abcd || !pi_cov16)) || (Mj > 0 && (!pj_abcd || !pj_cov16))) return FGO_EINVAL;
  for (int64_t r = 0; r < n_records; ++r)
    if (!quat_ok(pose_ij7 + 7 * r + 3)) return FGO_EINVAL;
  if (!normals_ok(pi_abcd, pi_ptr[0], Mi) || !normals_ok(pj_abcd, pj_ptr[0], Mj)) return FGO_EINVAL;
  if (int rc = select_device(device)) return rc;
  const size_t n = (size_t)n_records, mi = (size_t)Mi, mj = (size_t)Mj, D = sizeof(double);
  // inputs, then the result records, then the per-plane outputs that were asked for
  Staged S;
  const int h_pose = S.in(pose_ij7, 7 * n * D), h_info = S.in(info_ut21, 21 * n * D), h_cov = S.in(cov36, 36 * n * D);
  const int h_pi_ptr = S.in(pi_ptr, (n + 1) * sizeof(int64_t)), h_pj_ptr = S.in(pj_ptr, (n + 1) * sizeof(int64_t));
  const int h_pi_abcd = S.in(pi_abcd, 4 * mi * D), h_pi_cov = S.in(pi_cov16, 16 * mi * D);
  const int h_pj_abcd = S.in(pj_abcd, 4 * mj * D), h_pj_cov = S.in(pj_cov16, 16 * mj * D);
  const int h_res = S.out(result, n * sizeof(fgo_plane_check_result));
  const int h_match = S.out(match_out, mi * sizeof(int64_t)), h_d2 = S.out(d2_out, mi * D), h_raw = S.out(raw_out, mi * D);
  const int h_pred = S.out(pred_abcd_out, 4 * mi * D), h_pred_cov = S.out(pred_cov9_out, 9 * mi * D), h_sdj = S.out(sdj_out, mi * D);
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  PcArgs A;
  A.n = n_records;
  A.pose = S.ptr<double>(h_pose); A.info = S.ptr<double>(h_info); A.cov = S.ptr<double>(h_cov);
  A.pi_ptr = S.ptr<int64_t>(h_pi_ptr); A.pj_ptr = S.ptr<int64_t>(h_pj_ptr);
  A.pi_abcd = S.ptr<double>(h_pi_abcd); A.pi_cov = S.ptr<double>(h_pi_cov);
  A.pj_abcd = S.ptr<double>(h_pj_abcd); A.pj_cov = S.ptr<double>(h_pj_cov);
  A.cos_min = P.cos_min; A.d_max = P.d_max; A.failed00 = P.failed_info00;
  A.res = S.ptr<fgo_plane_check_result>(h_res);
  A.match = S.ptr<int64_t>(h_match); A.d2 = S.ptr<double>(h_d2); A.raw = S.ptr<double>(h_raw);
  A.pred = S.ptr<double>(h_pred); A.pred_cov = S.ptr<double>(h_pred_cov); A.sdj = S.ptr<double>(h_sdj);
  hipLaunchKernelGGL(k_plane_check, dim3((unsigned)n_records), dim3(64), 0, 0, A);
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  return S.download();
}
