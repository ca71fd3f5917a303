// HIP kernels (gfx950, f64, wave64) that gate candidate plane observations against the map's covariance (GTSAM semantics): for a
// candidate between pose x and plane p (already a variable) with measurement z = (n_z, d_z) in the pose frame and covariance S,
// at the current estimate,
//   e (3), Jx (3x6), Jp (3x3)   what dev::plane_factor<true> gives the linearisation of a real OrientedPlane3Factor
//   chi2 = e^T S^-1 e
//   P    = Jx Sxx Jx^T + Jx Sxp Jp^T + Jp Sxp^T Jx^T + Jp Spp Jp^T       (S.. = blocks of Sigma = H^-1; zero for a fixed endpoint)
//   d2   = e^T (P + S)^-1 e                                              (S is a covariance: P + S is factored as it stands)
//   cosn = n'^T n_z                                                      (n' = R^T n, the predicted normal)
// One launch serves every candidate of a request.  A candidate is owned by a lane group of 3 (lane = residual row, 21 candidates
// per wave, lane 63 idle): the group's first lane evaluates the factor, factors S for chi2 and leaves J, e in LDS; the three
// lanes form their rows of [Jx Jp] Sigma and of P + S (covariance blocks are read straight from the resident selected inverse, or
// from the blocks the column solves left on the device; of a plane's padded 6-block only the leading 3 rows / columns are
// read); the first lane factors the 3x3 result and solves.  Every small loop is unrolled with compile-time indices (no per-thread
// array is indexed at run time), no atomics, every sum in a fixed order: results are bit-identical from call to call and do not
// depend on a candidate's position in the batch.
// k_plane_assoc reduces the candidates of one pose against m planes per observation: smallest and second smallest d2 in the order
// of the plane list (a tie goes to the earlier entry), one lane per observation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_plan.hpp"
#include "factors_device.hpp"
#include "small_dense_device.hpp"

namespace fgo {
using namespace dev;

namespace {

constexpr int PG_G = 21;                       // lane groups of 3 in the one-wave workgroup
constexpr int PG_LDS = 39;                     // doubles per group: Jx (18), Jp (9), M = P + S (9), e (3)

__global__ __launch_bounds__(64) void k_plane_gate(PlaneGatePlan A, const double *__restrict__ vals) {
  __shared__ double lds[PG_G * PG_LDS];
  const int g = threadIdx.x / 3, r = threadIdx.x - 3 * g;
  const int64_t q = (int64_t)blockIdx.x * PG_G + g;
  const bool on = g < PG_G && q < A.n;
  double *sJx = lds + (g < PG_G ? g : 0) * PG_LDS, *sJp = sJx + 18, *sM = sJx + 27, *se = sJx + 36;
  const double *__restrict__ rec = A.rec + PGATE_REC * (on ? q : 0);
  double chi = 0, cosn = 0;
  bool pd = true;
  if (on && r == 0) {
    const Pose X = load_pose(vals + 8 * (int64_t)A.vx[q]);
    const double4 pl = *reinterpret_cast<const double4 *>(vals + 8 * (int64_t)A.vp[q]);
    const V3 nz = {rec[0], rec[1], rec[2]};
    double e[6];
    M6 Jx, Jp;
    plane_factor<true>(X, V3{pl.x, pl.y, pl.z}, pl.w, nz, rec[3], e, Jx, Jp);
    cosn = Jx.m[15] * nz.x + Jx.m[16] * nz.y + Jx.m[17] * nz.z;      // (row 2 of Jx carries n' = R^T n in its translation part)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int c = 0; c < 6; ++c) sJx[i * 6 + c] = Jx.m[i * 6 + c];
#pragma unroll
      for (int c = 0; c < 3; ++c) sJp[i * 3 + c] = Jp.m[i * 6 + c];
      se[i] = e[i];
    }
    double ls[6];
    pd = chol3(rec[4], rec[5], rec[7], rec[6], rec[8], rec[9], ls);
    chi = solve3_sq(ls, e[0], e[1], e[2]);
  }
  __syncthreads();
  if (on) {
    double jx[6], jp[3], xx[6] = {0, 0, 0, 0, 0, 0}, xp[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < 6; ++c) jx[c] = sJx[r * 6 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) jp[c] = sJp[r * 3 + c];
    // row r of Xx = Jx Sxx + Jp Sxp^T (6) and Xp = Jx Sxp + Jp Spp (3)
    const int64_t exx = A.enc[3 * q], epp = A.enc[3 * q + 1], exp_ = A.enc[3 * q + 2];
    if (exx >= 0) {                             // (a diagonal block: symmetric, never transposed)
      const double *__restrict__ B = A.Sig + 36 * (exx >> 1);
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int k = 0; k < 6; ++k) xx[k] += jx[c] * B[c * 6 + k];
    }
    if (exp_ != GATE_ZERO) {
      const int64_t code = exp_ >= 0 ? exp_ : GATE_EXTRA0 - exp_;
      const double *__restrict__ B = (exp_ >= 0 ? A.Sig : A.extra) + 36 * (code >> 1);
      const int sr = (code & 1) ? 1 : 6, sc = (code & 1) ? 6 : 1;           // Sxp(c, k) = B[c sr + k sc], c < 6, k < 3
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) xp[k] += jx[c] * B[c * sr + k * sc];
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 6; ++k) xx[k] += jp[c] * B[k * sr + c * sc];
    }
    if (epp >= 0) {                             // (the leading 3x3 of the plane's block; its identity padding is never read)
      const double *__restrict__ B = A.Sig + 36 * (epp >> 1);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) xp[k] += jp[c] * B[c * 6 + k];
    }
    // row r of P = Xx Jx^T + Xp Jp^T, then of M = P + S
    double p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double s = 0;
#pragma unroll
      for (int c = 0; c < 6; ++c) s += xx[c] * sJx[k * 6 + c];
#pragma unroll
      for (int c = 0; c < 3; ++c) s += xp[c] * sJp[k * 3 + c];
      p[k] = s;
    }
    if (A.want_P) {
      double *__restrict__ o = A.out + 7 * A.n + 9 * q + 3 * r;
#pragma unroll
      for (int k = 0; k < 3; ++k) o[k] = p[k];
    }
    // row r of S from its upper triangle s00 s01 s02 s11 s12 s22 (rec[4..9])
    const double s0 = r == 0 ? rec[4] : (r == 1 ? rec[5] : rec[6]);
    const double s1 = r == 0 ? rec[5] : (r == 1 ? rec[7] : rec[8]);
    const double s2 = r == 0 ? rec[6] : (r == 1 ? rec[8] : rec[9]);
    sM[r * 3 + 0] = p[0] + s0;
    sM[r * 3 + 1] = p[1] + s1;
    sM[r * 3 + 2] = p[2] + s2;
  }
  __syncthreads();
  if (on && r == 0) {
    double lm[6];
    const bool pd2 = chol3(sM[0], 0.5 * (sM[3] + sM[1]), sM[4], 0.5 * (sM[6] + sM[2]), 0.5 * (sM[7] + sM[5]), sM[8], lm);
    A.out[q] = solve3_sq(lm, se[0], se[1], se[2]);
    A.out[A.n + q] = chi;
    A.out[2 * A.n + q] = cosn;
    A.out[3 * A.n + q] = !pd ? 1.0 : (!pd2 ? 2.0 : 0.0);
    A.out[4 * A.n + 3 * q] = se[0];
    A.out[4 * A.n + 3 * q + 1] = se[1];
    A.out[4 * A.n + 3 * q + 2] = se[2];
  }
}

// Observation i against the planes j = 0 .. m-1 (candidate j k + i of the gate's output): an excluded candidate (cos below
// cos_min, S or P + S not positive definite) counts as +inf.  res: [k] position of the match in the plane list or -1 | [k][2]
// smallest, second smallest d2 | [k][m] the d2 matrix (want_matrix)
__global__ __launch_bounds__(64) void k_plane_assoc(const double *__restrict__ gate, int64_t k, int64_t m, double d2_gate, double cos_min,
                                                    int want_matrix, double *__restrict__ res) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= k) return;
  const int64_t n = k * m;
  const double inf = __builtin_huge_val();
  double b0 = inf, b1 = inf;
  int64_t j0 = -1;
  for (int64_t j = 0; j < m; ++j) {
    const int64_t q = j * k + i;
    const bool in = gate[3 * n + q] == 0.0 && gate[2 * n + q] >= cos_min;
    const double d = in ? gate[q] : inf;
    if (want_matrix) res[3 * k + i * m + j] = d;
    if (d < b0) { b1 = b0; b0 = d; j0 = j; }
    else if (d < b1) b1 = d;
  }
  res[i] = b0 < d2_gate ? (double)j0 : -1.0;
  res[k + 2 * i] = b0;
  res[k + 2 * i + 1] = b1;
}

}  // namespace

void launch_plane_gate(const PlaneGatePlan &A, const double *values, hipStream_t s) {
  if (A.n <= 0) return;
  hipLaunchKernelGGL(k_plane_gate, dim3((unsigned)((A.n + PG_G - 1) / PG_G)), dim3(64), 0, s, A, values);
}

void launch_plane_assoc(const double *gate_out, int64_t k, int64_t m, double d2_gate, double cos_min, bool want_matrix, double *res, hipStream_t s) {
  if (k <= 0) return;
  hipLaunchKernelGGL(k_plane_assoc, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, s, gate_out, k, m, d2_gate, cos_min, want_matrix ? 1 : 0, res);
}

}  // namespace fgo
