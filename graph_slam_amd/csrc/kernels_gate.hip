// HIP kernel (gfx950, f64, wave64) that gates candidate SE3 edges against the map's covariance: for a candidate between a and b
// with measurement Z and information Omega = L L^T, at the current estimate,
//   e, Ja, Jb   what the linearisation kernels compute for a real edge (dev::edge_se3 / dev::between_pose3)
//   chi2 = e^T Omega e
//   P    = Ja Saa Ja^T + Ja Sab Jb^T + Jb Sab^T Ja^T + Jb Sbb Jb^T          (S.. = blocks of Sigma = H^-1; zero for a fixed endpoint)
//   d2   = e^T (P + Omega^-1)^-1 e = w^T (I + L^T P L)^-1 w,  w = L^T e     (Omega^-1 is never formed)
// One launch serves every candidate of a request.  With covariances a candidate is owned by a lane group of 6 (lane = output
// row, ten candidates per wave, lanes 60..63 idle): the group's first lane evaluates the edge, factors Omega and leaves J, L, w
// in LDS; the six lanes form their rows of [Ja Jb] Sigma, P, P L and I + L^T P L (the covariance blocks are read straight from
// the resident selected inverse, or from the blocks the column solves left on the device); the first lane factors the 6x6
// result and solves.  Every 6x6 loop is unrolled with compile-time indices (no per-thread array is indexed at run time).
// Residual-only form (chi2 of edges already in the graph, candidates between fixed vertices): one lane per edge, d2 = w^T w.
// No atomics, every sum in a fixed order: results are bit-identical from call to call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_plan.hpp"
#include "pose3_device.hpp"
#include "small_dense_device.hpp"

namespace fgo {
using namespace dev;

namespace {

constexpr int GATE_G = 10;                     // lane groups of 6 in the one-wave workgroup
constexpr int GATE_LDS = 150;                  // doubles per group: Ja (later Y = P L), Jb, L, M (36 each), w (6)

__device__ __forceinline__ constexpr int ut(int r, int c) {      // index of (r, c) in the 21 upper-triangular entries, row-major
  return r <= c ? ut6(r, c) : ut6(c, r);
}

// lower Cholesky factor of the symmetric matrix whose lower triangle is a(i, j); false if a pivot is not positive (NaN included):
// the factor then carries a unit pivot there and nothing downstream divides by zero
template <class A>
__device__ __forceinline__ bool chol6(A a, double L[36]) {
  bool pd = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = a(j, j);
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j * 6 + k] * L[j * 6 + k];
    const bool ok = s > 0;
    pd = pd && ok;
    const double d = sqrt(ok ? s : 1.0);
    L[j * 6 + j] = d;
#pragma unroll
    for (int i = 0; i < j; ++i) L[i * 6 + j] = 0;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = a(i, j);
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i * 6 + k] * L[j * 6 + k];
      L[i * 6 + j] = t / d;
    }
  }
  return pd;
}

// the edge at the current estimate: e, and with JAC the Jacobians into sJa / sJb (row-major 6x6)
template <bool GTSAM, bool JAC>
__device__ __forceinline__ void gate_edge(const Pose &Xa, const Pose &Xb, const Pose &Zinv, double e[6], double *sJa, double *sJb) {
  if (GTSAM) {
    M6 Ji, Jj;
    between_pose3<JAC>(Xa, Xb, Zinv, e, Ji, Jj);
    if (JAC) {
#pragma unroll
      for (int k = 0; k < 36; ++k) { sJa[k] = Ji.m[k]; sJb[k] = Jj.m[k]; }
    }
  } else {
    EdgeLin L;
    edge_se3<JAC>(Xa, Xb, Zinv, L);
#pragma unroll
    for (int k = 0; k < 6; ++k) e[k] = L.e[k];
    if (JAC) {                                  // Ja = [[Ai, Bi], [0, Ci]], Jb = [[Aj, 0], [0, Cj]]
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          sJa[r * 6 + c] = L.Ai.m[r * 3 + c]; sJa[r * 6 + 3 + c] = L.Bi.m[r * 3 + c];
          sJa[(3 + r) * 6 + c] = 0;           sJa[(3 + r) * 6 + 3 + c] = L.Ci.m[r * 3 + c];
          sJb[r * 6 + c] = L.Aj.m[r * 3 + c]; sJb[r * 6 + 3 + c] = 0;
          sJb[(3 + r) * 6 + c] = 0;           sJb[(3 + r) * 6 + 3 + c] = L.Cj.m[r * 3 + c];
        }
    }
  }
}

template <bool GTSAM, bool COV>
__global__ __launch_bounds__(64) void k_gate(GatePlan A, const double *__restrict__ vals) {
  constexpr int PER = COV ? 6 : 1;
  __shared__ double lds[COV ? GATE_G * GATE_LDS : 1];
  const int g = threadIdx.x / PER, r = threadIdx.x - PER * g;
  const int64_t q = (int64_t)blockIdx.x * (COV ? GATE_G : 64) + g;
  const bool on = (!COV || g < GATE_G) && q < A.n;
  double *sJa = lds + (COV ? g * GATE_LDS : 0), *sJb = sJa + 36, *sL = sJa + 72, *sM = sJa + 108, *sw = sJa + 144;
  double chi = 0;
  bool pd = true;
  if (on && r == 0) {
    const double *__restrict__ rec = A.rec + GATE_REC * q;
    const Pose Xa = load_pose(vals + 8 * (int64_t)A.va[q]), Xb = load_pose(vals + 8 * (int64_t)A.vb[q]);
    const Pose Zinv = {{rec[0], rec[1], rec[2]}, {rec[3], rec[4], rec[5], rec[6]}};
    double e[6];
    gate_edge<GTSAM, COV>(Xa, Xb, Zinv, e, sJa, sJb);
    double W[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) W[k] = rec[7 + k];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = 0;
#pragma unroll
      for (int c = 0; c < 6; ++c) s += W[ut(i, c)] * e[c];
      chi += e[i] * s;
    }
    double L[36];
    pd = chol6([&](int i, int j) { return W[ut(i, j)]; }, L);
    double w[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double s = 0;
#pragma unroll
      for (int c = k; c < 6; ++c) s += L[c * 6 + k] * e[c];
      w[k] = s;
    }
    if (COV) {
#pragma unroll
      for (int k = 0; k < 36; ++k) sL[k] = L[k];
#pragma unroll
      for (int k = 0; k < 6; ++k) sw[k] = w[k];
    } else {
      double d2 = 0;
#pragma unroll
      for (int k = 0; k < 6; ++k) d2 += w[k] * w[k];
      A.out[q] = d2;
      A.out[A.n + q] = chi;
      A.out[2 * A.n + q] = pd ? 0.0 : 1.0;
    }
  }
  if (!COV) return;
  __syncthreads();
  double p[6] = {0, 0, 0, 0, 0, 0};
  if (on) {
    double ja[6], jb[6], xa[6] = {0, 0, 0, 0, 0, 0}, xb[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 6; ++c) { ja[c] = sJa[r * 6 + c]; jb[c] = sJb[r * 6 + c]; }
    // row r of Xa = Ja Saa + Jb Sab^T and Xb = Ja Sab + Jb Sbb
    const int64_t eaa = A.enc[3 * q], ebb = A.enc[3 * q + 1], eab = A.enc[3 * q + 2];
    if (eaa >= 0) {                             // (a diagonal block: symmetric, never transposed)
      const double *__restrict__ B = A.Sig + 36 * (eaa >> 1);
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int k = 0; k < 6; ++k) xa[k] += ja[c] * B[c * 6 + k];
    }
    if (eab != GATE_ZERO) {
      const int64_t code = eab >= 0 ? eab : GATE_EXTRA0 - eab;
      const double *__restrict__ B = (eab >= 0 ? A.Sig : A.extra) + 36 * (code >> 1);
      const int sr = (code & 1) ? 1 : 6, sc = (code & 1) ? 6 : 1;           // Sab(c, k) = B[c sr + k sc]
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          xb[k] += ja[c] * B[c * sr + k * sc];
          xa[k] += jb[c] * B[k * sr + c * sc];
        }
    }
    if (ebb >= 0) {
      const double *__restrict__ B = A.Sig + 36 * (ebb >> 1);
#pragma unroll
      for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int k = 0; k < 6; ++k) xb[k] += jb[c] * B[c * 6 + k];
    }
    // row r of P = Xa Ja^T + Xb Jb^T
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double s = 0;
#pragma unroll
      for (int c = 0; c < 6; ++c) s += xa[c] * sJa[k * 6 + c];
#pragma unroll
      for (int c = 0; c < 6; ++c) s += xb[c] * sJb[k * 6 + c];
      p[k] = s;
    }
    if (A.want_P) {
      double *__restrict__ o = A.out + 3 * A.n + 36 * q + 6 * r;
#pragma unroll
      for (int k = 0; k < 6; ++k) o[k] = p[k];
    }
    // row r of Y = P L (L lower triangular, zeros stored above the diagonal)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double s = 0;
#pragma unroll
      for (int c = k; c < 6; ++c) s += p[c] * sL[c * 6 + k];
      p[k] = s;
    }
  }
  __syncthreads();                              // every lane has read J: Ja's slot takes Y
  if (on) {
#pragma unroll
    for (int k = 0; k < 6; ++k) sJa[r * 6 + k] = p[k];
  }
  __syncthreads();
  if (on) {                                     // row r of M = I + L^T Y
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double s = 0;
#pragma unroll
      for (int c = 0; c < 6; ++c) s += sL[c * 6 + r] * sJa[c * 6 + k];
      sM[r * 6 + k] = s + (k == r ? 1.0 : 0.0);
    }
  }
  __syncthreads();
  if (on && r == 0) {
    double Gm[36];
    const bool pd2 = chol6([&](int i, int j) { return 0.5 * (sM[i * 6 + j] + sM[j * 6 + i]); }, Gm);
    double y[6], d2 = 0;                        // G y = w, d2 = y^T y
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = sw[i];
#pragma unroll
      for (int c = 0; c < i; ++c) s -= Gm[i * 6 + c] * y[c];
      y[i] = s / Gm[i * 6 + i];
      d2 += y[i] * y[i];
    }
    A.out[q] = d2;
    A.out[A.n + q] = chi;
    A.out[2 * A.n + q] = !pd ? 1.0 : (!pd2 ? 2.0 : 0.0);
  }
}

}  // namespace

void launch_gate(const GatePlan &A, const double *values, bool gtsam, bool with_cov, hipStream_t s) {
  if (A.n <= 0) return;
  const dim3 blk(64);
  if (with_cov) {
    const dim3 grid((unsigned)((A.n + GATE_G - 1) / GATE_G));
    if (gtsam) hipLaunchKernelGGL((k_gate<true, true>), grid, blk, 0, s, A, values);
    else hipLaunchKernelGGL((k_gate<false, true>), grid, blk, 0, s, A, values);
  } else {
    const dim3 grid((unsigned)((A.n + 63) / 64));
    if (gtsam) hipLaunchKernelGGL((k_gate<true, false>), grid, blk, 0, s, A, values);
    else hipLaunchKernelGGL((k_gate<false, false>), grid, blk, 0, s, A, values);
  }
}

}  // namespace fgo
