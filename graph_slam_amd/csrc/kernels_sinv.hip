// HIP kernels (gfx950, f64, wave64) of the selected inversion: H^-1 on the block pattern of the resident undamped factor
// L (H = L L^T in elimination order), the Takahashi recursion behind g2o's computeMarginals and GTSAM's Marginals.
// For column j with off-diagonal block rows S_j = {r_0 < ... < r_{m-1}} and U_qj = L_(r_q, j) L_jj^-1:
//   Sigma_(r_p, j) = - sum_q Sigma_(r_p, r_q) U_qj                 (Sigma_(r_p, r_q) = Sigma_(r_q, r_p)^T when q > p)
//   Sigma_jj       = L_jj^-T L_jj^-1 - sum_q Sigma_(r_q, j)^T U_qj
// Every Sigma on the right belongs to an ancestor of j (S_j is a clique of the filled graph), so the columns run in the reverse
// of the elimination: levels from the root down, inside a task its columns last to first.
//   k_sinv_prep    per column: D = L_jj^-1, C_j = D^T D (into U's diagonal slot), U = L_kj D for its off-diagonal blocks
//   k_sinv_sweep   one launch per level, one workgroup per task: a column's off-diagonal targets are owned by lane groups of 6
//                  (lane = output row) and gathered over the column's pair table in ascending q; then its diagonal block, the
//                  lane groups' partial sums combined in a fixed order
//   k_sinv_gather  the requested blocks (or their transposes) into one dense array for the copy to the host
//   k_sinv_rows    the rows of a column solve that the off-pattern pairs need (fgo_marginal_cov_pairs' fallback)
// No floating-point atomics, every sum in a fixed order: results are bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_plan.hpp"
#include "fgo_internal.hpp"

namespace fgo {

namespace {

constexpr int PREP_G = SINV_PREP_COLS;

__global__ __launch_bounds__(256) void k_sinv_prep(SinvPlan Q, const double *__restrict__ Lv, double *__restrict__ U) {
  __shared__ double sD[PREP_G * 36];
  const int g = threadIdx.x / 6, r = threadIdx.x - 6 * g;
  const int j = blockIdx.x * PREP_G + g;
  const bool on = g < PREP_G && j < Q.nb;
  int64_t b0 = 0, b1 = 0;
  if (on) {
    b0 = Q.colptr[j]; b1 = Q.colptr[j + 1];
    const double *Ld = Lv + 36 * b0;
    // lane r: column r of D, L_jj d = e_r by forward substitution
    double d[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = i == r ? 1.0 : 0.0;
#pragma unroll
      for (int c = 0; c < i; ++c) s -= Ld[i * 6 + c] * d[c];
      d[i] = s / Ld[i * 6 + i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) sD[36 * g + i * 6 + r] = d[i];
  }
  __syncthreads();
  if (!on) return;
  const double *D = sD + 36 * g;
  double *Uo = U + 36 * b0 + 6 * r;
#pragma unroll
  for (int b = 0; b < 6; ++b) {                       // C_j = D^T D, row r
    double s = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) s += D[c * 6 + r] * D[c * 6 + b];
    Uo[b] = s;
  }
  for (int64_t t = b0 + 1; t < b1; ++t) {             // U = L_kj D, row r (D lower triangular)
    const double *Lt = Lv + 36 * t + 6 * r;
    double l[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) l[c] = Lt[c];
    double *Ut = U + 36 * t + 6 * r;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      double s = 0;
#pragma unroll
      for (int c = b; c < 6; ++c) s += l[c] * D[c * 6 + b];
      Ut[b] = s;
    }
  }
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void k_sinv_sweep(SinvPlan Q, int task0) {
  constexpr int G = NW * SINV_WAVE_GROUPS;            // lane groups of 6: 10 per wave, lanes 60..63 idle
  __shared__ double sred[G * 36];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = lane / 6, r = lane - 6 * gl;
  const bool act = lane < 60;
  const int grp = wave * 10 + gl;
  const int task = task0 + blockIdx.x;
  const int c_begin = Q.task_ptr[task], c_end = Q.task_ptr[task + 1];
  double *__restrict__ Sig = Q.Sig;
  for (int ci = c_end - 1; ci >= c_begin; --ci) {
    const int j = Q.task_cols[ci];
    const int64_t b0 = Q.colptr[j];
    const int m = (int)(Q.colptr[j + 1] - b0 - 1);
    const int *__restrict__ E = Q.sidx + Q.sptr[j];
    const double *__restrict__ Uj = Q.U + 36 * (b0 + 1);
    if (act)
      for (int p = grp; p < m; p += G) {
        double acc[6] = {0, 0, 0, 0, 0, 0};
        const int64_t rowp = (int64_t)p * (p + 1) / 2;
        for (int q = 0; q < m; ++q) {
          double s[6];
          if (q <= p) {                               // Sigma_(r_p, r_q): row r of the block
            const double *B = Sig + 36 * (int64_t)E[rowp + q] + 6 * r;
#pragma unroll
            for (int c = 0; c < 6; ++c) s[c] = B[c];
          } else {                                    // Sigma_(r_q, r_p)^T: column r of the block
            const double *B = Sig + 36 * (int64_t)E[(int64_t)q * (q + 1) / 2 + p] + r;
#pragma unroll
            for (int c = 0; c < 6; ++c) s[c] = B[6 * c];
          }
          const double *Uq = Uj + 36 * q;
#pragma unroll
          for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int b = 0; b < 6; ++b) acc[b] += s[c] * Uq[c * 6 + b];
        }
        double *O = Sig + 36 * (b0 + 1 + p) + 6 * r;
#pragma unroll
        for (int b = 0; b < 6; ++b) O[b] = -acc[b];
      }
    __syncthreads();
    // diagonal: lane group grp sums q = grp, grp + G, ... of Sigma_(r_q, j)^T U_qj; the partials are combined in group order
    double acc[6] = {0, 0, 0, 0, 0, 0};
    if (act)
      for (int q = grp; q < m; q += G) {
        const double *B = Sig + 36 * (b0 + 1 + q) + r;
        double s[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c] = B[6 * c];
        const double *Uq = Uj + 36 * q;
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
          for (int b = 0; b < 6; ++b) acc[b] += s[c] * Uq[c * 6 + b];
      }
    if (act) {
#pragma unroll
      for (int b = 0; b < 6; ++b) sred[grp * 36 + r * 6 + b] = acc[b];
    }
    __syncthreads();
    if (threadIdx.x < 36) {
      double v = Q.U[36 * b0 + threadIdx.x];
      for (int g = 0; g < G; ++g) v -= sred[g * 36 + threadIdx.x];
      Sig[36 * b0 + threadIdx.x] = v;
    }
    __syncthreads();
  }
}

// out[i] = block (enc[i] >> 1) of Sigma, transposed when enc[i] & 1
__global__ __launch_bounds__(256) void k_sinv_gather(const int64_t *__restrict__ enc, int64_t n, const double *__restrict__ Sig,
                                                     double *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 36) return;
  const int64_t i = t / 36;
  const int e = (int)(t - 36 * i);
  const int64_t code = enc[i];
  const double *B = Sig + 36 * (code >> 1);
  out[t] = (code & 1) ? B[(e % 6) * 6 + e / 6] : B[e];
}

// out[i * istride + r * rstride] = x[6 cols[i] + r]: the rows of a column solve that a group of off-pattern pairs needs (6 / 1:
// packed for the copy to the host; 36 / 6: column k of row-major blocks that stay on the device, out offset by k)
__global__ __launch_bounds__(256) void k_sinv_rows(const int *__restrict__ cols, int64_t n, const double *__restrict__ x,
                                                   double *__restrict__ out, int64_t istride, int64_t rstride) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 6) return;
  const int64_t i = t / 6, r = t - 6 * i;
  out[i * istride + r * rstride] = x[6 * (int64_t)cols[i] + r];
}

}  // namespace

void launch_sinv_prep(const SinvPlan &Q, const double *Lv, double *U, hipStream_t s) {
  if (Q.nb > 0) hipLaunchKernelGGL(k_sinv_prep, dim3(sinv_prep_workgroups(Q.nb)), dim3(256), 0, s, Q, Lv, U);
}

// levels from the root down; a level with fewer tasks than the device has compute units gets 16-wave workgroups (the
// columns near the root have the longest patterns and nothing else runs beside them), a wide one 4-wave workgroups
// (sinv_sweep_waves, which fgo_debug_selinv_census asks too; FGO_TUNE sinv_wide moves the threshold).
// (Measured at config 2: 8-wave workgroups with four or eight terms of a gather in flight were slower -- sweep 70.2 / 67.4 ms
// against 55.4 ms: the narrow levels need lane groups for more targets of a column more than deeper pipelining of each.
// Two targets per lane group, every U element loaded feeding both, was slower too: 59.3 ms.)
void launch_sinv_sweep(const SinvPlan &Q, const HostSchedule &H, hipStream_t s) {
  for (int l = H.n_levels - 1; l >= 0; --l) {
    const int t0 = H.level_ptr[l], nt = H.level_ptr[l + 1] - t0;
    if (nt <= 0) continue;
    if (sinv_sweep_waves(nt, H.cus) == 16) hipLaunchKernelGGL(k_sinv_sweep<16>, dim3(nt), dim3(16 * 64), 0, s, Q, t0);
    else hipLaunchKernelGGL(k_sinv_sweep<4>, dim3(nt), dim3(4 * 64), 0, s, Q, t0);
  }
}

void launch_sinv_gather(const int64_t *enc, int64_t n, const double *Sig, double *out, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_sinv_gather, dim3((unsigned)((n * 36 + 255) / 256)), dim3(256), 0, s, enc, n, Sig, out);
}

void launch_sinv_rows(const int *cols, int64_t n, const double *x, double *out, hipStream_t s, int64_t istride, int64_t rstride) {
  if (n > 0) hipLaunchKernelGGL(k_sinv_rows, dim3((unsigned)((n * 6 + 255) / 256)), dim3(256), 0, s, cols, n, x, out, istride, rstride);
}

}  // namespace fgo
