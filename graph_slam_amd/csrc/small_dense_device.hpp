// Device-side small dense numerics shared by the batched front-end kernels (gfx950, f64, wave64): the wave and workgroup sums, the wave-aggregated counter,
// the counter-based RANSAC sampler, packed-triangle indexing, the 3x3 and 6x6 Cholesky helpers and the cyclic Jacobi rotation.
// Everything is fully unrolled with compile-time indices, so a caller that reads only part of a result pays only for that part.
//
// Near-relatives that are NOT here, because their storage or pivot rule differs and different rules mean different code:
//   chol6      (kernels_gate.hip)           full 36-entry storage with the zeros above the diagonal written, functor input, pivot > 0
//   chol6_lds  (kernels_factor.hip)         the factor sweep's 6x6 block read from LDS: right-looking, rsqrt, returns 1 / L_jj
//   chol12     (kernels_two_view.hip)       12x12, multiplies by 1 / l, no unit pivot on failure
//   the 6x6 covariance of kernels_vro_ransac.hip (the steps of inv6 with the status seeded by the wave's `bad` flag and the full
//   square as output) and of kernels_two_view.hip (L^-1 and L^-T L^-1 of the 12x12 factor's trailing block, fused with L L^T):
//   both were tried on chol6_packed / tri6_inverse and both kernels' instruction streams moved, so they keep their own loops
//   pt_factor  (kernels_two_view.hip)       3x3 that returns L^-1 directly
//   the 3x3 inverse of plane_fit_device.hpp and the 3x3 factors of kernels_imu_check.hip / kernels_vro_ransac.hip, which
//   test their pivots with pivot_ok where chol3 tests > 0 only
//   bsum4      (kernels_gtsam.hip), block_sum (kernels.hip)   one value, one barrier before the read and one after; bsum below
//   puts its first barrier before the write
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fgo {
namespace dev {

// The xor butterfly over the 64 lanes of a wave.  Each step combines the same two numbers on both sides of the exchange, and +
// and max are commutative, so every lane ends with the same bits: a decision taken on the result is wave-uniform without a
// broadcast.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// Counts the lanes that get here: the first of them adds their number, one atomic per wave and call.  (One atomicAdd of 1 per lane,
// all on one address, measured 12 ns per POINT in a kernel that counted the kept points of a map: nine tenths of the call.)
__device__ __forceinline__ void wave_count(long long *counter) {
  const unsigned long long m = __ballot(1);
  if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1)
    atomicAdd(reinterpret_cast<unsigned long long *>(counter), (unsigned long long)__popcll(m));
}

// the sums of a workgroup of W waves: butterfly inside a wave, the waves in wave order; two barriers, the first lets the readers
// of the previous sum finish.  red holds W * N values.  Every thread of the workgroup has to call it.
template <int W, class T, int N>
__device__ __forceinline__ void bsum(T (&v)[N], T *red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < N; ++c) v[c] = wave_sum(v[c]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < N; ++c) red[wave * N + c] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < N; ++c) {
    T t = red[c];
#pragma unroll
    for (int w = 1; w < W; ++w) t += red[w * N + c];
    v[c] = t;
  }
}

// ---- RANSAC: the sampler tests/vro_ransac_reference.py and tests/plane_extract_reference.py restate
__device__ __forceinline__ uint64_t mix(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// three distinct indices below M >= 3 from the counter-based hash; counter = the hypothesis (with the round folded in, if any)
__device__ __forceinline__ void sample3(uint64_t seed, uint64_t counter, int M, int &a, int &b, int &c) {
  const uint64_t g = 0x9E3779B97F4A7C15ull, k0 = 3ull * counter + 1ull;
  a = (int)(mix(seed + k0 * g) % (uint64_t)M);
  b = (int)(mix(seed + (k0 + 1) * g) % (uint64_t)(M - 1));
  b += b >= a;
  c = (int)(mix(seed + (k0 + 2) * g) % (uint64_t)(M - 2));
  c += c >= min(a, b);
  c += c >= max(a, b);
}
// larger count first, then the lower hypothesis
__device__ __forceinline__ void better(int &cnt, int &h, int cnt2, int h2) {
  if (cnt2 > cnt || (cnt2 == cnt && h2 < h)) { cnt = cnt2; h = h2; }
}

// ---- packed triangles and pivots
__device__ __forceinline__ constexpr int lt(int r, int c) { return r * (r + 1) / 2 + c; }                // lower triangle packed by rows, c <= r
__device__ __forceinline__ constexpr int ut6(int r, int c) { return r * 6 - r * (r - 1) / 2 + c - r; }   // upper triangle of a 6x6, by rows, r <= c
__device__ __forceinline__ bool pivot_ok(double d) { return d > 0 && d < __builtin_huge_val(); }         // positive and finite (NaN fails)

// ---- 3x3
// lower Cholesky factor (l00 l10 l11 l20 l21 l22) of the symmetric 3x3 matrix a00 a10 a11 a20 a21 a22; false if a pivot is not
// positive (NaN included): the factor then carries a unit pivot there and nothing downstream divides by zero
__device__ __forceinline__ bool chol3(double a00, double a10, double a11, double a20, double a21, double a22, double l[6]) {
  const bool ok0 = a00 > 0;
  l[0] = sqrt(ok0 ? a00 : 1.0);
  l[1] = a10 / l[0];
  l[3] = a20 / l[0];
  const double s1 = a11 - l[1] * l[1];
  const bool ok1 = s1 > 0;
  l[2] = sqrt(ok1 ? s1 : 1.0);
  l[4] = (a21 - l[3] * l[1]) / l[2];
  const double s2 = a22 - l[3] * l[3] - l[4] * l[4];
  const bool ok2 = s2 > 0;
  l[5] = sqrt(ok2 ? s2 : 1.0);
  return ok0 && ok1 && ok2;
}
// y = L^-1 e, returns y^T y = e^T (L L^T)^-1 e
__device__ __forceinline__ double solve3_sq(const double l[6], double e0, double e1, double e2) {
  const double y0 = e0 / l[0];
  const double y1 = (e1 - l[1] * y0) / l[2];
  const double y2 = (e2 - l[3] * y0 - l[4] * y1) / l[5];
  return y0 * y0 + y1 * y1 + y2 * y2;
}

// ---- 6x6, packed: A = L L^T, L^-1, A^-1 = L^-T L^-1
// the lower Cholesky factor L (packed by rows) of the symmetric 6x6 A given by its upper triangle (by rows); false if a pivot is
// <= 0 or not finite: the factor then carries a unit pivot there and nothing downstream divides by zero
__device__ __forceinline__ bool chol6_packed(const double *__restrict__ a_ut, double L[21]) {
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) L[lt(r, c)] = a_ut[ut6(c, r)];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = L[lt(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[lt(j, k)] * L[lt(j, k)];
    const bool okj = pivot_ok(d);
    ok = ok && okj;
    const double l = sqrt(okj ? d : 1.0);
    L[lt(j, j)] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = L[lt(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[lt(i, k)] * L[lt(j, k)];
      L[lt(i, j)] = s / l;
    }
  }
  return ok;
}
// Mi = L^-1 (lower, packed by rows) of a lower triangular L (packed by rows)
__device__ __forceinline__ void tri6_inverse(const double L[21], double Mi[21]) {
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    Mi[lt(c, c)] = 1.0 / L[lt(c, c)];
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      double s = 0;
#pragma unroll
      for (int k = c; k < r; ++k) s += L[lt(r, k)] * Mi[lt(k, c)];
      Mi[lt(r, c)] = -s / L[lt(r, r)];
    }
  }
}
// S = A^-1 = L^-T L^-1 (upper triangle, by rows) of the symmetric 6x6 A given by its upper triangle; false if a pivot is <= 0 or
// not finite.  The last step stays in this function: as a routine of its own it moves the pivot tests in the callers' instruction
// streams.
__device__ __forceinline__ bool inv6(const double *__restrict__ a_ut, double S[21]) {
  double L[21], Mi[21];
  const bool ok = chol6_packed(a_ut, L);
  tri6_inverse(L, Mi);
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) {
      double s = 0;
#pragma unroll
      for (int k = c; k < 6; ++k) s += Mi[lt(k, r)] * Mi[lt(k, c)];
      S[ut6(r, c)] = s;
    }
  return ok;
}

// ---- one cyclic Jacobi rotation on the symmetric NxN a (full storage) with the eigenvectors accumulated in the columns of v
template <int N, int P, int Q>
__device__ __forceinline__ void jacobi_rot(double a[N * N], double v[N * N]) {
  const double apq = a[N * P + Q];
  if (apq == 0.0) return;
  const double theta = (a[N * Q + Q] - a[N * P + P]) / (2.0 * apq);
  const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
  for (int k = 0; k < N; ++k) {                    // columns P, Q
    const double akp = a[N * k + P], akq = a[N * k + Q];
    a[N * k + P] = c * akp - s * akq;
    a[N * k + Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {                    // rows P, Q
    const double apk = a[N * P + k], aqk = a[N * Q + k];
    a[N * P + k] = c * apk - s * aqk;
    a[N * Q + k] = s * apk + c * aqk;
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double vkp = v[N * k + P], vkq = v[N * k + Q];
    v[N * k + P] = c * vkp - s * vkq;
    v[N * k + Q] = s * vkp + c * vkq;
  }
}

}  // namespace dev
}  // namespace fgo
