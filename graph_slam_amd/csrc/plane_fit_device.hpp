// What the plane kernels share (gfx950, f64, wave64).  First the plane fit of the depth-frame kernels: kernels_plane_extract.hip fits
// the planes it finds and kernels_plane_propagate.hip refits the planes it carries over with the SAME arithmetic -- the
// point-to-plane distance, the orientation rule, the total-least-squares fit and the sandwich covariance of include/fgo.h
// (fgo_plane_extract_batch).  Every function of that part is called by every thread of a workgroup of PX_T threads; every sum over
// pixels is a per-lane sum in pixel order, a butterfly inside the wave and the waves in wave order, so the result is bit-identical
// in every thread and from call to call.  Then the plane as an input and the variance of its distance after a change of frame
// (kernels_plane_check.hip, kernels_plane_propagate.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pose3_device.hpp"
#include "small_dense_device.hpp"

namespace fgo {
namespace dev {

constexpr int PX_WAVES = 4;                      // waves of a workgroup
constexpr int PX_T = 64 * PX_WAVES;
constexpr int PX_SWEEPS = 8;                     // cyclic Jacobi sweeps of the 3x3 eigenproblem (quadratic convergence: 4 - 5 reach rounding)
constexpr int PX_NSUM = 13;                      // the widest block sum: rmse, A (6), M (6)

struct Pl { double n[3], d; };

// |n.p + d| with the roundings spelled out: the scoring, the refinement and the final pass have to agree on every point
__device__ __forceinline__ double pdist(const Pl &P, double x, double y, double z) {
  return fabs(fma(P.n[0], x, fma(P.n[1], y, fma(P.n[2], z, P.d))));
}
// the camera is on the positive side
__device__ __forceinline__ void orient(Pl &P) {
  if (P.d < 0) { P.n[0] = -P.n[0]; P.n[1] = -P.n[1]; P.n[2] = -P.n[2]; P.d = -P.d; }
}

// The total-least-squares plane of the points sel names among `count` slots (sel(i) = the pixel of slot i, or -1), by every thread
// of the workgroup: the centroid, the scatter of the centred points (two passes), the eigenvector of the smallest eigenvalue.
// N = the number of points.  N == 0 leaves non-finite values behind; the callers never fit an empty set.
template <class Sel>
__device__ __forceinline__ void fit_plane(const double *__restrict__ pts, int count, Sel sel, double *red, Pl &P, double cen[3], int &N) {
  double s[4] = {0, 0, 0, 0};
  for (int i = threadIdx.x; i < count; i += PX_T) {
    const int pix = sel(i);
    if (pix < 0) continue;
    const double *p = pts + 3 * (int64_t)pix;
    s[0] += p[0]; s[1] += p[1]; s[2] += p[2]; s[3] += 1.0;
  }
  bsum<PX_WAVES>(s, red);
  N = (int)s[3];                                  // exact: at most 2^24 ones
#pragma unroll
  for (int k = 0; k < 3; ++k) cen[k] = s[k] / s[3];
  double q[6] = {0, 0, 0, 0, 0, 0};               // xx xy xz yy yz zz
  for (int i = threadIdx.x; i < count; i += PX_T) {
    const int pix = sel(i);
    if (pix < 0) continue;
    const double *p = pts + 3 * (int64_t)pix;
    const double x = p[0] - cen[0], y = p[1] - cen[1], z = p[2] - cen[2];
    q[0] += x * x; q[1] += x * y; q[2] += x * z; q[3] += y * y; q[4] += y * z; q[5] += z * z;
  }
  bsum<PX_WAVES>(q, red);
  double a[9] = {q[0], q[1], q[2], q[1], q[3], q[4], q[2], q[4], q[5]};
  double v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll 1
  for (int sweep = 0; sweep < PX_SWEEPS; ++sweep) {
    jacobi_rot<3, 0, 1>(a, v); jacobi_rot<3, 0, 2>(a, v); jacobi_rot<3, 1, 2>(a, v);
  }
  double least = a[0], e[3] = {v[0], v[3], v[6]};
#pragma unroll
  for (int k = 1; k < 3; ++k)
    if (a[4 * k] < least) { least = a[4 * k]; e[0] = v[k]; e[1] = v[3 + k]; e[2] = v[6 + k]; }
  const double nn = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
  P.n[0] = e[0] / nn; P.n[1] = e[1] / nn; P.n[2] = e[2] / nn;
  P.d = -(P.n[0] * cen[0] + P.n[1] * cen[1] + P.n[2] * cen[2]);
  orient(P);
}

__device__ __forceinline__ bool finite(double d) { return fabs(d) < __builtin_huge_val(); }

// the pixel-plus-depth noise model of a point: what sigma^2 = n^T Sigma(p) n needs
struct PxNoise { double fx, fy, s_px2, sz0, sz1, sz2; };

// The covariance of the fit P of the pixels `member` names (member(pix) = the pixel belongs to the plane) among NP pixels, N of
// them, with the centroid cen: the basis B = (b1, b2), rmse and the sandwich C = A^-1 M A^-1 (3x3, exactly symmetric) in the
// tangent [dn(2); dd].  false if A is not positive definite or a value of the plane is not finite.
template <class Member>
__device__ __forceinline__ bool fit_covariance(const double *__restrict__ pts, int NP, Member member, const Pl &P, const double cen[3], int N,
                                               const PxNoise &A, double *red, double b1[3], double b2[3], double C[9], double &rmse) {
  const int tid = threadIdx.x;
  // B = Unit3::basis(n): b1 = normalise(n x the axis of the smallest |n_i|), b2 = n x b1 (ties: x, then y, then z)
  const double mx = fabs(P.n[0]), my = fabs(P.n[1]), mz = fabs(P.n[2]);
  double ax[3] = {0, 0, 1};
  if (mx <= my && mx <= mz) { ax[0] = 1; ax[2] = 0; }
  else if (my <= mx && my <= mz) { ax[1] = 1; ax[2] = 0; }
  b1[0] = P.n[1] * ax[2] - P.n[2] * ax[1]; b1[1] = P.n[2] * ax[0] - P.n[0] * ax[2]; b1[2] = P.n[0] * ax[1] - P.n[1] * ax[0];
  const double nb = sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
  b1[0] /= nb; b1[1] /= nb; b1[2] /= nb;
  b2[0] = P.n[1] * b1[2] - P.n[2] * b1[1]; b2[1] = P.n[2] * b1[0] - P.n[0] * b1[2]; b2[2] = P.n[0] * b1[1] - P.n[1] * b1[0];
  // J = [p^T B, 1], sigma^2 = n^T Sigma(p) n: ss, A = sum J^T J (a00 a01 a02 a11 a12 a22), M = sum sigma^2 J^T J
  double s[PX_NSUM];
#pragma unroll
  for (int c = 0; c < PX_NSUM; ++c) s[c] = 0;
  for (int pix = tid; pix < NP; pix += PX_T) {
    if (!member(pix)) continue;
    const double *p = pts + 3 * (int64_t)pix;
    const double x = p[0], y = p[1], z = p[2];
    const double e = fma(P.n[0], x, fma(P.n[1], y, fma(P.n[2], z, P.d)));
    const double j0 = b1[0] * x + b1[1] * y + b1[2] * z, j1 = b2[0] * x + b2[1] * y + b2[2] * z;
    const double sz = A.sz0 + z * (A.sz1 + z * A.sz2), gx = P.n[0] * z / A.fx, gy = P.n[1] * z / A.fy;
    const double nr = P.n[0] * (x / z) + P.n[1] * (y / z) + P.n[2];
    const double v = A.s_px2 * (gx * gx + gy * gy) + sz * sz * nr * nr;
    s[0] += e * e;
    s[1] += j0 * j0; s[2] += j0 * j1; s[3] += j0; s[4] += j1 * j1; s[5] += j1; s[6] += 1.0;
    s[7] += v * j0 * j0; s[8] += v * j0 * j1; s[9] += v * j0; s[10] += v * j1 * j1; s[11] += v * j1; s[12] += v;
  }
  bsum<PX_WAVES>(s, red);
  rmse = sqrt(s[0] / (double)N);
  // A = L L^T, Ai = A^-1 = L^-T L^-1
  const bool ok0 = pivot_ok(s[1]);
  const double l00 = sqrt(ok0 ? s[1] : 1.0), l10 = s[2] / l00, l20 = s[3] / l00;
  const double d1 = s[4] - l10 * l10;
  const bool ok1 = pivot_ok(d1);
  const double l11 = sqrt(ok1 ? d1 : 1.0), l21 = (s[5] - l20 * l10) / l11;
  const double d2 = s[6] - l20 * l20 - l21 * l21;
  const bool ok2 = pivot_ok(d2);
  const double l22 = sqrt(ok2 ? d2 : 1.0);
  const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
  const double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22, i20 = -(l20 * i00 + l21 * i10) * i22;     // L^-1, lower
  double Ai[9];
  Ai[0] = i00 * i00 + i10 * i10 + i20 * i20; Ai[1] = i10 * i11 + i20 * i21; Ai[2] = i20 * i22;
  Ai[4] = i11 * i11 + i21 * i21; Ai[5] = i21 * i22; Ai[8] = i22 * i22;
  Ai[3] = Ai[1]; Ai[6] = Ai[2]; Ai[7] = Ai[5];
  const double Mm[9] = {s[7], s[8], s[9], s[8], s[10], s[11], s[9], s[11], s[12]};
  double T[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) T[3 * r + c] = Ai[3 * r] * Mm[c] + Ai[3 * r + 1] * Mm[3 + c] + Ai[3 * r + 2] * Mm[6 + c];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = r; c < 3; ++c) {
      C[3 * r + c] = T[3 * r] * Ai[c] + T[3 * r + 1] * Ai[3 + c] + T[3 * r + 2] * Ai[6 + c];
      C[3 * c + r] = C[3 * r + c];
    }
  double chk = P.n[0] + P.n[1] + P.n[2] + P.d + cen[0] + cen[1] + cen[2] + rmse;
#pragma unroll
  for (int c = 0; c < 9; ++c) chk += C[c];
  return ok0 && ok1 && ok2 && finite(chk);
}

// what one thread writes of a fitted plane: abcd (4), cov16 = E C E^T with E = [[B, 0], [0, 1]] (4x4 row-major), and, if asked
// for, the upper triangle of C
__device__ __forceinline__ void store_plane(const Pl &P, const double b1[3], const double b2[3], const double C[9], double *__restrict__ abcd,
                                            double *__restrict__ o, double *__restrict__ u) {
  abcd[0] = P.n[0]; abcd[1] = P.n[1]; abcd[2] = P.n[2]; abcd[3] = P.d;
  const double Bm[6] = {b1[0], b2[0], b1[1], b2[1], b1[2], b2[2]};     // 3x2, row-major
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double t0 = Bm[2 * r] * C[0] + Bm[2 * r + 1] * C[3], t1 = Bm[2 * r] * C[1] + Bm[2 * r + 1] * C[4];
#pragma unroll
    for (int c = r; c < 3; ++c) {
      o[4 * r + c] = t0 * Bm[2 * c] + t1 * Bm[2 * c + 1];
      o[4 * c + r] = o[4 * r + c];
    }
    o[4 * r + 3] = Bm[2 * r] * C[2] + Bm[2 * r + 1] * C[5];
    o[12 + r] = o[4 * r + 3];
  }
  o[15] = C[8];
  if (u) { u[0] = C[0]; u[1] = C[1]; u[2] = C[2]; u[3] = C[4]; u[4] = C[5]; u[5] = C[8]; }
}

// ---- a plane as the calls take it, and the variance of its distance after a change of frame (the plane check and the propagation)
// the 3x3 block (r0, c0) of the symmetric 6x6 held as its upper triangle
__device__ __forceinline__ M3 block3(const double S[21], int r0, int c0) {
  M3 B;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int r = r0 + a, c = c0 + b;
      B.m[a * 3 + b] = r <= c ? S[ut6(r, c)] : S[ut6(c, r)];
    }
  return B;
}

// (a, b, c, d) with the normal normalised, d untouched, and of CPlane::m_CP (4x4 row-major) the upper triangle of the normal block
// and entry (3, 3)
struct PlaneIn { V3 n; double d; M3 Sn; double Sd; };
__device__ __forceinline__ PlaneIn load_plane(const double *__restrict__ abcd, const double *__restrict__ cov16) {
  PlaneIn P;
  const double nn = sqrt(abcd[0] * abcd[0] + abcd[1] * abcd[1] + abcd[2] * abcd[2]);
  P.n = {abcd[0] / nn, abcd[1] / nn, abcd[2] / nn};
  P.d = abcd[3];
  P.Sn = {{cov16[0], cov16[1], cov16[2], cov16[1], cov16[5], cov16[6], cov16[2], cov16[6], cov16[10]}};
  P.Sd = cov16[15];
  return P;
}
// CGraphGT::computeSdj (gtsam/gtsam_graph.cpp:725-748): S_dj = S_di + n^T S_t n + g^T S_ni g, g = (I - n n^T) t, for the plane carried
// through a pose with translation t whose covariance block is S_t
__device__ __forceinline__ double predicted_sdj(const PlaneIn &P, V3 t, const M3 &St) {
  const double nt = dot3(P.n, t);
  const V3 gv = {t.x - P.n.x * nt, t.y - P.n.y * nt, t.z - P.n.z * nt};
  return P.Sd + dot3(P.n, mv(St, P.n)) + dot3(gv, mv(P.Sn, gv));
}

}  // namespace dev
}  // namespace fgo
