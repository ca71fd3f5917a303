// Dense depth alignment of key-frame pairs on the MI355X (gfx950, f64, wave64): projective point-to-plane ICP of the two depth
// frames of a pair, coarse to fine, with the information of the result -- what fgo_vro_ransac_batch returns, for the pairs whose
// feature registration failed.  An ICP is not in the reference; include/fgo_dense.h states the semantics this file implements and
// tests/depth_align_reference.py restates them in numpy.  The pairs are independent: fgo_depth_align_batch runs ONE WORKGROUP PER
// PAIR (4 waves) and the whole coarse-to-fine loop of all pairs in ONE launch.
//
//   stage     lds form: the target frame's depth words are copied into LDS once (176 x 144: 50 688 bytes); global form: they stay
//             where they are.  Nothing else of a frame is kept: points and normals are recomputed from the words at every look-up,
//             so there is no per-frame point or normal map in HBM.
//   evaluate  a lane takes the sampled source pixels tid, tid + 256, ... of the level in pixel order (neighbouring lanes read
//             neighbouring samples of a row), moves the point, rounds its projection, gathers the target word and its four
//             normal neighbours, applies the gates and adds w J^T J, w J^T r, w r^2, r^2 and 1 to its 30 running sums.
//   reduce    dev::bsum: butterfly inside a wave, the waves in wave order through LDS; every thread holds the totals.
//   solve     wave 0 alone (every lane the same numbers): the scaled 6x6 Cholesky of small_dense_device.hpp, the pivots, the step,
//             the retraction of pose3_device.hpp; lane 0 leaves the pose and what to do next in LDS for the other waves.
// Every branch that holds a barrier is uniform over the workgroup: the level and iteration counts come from the arguments, the
// status and the convergence flag from LDS.  No atomics.  The file is compiled with contraction off, the shared helpers included.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include <cmath>
#include <vector>
#include "../../include/fgo_dense.h"
#include "small_dense_device.hpp"
#include "pose3_device.hpp"
#include "batch_call.hpp"

namespace fgo {
using namespace dev;

namespace {

constexpr int DA_T = 256, DA_W = 4;           // threads and waves of a workgroup
constexpr int DA_NS = 30;                     // H (21), g (6), chi2, ss, count
constexpr int DA_G = 21, DA_CHI2 = 27, DA_SS = 28, DA_CNT = 29;
constexpr int DA_LDS_BYTES = 60 * 1024;       // the largest frame the lds form stages (with the static LDS below: under 64 KB)

struct DaArgs {
  int W, H;
  const uint16_t *depth;
  const int64_t *fi, *fj;
  const double *init;                         // n x 7, normalised on the host; NULL = identity
  double fx, fy, cx, cy, z_scale, z_min, z_max, s_px2, sz0, sz1, sz2;
  int n_levels, skip[3], iters[3], step, min_pairs;
  double jump, max_dist, min_cos, eps_rot, eps_trans, min_pivot;
  double *pose, *info, *cov, *neq;            // info / cov / neq may be NULL
  fgo_depth_align_result *res;
};

__device__ __forceinline__ double da_z(const DaArgs &A, uint16_t w, bool &ok) {
  const double z = (double)w * A.z_scale;
  ok = z > A.z_min && z < A.z_max;
  return z;
}
__device__ __forceinline__ void da_xy(const DaArgs &A, int u, int v, double z, double p[3]) {
  p[0] = (((double)u - A.cx) * z) / A.fx;
  p[1] = (((double)v - A.cy) * z) / A.fy;
  p[2] = z;
}
__device__ __forceinline__ double da_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// sigma^2 = n^T Sigma(p) n of the pixel + depth model (Sigma = G diag(s_px2, s_px2, sigma_z(z)^2) G^T as the RANSAC's point_cov
// builds it): a scalar, so no 3x3 factor is needed
__device__ __forceinline__ double da_sigma2(const DaArgs &A, const double n[3], const double p[3]) {
  const double z = p[2], sz = A.sz0 + z * (A.sz1 + z * A.sz2), gx = (n[0] * z) / A.fx, gy = (n[1] * z) / A.fy;
  const double nr = (n[0] * (p[0] / z) + n[1] * (p[1] / z)) + n[2];
  return A.s_px2 * (gx * gx + gy * gy) + (sz * sz) * (nr * nr);
}

// the target's point and normal at (u, v), from the depth words at tg (LDS or global); false if either is invalid
__device__ __forceinline__ bool da_target(const DaArgs &A, const uint16_t *tg, int u, int v, double p[3], double n[3]) {
  const int s = A.step;
  if (u - s < 0 || u + s >= A.W || v - s < 0 || v + s >= A.H) return false;
  const int o = v * A.W + u, sv = s * A.W;
  bool okc, okl, okr, oku, okd;
  const double zc = da_z(A, tg[o], okc), zl = da_z(A, tg[o - s], okl), zr = da_z(A, tg[o + s], okr);
  const double zu = da_z(A, tg[o - sv], oku), zd = da_z(A, tg[o + sv], okd);
  if (!(okc && okl && okr && oku && okd)) return false;
  if (fabs(zl - zc) > A.jump || fabs(zr - zc) > A.jump || fabs(zu - zc) > A.jump || fabs(zd - zc) > A.jump) return false;
  double pl[3], pr[3], pu[3], pd[3];
  da_xy(A, u, v, zc, p);
  da_xy(A, u - s, v, zl, pl); da_xy(A, u + s, v, zr, pr); da_xy(A, u, v - s, zu, pu); da_xy(A, u, v + s, zd, pd);
  const double a[3] = {pr[0] - pl[0], pr[1] - pl[1], pr[2] - pl[2]}, b[3] = {pd[0] - pu[0], pd[1] - pu[1], pd[2] - pu[2]};
  const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double l = sqrt(da_dot(c, c));
  if (!(l > 0)) return false;
  n[0] = c[0] / l; n[1] = c[1] / l; n[2] = c[2] / l;
  if (da_dot(n, p) > 0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
  return true;
}

// one evaluation at X on the level of stride k: this lane's share of the 30 sums
__device__ __forceinline__ void da_evaluate(const DaArgs &A, const uint16_t *__restrict__ src, const uint16_t *tg, const Pose &X, int k, double acc[DA_NS]) {
#pragma unroll
  for (int c = 0; c < DA_NS; ++c) acc[c] = 0;
  const M3 R = qmat(X.q);
  const double t[3] = {X.t.x, X.t.y, X.t.z};
  const int sw = (A.W + k - 1) / k, sh = (A.H + k - 1) / k, ns = sw * sh;
  for (int s = threadIdx.x; s < ns; s += DA_T) {
    const int vs = s / sw, u = (s - vs * sw) * k, v = vs * k;
    bool ok;
    const double z = da_z(A, src[v * A.W + u], ok);
    if (!ok) continue;
    double pj[3], q[3];
    da_xy(A, u, v, z, pj);
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = ((R.m[3 * c] * pj[0] + R.m[3 * c + 1] * pj[1]) + R.m[3 * c + 2] * pj[2]) + t[c];
    if (!(q[2] > 0)) continue;
    const double ud = rint((A.fx * q[0]) / q[2] + A.cx), vd = rint((A.fy * q[1]) / q[2] + A.cy);
    if (!(ud >= 0 && ud <= (double)(A.W - 1) && vd >= 0 && vd <= (double)(A.H - 1))) continue;      // a NaN fails
    double pi[3], n[3];
    if (!da_target(A, tg, (int)ud, (int)vd, pi, n)) continue;
    const double e[3] = {q[0] - pi[0], q[1] - pi[1], q[2] - pi[2]};
    if (sqrt(da_dot(e, e)) > A.max_dist) continue;
    if (fabs(da_dot(n, q)) < A.min_cos * sqrt(da_dot(q, q))) continue;
    const double r = da_dot(n, e);
    double m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = (R.m[c] * n[0] + R.m[3 + c] * n[1]) + R.m[6 + c] * n[2];
    const double J[6] = {pj[1] * m[2] - pj[2] * m[1], pj[2] * m[0] - pj[0] * m[2], pj[0] * m[1] - pj[1] * m[0], m[0], m[1], m[2]};
    const double w = 1.0 / (da_sigma2(A, n, pi) + da_sigma2(A, m, pj));
    double Jw[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) Jw[a] = w * J[a];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = a; b < 6; ++b) acc[ut6(a, b)] += Jw[a] * J[b];
      acc[DA_G + a] += Jw[a] * r;
    }
    acc[DA_CHI2] += (w * r) * r;
    acc[DA_SS] += r * r;
    acc[DA_CNT] += 1.0;
  }
}

// the normal equations of one evaluation: the status, the smallest pivot, the scales s and M = L^-1 of the scaled matrix
__device__ __forceinline__ int da_factor(const DaArgs &A, const double sum[DA_NS], double &min_pivot, double sc[6], double Mi[21]) {
  min_pivot = 0;
  bool fin = true;
#pragma unroll
  for (int c = 0; c < DA_NS; ++c) fin = fin && fabs(sum[c]) < __builtin_huge_val();
  if (!fin) return FGO_DA_NUM;
  if ((int)sum[DA_CNT] < A.min_pairs) return FGO_DA_TOO_FEW;
  bool pos = true;
#pragma unroll
  for (int r = 0; r < 6; ++r) pos = pos && sum[ut6(r, r)] > 0;
  if (!pos) return FGO_DA_DEGENERATE;
  double Hs[21], L[21];
#pragma unroll
  for (int r = 0; r < 6; ++r) sc[r] = 1.0 / sqrt(sum[ut6(r, r)]);
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) Hs[ut6(r, c)] = (sum[ut6(r, c)] * sc[r]) * sc[c];
  chol6_packed(Hs, L);
  // the pivots as chol6_packed met them: d_j = Hs_jj - sum_k L_jk^2 in its own order
  double mp = __builtin_huge_val();
  bool nan = false;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = Hs[ut6(j, j)];
#pragma unroll
    for (int kk = 0; kk < j; ++kk) d -= L[lt(j, kk)] * L[lt(j, kk)];
    nan = nan || d != d;
    mp = d < mp ? d : mp;
  }
  min_pivot = nan ? 0.0 : mp;
  if (nan || !(mp >= A.min_pivot)) return FGO_DA_DEGENERATE;
  tri6_inverse(L, Mi);
  return FGO_DA_OK;
}

// delta = s * (M^T (M (s * g)))
__device__ __forceinline__ void da_step(const double sum[DA_NS], const double sc[6], const double Mi[21], double delta[6]) {
  double y[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double s = 0;
#pragma unroll
    for (int c = 0; c <= r; ++c) s += Mi[lt(r, c)] * (sc[c] * sum[DA_G + c]);
    y[r] = s;
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double s = 0;
#pragma unroll
    for (int r = c; r < 6; ++r) s += Mi[lt(r, c)] * y[r];
    delta[c] = sc[c] * s;
  }
}

template <bool LDS>
__global__ __launch_bounds__(DA_T) void k_depth_align(DaArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint16_t s_tgt[];
  __shared__ double s_red[DA_W * DA_NS];
  __shared__ double s_pose[8];
  __shared__ int s_ctl[2];                                  // the status and the convergence flag of the last step
  const int64_t pair = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int NP = A.W * A.H;
  const uint16_t *__restrict__ src = A.depth + A.fj[pair] * (int64_t)NP;
  const uint16_t *tg = A.depth + A.fi[pair] * (int64_t)NP;
  if (LDS) {
    if ((NP & 7) == 0) {                                    // frames start at multiples of 16 bytes
      const uint4 *g4 = reinterpret_cast<const uint4 *>(tg);
      uint4 *s4 = reinterpret_cast<uint4 *>(s_tgt);
      for (int e = tid; e < NP / 8; e += DA_T) s4[e] = g4[e];
    } else {
      for (int e = tid; e < NP; e += DA_T) s_tgt[e] = tg[e];
    }
    __syncthreads();
    tg = s_tgt;
  }
  Pose X = {{0, 0, 0}, {0, 0, 0, 1}};
  if (A.init) {
    const double *p = A.init + 7 * pair;
    X = {{p[0], p[1], p[2]}, {p[3], p[4], p[5], p[6]}};
  }
  int status = FGO_DA_OK, steps = 0, conv = 0;
  bool first = true;
  double acc[DA_NS], min_pivot = 0, sc[6], Mi[21];
  for (int l = 0; l < A.n_levels && status == FGO_DA_OK; ++l) {
    conv = 0;
    for (int it = 0; it < A.iters[l]; ++it) {
      da_evaluate(A, src, tg, X, A.skip[l], acc);
      bsum<DA_W>(acc, s_red);
      if (first && A.neq && tid == 0) {
        for (int c = 0; c < 28; ++c) A.neq[28 * pair + c] = acc[c];
      }
      first = false;
      if (wave == 0) {
        int st = da_factor(A, acc, min_pivot, sc, Mi), cv = 0;
        if (st == FGO_DA_OK) {
          double d[6];
          da_step(acc, sc, Mi, d);
          cv = sqrt(da_dot(d, d)) < A.eps_rot && sqrt(da_dot(d + 3, d + 3)) < A.eps_trans;
#pragma unroll
          for (int c = 0; c < 6; ++c) d[c] = -d[c];
          X = retract_pose3(X, d);
          const double chk = ((X.t.x + X.t.y) + X.t.z) + ((X.q.x + X.q.y) + (X.q.z + X.q.w));
          if (!(fabs(chk) < __builtin_huge_val())) st = FGO_DA_NUM;
        }
        if (tid == 0) {
          s_pose[0] = X.t.x; s_pose[1] = X.t.y; s_pose[2] = X.t.z;
          s_pose[3] = X.q.x; s_pose[4] = X.q.y; s_pose[5] = X.q.z; s_pose[6] = X.q.w;
          s_ctl[0] = st; s_ctl[1] = cv;
        }
      }
      __syncthreads();          // the next writer of s_pose / s_ctl is behind the two barriers of the next bsum
      X = {{s_pose[0], s_pose[1], s_pose[2]}, {s_pose[3], s_pose[4], s_pose[5], s_pose[6]}};
      status = s_ctl[0]; conv = s_ctl[1];
      if (status != FGO_DA_OK) break;
      ++steps;
      if (conv) break;
    }
  }
  if (status == FGO_DA_OK) {    // uniform: the status came out of LDS
    da_evaluate(A, src, tg, X, A.skip[A.n_levels - 1], acc);
    bsum<DA_W>(acc, s_red);
    if (first && A.neq && tid == 0) {
      for (int c = 0; c < 28; ++c) A.neq[28 * pair + c] = acc[c];
    }
    if (tid == 0) status = da_factor(A, acc, min_pivot, sc, Mi);
  }
  if (tid != 0) return;         // the last barrier is behind
  fgo_depth_align_result res = {status, acc[DA_CNT] >= 0 && acc[DA_CNT] < 0x1p31 ? (int)acc[DA_CNT] : 0, steps, 0, 0.0, 0.0, min_pivot};
  double *po = A.pose + 7 * pair;
  if (status == FGO_DA_OK) {
    res.converged = conv;
    res.rmse = sqrt(acc[DA_SS] / acc[DA_CNT]);
    res.chi2 = acc[DA_CHI2];
    const double sg = X.q.w < 0 ? -1.0 : 1.0;
    po[0] = X.t.x; po[1] = X.t.y; po[2] = X.t.z; po[3] = sg * X.q.x; po[4] = sg * X.q.y; po[5] = sg * X.q.z; po[6] = sg * X.q.w;
    if (A.info) {
      for (int c = 0; c < 21; ++c) A.info[21 * pair + c] = acc[c];
    }
    if (A.cov) {
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) {
          double s = 0;
#pragma unroll
          for (int kk = c; kk < 6; ++kk) s += Mi[lt(kk, r)] * Mi[lt(kk, c)];
          s = (s * sc[r]) * sc[c];
          A.cov[36 * pair + 6 * r + c] = s;
          A.cov[36 * pair + 6 * c + r] = s;
        }
    }
  } else {                      // the void record of a failed pair
    po[0] = po[1] = po[2] = po[3] = po[4] = po[5] = 0; po[6] = 1;
    if (A.info) {
      for (int c = 0; c < 21; ++c) A.info[21 * pair + c] = 0;
      for (int r = 0; r < 6; ++r) A.info[21 * pair + ut6(r, r)] = 10000.0;
    }
    if (A.cov) {
      for (int c = 0; c < 36; ++c) A.cov[36 * pair + c] = 0;
    }
  }
  A.res[pair] = res;
}

int g_da_form = 0;
double g_da_kernel_ms = 0.0;

bool nonneg_finite(double v) { return v >= 0 && std::isfinite(v); }
bool pos_finite(double v) { return v > 0 && std::isfinite(v); }

}  // namespace
}  // namespace fgo

extern "C" double fgo_debug_depth_align_kernel_ms(void) { return fgo::g_da_kernel_ms; }
extern "C" int fgo_debug_depth_align_form(int form) {
  if (form >= 0 && form <= 2) fgo::g_da_form = form;
  return fgo::g_da_form;
}

extern "C" void fgo_depth_align_params_default(fgo_depth_align_params *p) {
  if (!p) return;
  p->fx = p->fy = 250.5773;
  p->cx = 90.0; p->cy = 70.0;
  p->z_scale = 0.001;
  p->z_min = 0.1; p->z_max = 5.0;
  p->sigma_px = 1.0;
  p->sigma_z[0] = 0.014; p->sigma_z[1] = 0.0; p->sigma_z[2] = 0.0;
  p->n_levels = 3;
  p->skip[0] = 4; p->skip[1] = 2; p->skip[2] = 2;
  p->iters[0] = 10; p->iters[1] = 10; p->iters[2] = 5;
  p->normal_step = 2;
  p->normal_jump = 0.05;
  p->max_dist = 0.10;
  p->min_cos = 0.17364817766693041;     // cos 80 deg
  p->min_pairs = 500;
  p->eps_rot = 1e-6; p->eps_trans = 1e-6;
  p->min_pivot = 1e-6;
}

extern "C" int fgo_depth_align_batch(int device, int64_t n_frames, int width, int height, const uint16_t *depth, int64_t n_pairs,
                                     const int64_t *frame_i, const int64_t *frame_j, const double *pose_ij7_init,
                                     const fgo_depth_align_params *params, double *pose_ij7_out, double *info_ut21_out, double *cov36_out,
                                     double *normal_eq_out, fgo_depth_align_result *result) {
  using namespace fgo;
  fgo_depth_align_params P;
  fgo_depth_align_params_default(&P);
  if (params) P = *params;
  if (n_frames < 0 || n_pairs < 0 || n_pairs > INT_MAX) return FGO_EINVAL;
  if (width < 1 || height < 1 || (int64_t)width * height > FGO_DA_MAX_PIXELS) return FGO_EINVAL;
  const int64_t NP = (int64_t)width * height;
  if (n_frames > INT64_MAX / (NP * 2)) return FGO_EINVAL;
  if (!pinhole_ok(P.fx, P.fy, P.cx, P.cy, P.z_scale) || !(P.z_min >= 0) || !(P.z_min < P.z_max)) return FGO_EINVAL;
  if (!pos_finite(P.sigma_px)) return FGO_EINVAL;
  if (!nonneg_finite(P.sigma_z[0]) || !nonneg_finite(P.sigma_z[1]) || !nonneg_finite(P.sigma_z[2]) ||
      !(P.sigma_z[0] + P.sigma_z[1] + P.sigma_z[2] > 0))
    return FGO_EINVAL;
  if (P.n_levels < 1 || P.n_levels > FGO_DA_MAX_LEVELS) return FGO_EINVAL;
  for (int l = 0; l < P.n_levels; ++l)
    if (P.skip[l] < 1 || P.iters[l] < 0 || P.iters[l] > 100) return FGO_EINVAL;
  if (P.normal_step < 1 || P.normal_step > 64 || !pos_finite(P.normal_jump) || !pos_finite(P.max_dist)) return FGO_EINVAL;
  if (!in_closed(P.min_cos, 0.0, 1.0) || P.min_pairs < 6 || !nonneg_finite(P.eps_rot) || !nonneg_finite(P.eps_trans)) return FGO_EINVAL;
  if (!(P.min_pivot >= 0 && P.min_pivot < 1)) return FGO_EINVAL;
  if (n_pairs == 0) return FGO_OK;
  if (!depth || !frame_i || !frame_j || !pose_ij7_out || !result) return FGO_EINVAL;
  for (int64_t p = 0; p < n_pairs; ++p)
    if (frame_i[p] < 0 || frame_i[p] >= n_frames || frame_j[p] < 0 || frame_j[p] >= n_frames) return FGO_EINVAL;
  std::vector<double> init;
  if (pose_ij7_init) {
    init.assign(pose_ij7_init, pose_ij7_init + 7 * (size_t)n_pairs);
    for (int64_t p = 0; p < n_pairs; ++p) {
      double *x = init.data() + 7 * p;
      if (!quat_ok(x + 3) || !std::isfinite(x[0]) || !std::isfinite(x[1]) || !std::isfinite(x[2])) return FGO_EINVAL;
      const double n = std::sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6]);
      for (int k = 3; k < 7; ++k) x[k] /= n;
    }
  }
  if (int rc = select_device(device)) return rc;

  const size_t n = (size_t)n_pairs, D = sizeof(double);
  Staged S;
  const int h_depth = S.in(depth, (size_t)n_frames * (size_t)NP * sizeof(uint16_t));
  const int h_fi = S.in(frame_i, n * sizeof(int64_t)), h_fj = S.in(frame_j, n * sizeof(int64_t));
  const int h_init = S.in(pose_ij7_init ? init.data() : nullptr, 7 * n * D);
  const int h_pose = S.out(pose_ij7_out, 7 * n * D), h_info = S.out(info_ut21_out, 21 * n * D), h_cov = S.out(cov36_out, 36 * n * D);
  const int h_neq = S.out(normal_eq_out, 28 * n * D), h_res = S.out(result, n * sizeof(fgo_depth_align_result));
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  DaArgs A;
  A.W = width; A.H = height;
  A.depth = S.ptr<uint16_t>(h_depth); A.fi = S.ptr<int64_t>(h_fi); A.fj = S.ptr<int64_t>(h_fj); A.init = S.ptr<double>(h_init);
  A.fx = P.fx; A.fy = P.fy; A.cx = P.cx; A.cy = P.cy; A.z_scale = P.z_scale; A.z_min = P.z_min; A.z_max = P.z_max;
  A.s_px2 = P.sigma_px * P.sigma_px; A.sz0 = P.sigma_z[0]; A.sz1 = P.sigma_z[1]; A.sz2 = P.sigma_z[2];
  A.n_levels = P.n_levels;
  for (int l = 0; l < 3; ++l) { A.skip[l] = l < P.n_levels ? P.skip[l] : 1; A.iters[l] = l < P.n_levels ? P.iters[l] : 0; }
  A.step = P.normal_step; A.min_pairs = P.min_pairs;
  A.jump = P.normal_jump; A.max_dist = P.max_dist; A.min_cos = P.min_cos; A.eps_rot = P.eps_rot; A.eps_trans = P.eps_trans;
  A.min_pivot = P.min_pivot;
  A.pose = S.ptr<double>(h_pose); A.info = S.ptr<double>(h_info); A.cov = S.ptr<double>(h_cov); A.neq = S.ptr<double>(h_neq);
  A.res = S.ptr<fgo_depth_align_result>(h_res);
  const size_t words = ((size_t)NP * sizeof(uint16_t) + 15) & ~(size_t)15;
  const bool lds = g_da_form != 2 && words <= (size_t)DA_LDS_BYTES;
  KernelTimer timer;
  if (!timer.start()) return FGO_ENUM;
  if (lds) hipLaunchKernelGGL(k_depth_align<true>, dim3((unsigned)n_pairs), dim3(DA_T), words, 0, A);
  else hipLaunchKernelGGL(k_depth_align<false>, dim3((unsigned)n_pairs), dim3(DA_T), 0, 0, A);
  timer.stop();
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  g_da_kernel_ms = timer.ms();
  return S.download();
}
