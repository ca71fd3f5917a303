// Plane extraction from depth frames on the MI355X (gfx950, f64, wave64): what the reference obtains frame after frame from
// CPlaneNode::extractPlanes(i_img, d_img, &sr4k) (gtsam/test_plane_check_vo.cpp:181,188,213; gtsam/test_ba_imu_graph.cpp:137,274,297)
// and hands on as CPlane::m_CP -- a sequential RANSAC over the range image, a total-least-squares fit on the inliers and the
// covariance of that fit -- for ONE frame.  The plane package's arithmetic is not in the reference; include/fgo.h states the
// semantics this file implements, and tests/plane_extract_reference.py restates them in numpy.  The frames are independent:
// fgo_plane_extract_batch runs ONE WORKGROUP (PX_WAVES waves) PER FRAME and all frames in one launch.
//
//   points   every pixel is back-projected once into the frame's scratch (3 doubles per pixel); its label starts as -2 (no depth)
//            or -1 (free).
//   compact  the candidates of a round (the free pixels) are written in pixel order by a workgroup prefix scan: a ballot and a
//            population count inside a wave, the wave totals through LDS, PX_T pixels at a time.
//   score    PX_HPL HYPOTHESES PER LANE, PX_PASS = PX_T PX_HPL a pass.  A lane draws its three candidates from the counter-based
//            hash and builds (n, d).  The candidates are staged in LDS PX_CHUNK at a time (x, y as one 16-byte pair, z apart);
//            every lane reads the same point at the same time (a broadcast read) and tests |n.p + d| <= max_dist for each of its
//            hypotheses.  A dead hypothesis carries n = 0, d = huge and counts nothing, so the loop does not diverge; the barriers
//            around the staging are outside every branch that is not uniform over the workgroup.
//   winner   a lane keeps the best (count, h) of its own hypotheses (h rises, a later one has to be strictly better); the lanes are
//            merged by an integer butterfly (larger count, then lower h), the waves through LDS in wave order.
//   fit      the lanes stride the candidates (or the pixels): sums for the centroid, sums for the scatter of the centred points, the
//            3x3 eigenproblem by PX_SWEEPS cyclic Jacobi sweeps (uniform over the workgroup, redundantly in every lane), the new
//            set by the same distance function the scoring uses.
//   final    every pixel with a depth goes to the nearest kept plane, planes left below min_pixels are dropped, every remaining
//            plane is fitted once more; a last pass forms the two 3x3 sums of the sandwich covariance.
// Every sum over pixels is a per-lane sum in pixel order followed by a butterfly whose result is bit-identical in every lane, and
// the waves' sums are added in wave order by every lane: no atomics, no dependence on the rest of the batch, and every decision is
// uniform over the workgroup without a broadcast.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include <cmath>
#include "../../include/fgo.h"
#include "small_dense_device.hpp"
#include "plane_fit_device.hpp"
#include "batch_call.hpp"

namespace fgo {
using namespace dev;

namespace {

// PX_WAVES, PX_T, PX_SWEEPS and PX_NSUM, with the fit itself, are in plane_fit_device.hpp
constexpr int PX_HPL = 2;                        // hypotheses a lane scores at a time: one LDS read serves both
constexpr int PX_PASS = PX_T * PX_HPL;           // hypotheses of one pass over the candidates
constexpr int PX_CHUNK = 2048;                   // candidates staged in LDS at a time (48 KB)
constexpr int PX_MAX_PIXELS = 1 << 24;
constexpr int PX_MAX_HYP = 1 << 16;

struct PxArgs {
  int64_t n;
  int W, NP;
  const uint16_t *depth;
  double fx, fy, cx, cy, z_scale, z_min, z_max, max_dist, min_area, s_px2, sz0, sz1, sz2;
  int K, min_pixels, max_planes, refine_rounds;
  uint64_t seed;
  double *pts;                                  // scratch: n x NP x 3
  int32_t *cand;                                // scratch: n x NP, the candidates of the round in pixel order
  uint8_t *inset;                               // scratch: n x NP, by candidate
  int8_t *label;                                // n x NP: always there, the kernel works in it
  double *abcd, *cov16, *ut6;                   // ut6 may be NULL
  fgo_plane_extract_plane *plane;               // may be NULL
  int32_t *hyp;                                 // may be NULL
  fgo_plane_extract_result *res;
};

// hypothesis hc = r K + h over the M >= 3 candidates; false if it is invalid
__device__ __forceinline__ bool hypothesis(const PxArgs &A, const double *__restrict__ pts, const int32_t *__restrict__ cand, uint64_t hc, int M, Pl &P) {
  int a, b, c;
  sample3(A.seed, hc, M, a, b, c);
  const double *pa = pts + 3 * (int64_t)cand[a], *pb = pts + 3 * (int64_t)cand[b], *pc = pts + 3 * (int64_t)cand[c];
  const double a0 = pa[0], a1 = pa[1], a2 = pa[2];
  const double e0 = pb[0] - a0, e1 = pb[1] - a1, e2 = pb[2] - a2, f0 = pc[0] - a0, f1 = pc[1] - a1, f2 = pc[2] - a2;
  const double m0 = e1 * f2 - e2 * f1, m1 = e2 * f0 - e0 * f2, m2 = e0 * f1 - e1 * f0;
  const double nm = sqrt(m0 * m0 + m1 * m1 + m2 * m2);
  if (!(nm >= A.min_area)) return false;
  P.n[0] = m0 / nm; P.n[1] = m1 / nm; P.n[2] = m2 / nm;
  P.d = -(P.n[0] * a0 + P.n[1] * a1 + P.n[2] * a2);
  orient(P);
  return true;
}

__global__ __launch_bounds__(PX_T) void k_plane_extract(PxArgs A) {
  __shared__ __attribute__((aligned(16))) double2 s_xy[PX_CHUNK];     // a chunk of candidates
  __shared__ double s_z[PX_CHUNK];
  __shared__ double red_d[PX_WAVES * PX_NSUM];
  __shared__ int red_i[PX_WAVES * FGO_PX_MAX_PLANES];
  __shared__ int w_n[PX_WAVES], w_cnt[PX_WAVES], w_h[PX_WAVES], w_valid[PX_WAVES];
  __shared__ Pl pl[FGO_PX_MAX_PLANES];                                // the planes the rounds kept
  __shared__ int pl_meta[FGO_PX_MAX_PLANES][4];                       // best_hypothesis, best_count, n_valid_hyp, fits
  __shared__ int pl_map[FGO_PX_MAX_PLANES];                           // final pass: the new index of a kept plane, or -1
  const int64_t frame = blockIdx.x;
  if (frame >= A.n) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NP = A.NP, K = A.K;
  const uint16_t *__restrict__ dep = A.depth + frame * NP;
  double *__restrict__ pts = A.pts + 3 * frame * NP;
  int32_t *__restrict__ cand = A.cand + frame * NP;
  uint8_t *__restrict__ inset = A.inset + frame * NP;
  int8_t *__restrict__ lab = A.label + frame * NP;
  int32_t *__restrict__ hyp = A.hyp ? A.hyp + frame * (int64_t)A.max_planes * K : nullptr;
  const double md = A.max_dist;

  // ---- points
  int nv[1] = {0};
  for (int pix = tid; pix < NP; pix += PX_T) {
    const int v = pix / A.W, u = pix - v * A.W;
    const double z = (double)dep[pix] * A.z_scale;
    const bool valid = z > A.z_min && z < A.z_max;
    pts[3 * (int64_t)pix] = ((double)u - A.cx) * z / A.fx;
    pts[3 * (int64_t)pix + 1] = ((double)v - A.cy) * z / A.fy;
    pts[3 * (int64_t)pix + 2] = z;
    lab[pix] = valid ? -1 : -2;
    nv[0] += valid;
  }
  bsum<PX_WAVES>(nv, red_i);                                 // its barriers publish pts and lab to the workgroup
  const int n_valid_pixels = nv[0];

  // ---- rounds: everything below that is not indexed by a pixel is uniform over the workgroup
  int kept = 0, rounds_run = 0;
  const int need = max(3, A.min_pixels);
  for (int r = 0; r < A.max_planes; ++r) {
    // compact the free pixels in pixel order
    __syncthreads();                               // the labels and the plane of the round before are visible
    int M = 0;
    for (int base = 0; base < NP; base += PX_T) {
      const int pix = base + tid;
      const bool f = pix < NP && lab[pix] == -1;
      const unsigned long long bal = __ballot(f);
      __syncthreads();                             // the readers of w_n of the tile before are done
      if (lane == 0) w_n[wave] = __popcll(bal);
      __syncthreads();
      int off = M;
#pragma unroll
      for (int w = 0; w < PX_WAVES; ++w) {
        const int c = w_n[w];
        off += w < wave ? c : 0;
        M += c;
      }
      if (f) cand[off + __popcll(bal & ((1ull << lane) - 1ull))] = pix;
    }
    __syncthreads();                               // cand is complete
    if (M < need) break;
    ++rounds_run;

    // score
    int my_cnt = -1, my_h = INT_MAX, my_valid = 0;
    const int passes = (K + PX_PASS - 1) / PX_PASS, chunks = (M + PX_CHUNK - 1) / PX_CHUNK;
    for (int pass = 0; pass < passes; ++pass) {
      Pl H[PX_HPL];
      bool live[PX_HPL];
      int cnt[PX_HPL];
#pragma unroll
      for (int j = 0; j < PX_HPL; ++j) {
        const int h = pass * PX_PASS + j * PX_T + tid;
        live[j] = h < K && hypothesis(A, pts, cand, (uint64_t)r * (uint64_t)K + (uint64_t)h, M, H[j]);
        if (!live[j]) { H[j].n[0] = H[j].n[1] = H[j].n[2] = 0; H[j].d = 1e300; }
        cnt[j] = 0;
      }
      bool any = false;
#pragma unroll
      for (int j = 0; j < PX_HPL; ++j) any = any || live[j];
      for (int ch = 0; ch < chunks; ++ch) {
        const int m0 = ch * PX_CHUNK, mc = min(PX_CHUNK, M - m0);
        if (chunks > 1 || pass == 0) {             // uniform: a round of one chunk is staged once
          __syncthreads();
          for (int e = tid; e < mc; e += PX_T) {
            const double *p = pts + 3 * (int64_t)cand[m0 + e];
            s_xy[e] = make_double2(p[0], p[1]);
            s_z[e] = p[2];
          }
          __syncthreads();
        }
        if (any) {
#pragma unroll 8
          for (int m = 0; m < mc; ++m) {            // unrolled: the LDS reads of eight points are in flight at once
            const double2 xy = s_xy[m];
            const double z = s_z[m];
#pragma unroll
            for (int j = 0; j < PX_HPL; ++j) cnt[j] += pdist(H[j], xy.x, xy.y, z) <= md;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < PX_HPL; ++j) {
        const int h = pass * PX_PASS + j * PX_T + tid;
        if (h < K) {
          const int c = live[j] ? cnt[j] : -1;
          if (hyp) hyp[(int64_t)r * K + h] = c;
          my_valid += live[j];
          if (c > my_cnt) { my_cnt = c; my_h = h; }
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) better(my_cnt, my_h, __shfl_xor(my_cnt, o, 64), __shfl_xor(my_h, o, 64));
    my_valid = wave_sum(my_valid);
    __syncthreads();                               // the readers of the round before are done
    if (lane == 0) { w_cnt[wave] = my_cnt; w_h[wave] = my_h; w_valid[wave] = my_valid; }
    __syncthreads();
    int best_cnt = w_cnt[0], best_h = w_h[0], n_valid = w_valid[0];
#pragma unroll
    for (int w = 1; w < PX_WAVES; ++w) { better(best_cnt, best_h, w_cnt[w], w_h[w]); n_valid += w_valid[w]; }
    if (best_cnt < 0 || best_cnt < A.min_pixels) break;

    // refine: the set starts as the winner's inliers; a thread owns the candidates tid, tid + PX_T, ...
    Pl P;
    hypothesis(A, pts, cand, (uint64_t)r * (uint64_t)K + (uint64_t)best_h, M, P);
    for (int i = tid; i < M; i += PX_T) {
      const double *p = pts + 3 * (int64_t)cand[i];
      inset[i] = pdist(P, p[0], p[1], p[2]) <= md;
    }
    int fits = 0;
    bool keep = true;
    for (int round = 0; round < A.refine_rounds; ++round) {
      double cen[3];
      int N;
      fit_plane(pts, M, [&](int i) { return inset[i] ? cand[i] : -1; }, red_d, P, cen, N);
      ++fits;
      int chg[2] = {0, 0};                         // changed, members
      for (int i = tid; i < M; i += PX_T) {
        const double *p = pts + 3 * (int64_t)cand[i];
        const bool in = pdist(P, p[0], p[1], p[2]) <= md;
        chg[0] += in != (inset[i] != 0);
        chg[1] += in;
        inset[i] = in;
      }
      bsum<PX_WAVES>(chg, red_i);
      if (chg[1] < A.min_pixels) { keep = false; break; }
      if (chg[0] == 0) break;
    }
    if (!keep) break;
    for (int i = tid; i < M; i += PX_T)
      if (inset[i]) lab[cand[i]] = (int8_t)r;
    if (tid == 0) {
      pl[kept] = P;
      pl_meta[kept][0] = best_h; pl_meta[kept][1] = best_cnt; pl_meta[kept][2] = n_valid; pl_meta[kept][3] = fits;
    }
    ++kept;
  }
  __syncthreads();

  // ---- final pass: every pixel with a depth goes to the nearest kept plane (ties to the lower index)
  int cntk[FGO_PX_MAX_PLANES];
#pragma unroll
  for (int k = 0; k < FGO_PX_MAX_PLANES; ++k) cntk[k] = 0;
  for (int pix = tid; pix < NP; pix += PX_T) {
    if (lab[pix] == -2) continue;
    const double *p = pts + 3 * (int64_t)pix;
    const double x = p[0], y = p[1], z = p[2];
    int best = -1;
    double bd = __builtin_huge_val();
    for (int k = 0; k < kept; ++k) {
      const double d = pdist(pl[k], x, y, z);
      if (d < bd) { bd = d; best = k; }
    }
    if (!(bd <= md)) best = -1;
    lab[pix] = (int8_t)best;
#pragma unroll
    for (int k = 0; k < FGO_PX_MAX_PLANES; ++k) cntk[k] += best == k;
  }
  bsum<PX_WAVES>(cntk, red_i);
  int n_planes = 0;
#pragma unroll
  for (int k = 0; k < FGO_PX_MAX_PLANES; ++k) {
    const bool stays = k < kept && cntk[k] >= A.min_pixels;
    if (tid == 0) pl_map[k] = stays ? n_planes : -1;
    n_planes += stays;
  }
  __syncthreads();
  if (n_planes != kept) {
    for (int pix = tid; pix < NP; pix += PX_T) {
      const int l = lab[pix];
      if (l >= 0) lab[pix] = (int8_t)pl_map[l];
    }
  }
  __syncthreads();

  // ---- the final fit of every remaining plane, and the covariance of that fit
  int status = FGO_PX_OK;
  double *abcd = A.abcd + frame * A.max_planes * 4, *cov16 = A.cov16 + frame * A.max_planes * 16;
  double *ut6 = A.ut6 ? A.ut6 + frame * A.max_planes * 6 : nullptr;
  fgo_plane_extract_plane *po = A.plane ? A.plane + frame * A.max_planes : nullptr;
  const PxNoise noise = {A.fx, A.fy, A.s_px2, A.sz0, A.sz1, A.sz2};
  int old = 0;
  for (int k = 0; k < n_planes; ++k, ++old) {
    while (pl_map[old] < 0) ++old;                 // the round's slot this plane came from
    Pl P;
    double cen[3];
    int N;
    fit_plane(pts, NP, [&](int pix) { return lab[pix] == k ? pix : -1; }, red_d, P, cen, N);
    double b1[3], b2[3], C[9], rmse;
    if (!fit_covariance(pts, NP, [&](int pix) { return lab[pix] == k; }, P, cen, N, noise, red_d, b1, b2, C, rmse)) { status = FGO_PX_NUM; break; }
    if (tid == 0) {
      store_plane(P, b1, b2, C, abcd + 4 * k, cov16 + 16 * k, ut6 ? ut6 + 6 * k : nullptr);
      if (po) po[k] = {N, pl_meta[old][0], pl_meta[old][1], pl_meta[old][2], pl_meta[old][3], 0, rmse, {cen[0], cen[1], cen[2]}};
    }
  }

  // ---- a frame that failed numerically has no planes: zero outputs, labels of -2 / -1 only
  if (status != FGO_PX_OK) {
    __syncthreads();                               // thread 0's writes of the planes before the failing one
    for (int pix = tid; pix < NP; pix += PX_T)
      if (lab[pix] >= 0) lab[pix] = -1;
    for (int e = tid; e < 4 * A.max_planes; e += PX_T) abcd[e] = 0;
    for (int e = tid; e < 16 * A.max_planes; e += PX_T) cov16[e] = 0;
    if (ut6)
      for (int e = tid; e < 6 * A.max_planes; e += PX_T) ut6[e] = 0;
    if (po)
      for (int e = tid; e < A.max_planes; e += PX_T) po[e] = {0, 0, 0, 0, 0, 0, 0.0, {0.0, 0.0, 0.0}};
    n_planes = 0;
  }
  if (hyp)
    for (int e = rounds_run * K + tid; e < A.max_planes * K; e += PX_T) hyp[e] = -2;
  if (tid == 0) A.res[frame] = {status, n_planes, n_valid_pixels, rounds_run};
}

double g_kernel_ms = 0.0;

}  // namespace
}  // namespace fgo

extern "C" double fgo_debug_plane_extract_kernel_ms(void) { return fgo::g_kernel_ms; }

extern "C" void fgo_plane_extract_params_default(fgo_plane_extract_params *p) {
  if (!p) return;
  p->fx = p->fy = 250.5773;
  p->cx = 90.0; p->cy = 70.0;
  p->z_scale = 0.001;
  p->z_min = 0.1; p->z_max = 5.0;
  p->hypotheses = 512;
  p->seed = 0;
  p->max_dist = 0.05;
  p->min_area = 1e-3;
  p->min_pixels = 1500;
  p->max_planes = 4;
  p->refine_rounds = 3;
  p->sigma_px = 1.0;
  p->sigma_z[0] = 0.014; p->sigma_z[1] = 0.0; p->sigma_z[2] = 0.0;
}

extern "C" int fgo_plane_extract_batch(int device, int64_t n_frames, int width, int height, const uint16_t *depth,
                                       const fgo_plane_extract_params *params, fgo_plane_extract_result *result, double *abcd_out,
                                       double *cov16_out, double *cov_ut6_out, fgo_plane_extract_plane *plane_out, int8_t *label_out,
                                       int32_t *hyp_count_out) {
  using namespace fgo;
  fgo_plane_extract_params P;
  fgo_plane_extract_params_default(&P);
  if (params) P = *params;
  if (n_frames < 0 || n_frames > INT_MAX) return FGO_EINVAL;
  if (width < 1 || height < 1 || (int64_t)width * height > PX_MAX_PIXELS) return FGO_EINVAL;
  if (!(P.fx > 0) || !(P.fy > 0) || !(P.z_scale > 0) || !(P.max_dist > 0) || !(P.min_area > 0) || !(P.sigma_px > 0)) return FGO_EINVAL;
  if (!(P.z_min < P.z_max) || !(fabs(P.cx) < HUGE_VAL) || !(fabs(P.cy) < HUGE_VAL)) return FGO_EINVAL;
  if (P.hypotheses < 1 || P.hypotheses > PX_MAX_HYP || P.max_planes < 1 || P.max_planes > FGO_PX_MAX_PLANES || P.refine_rounds < 0 ||
      P.refine_rounds > 10 || P.min_pixels < 3)
    return FGO_EINVAL;
  if (!(P.sigma_z[0] >= 0) || !(P.sigma_z[1] >= 0) || !(P.sigma_z[2] >= 0) || !(P.sigma_z[0] + P.sigma_z[1] + P.sigma_z[2] > 0)) return FGO_EINVAL;
  if (n_frames == 0) return FGO_OK;
  if (!depth || !result || !abcd_out || !cov16_out) return FGO_EINVAL;
  if (int rc = select_device(device)) return rc;
  const size_t n = (size_t)n_frames, np = (size_t)width * (size_t)height, D = sizeof(double), K = (size_t)P.hypotheses, mp = (size_t)P.max_planes;
  // the input; scratch: the points, the candidates and the set; then the outputs (the labels are always there: the kernel works in them)
  Staged S;
  const int h_depth = S.in(depth, n * np * sizeof(uint16_t));
  const int h_pts = S.out(nullptr, 3 * n * np * D, true), h_cand = S.out(nullptr, n * np * sizeof(int32_t), true), h_set = S.out(nullptr, n * np, true);
  const int h_res = S.out(result, n * sizeof(fgo_plane_extract_result));
  void *const slot_host[4] = {abcd_out, cov16_out, cov_ut6_out, plane_out};
  const size_t slot_bytes[4] = {4 * n * mp * D, 16 * n * mp * D, 6 * n * mp * D, n * mp * sizeof(fgo_plane_extract_plane)};
  int h_slot[4];
  for (int k = 0; k < 4; ++k) h_slot[k] = S.out(slot_host[k], slot_bytes[k]);
  const int h_label = S.out(label_out, n * np, true), h_hyp = S.out(hyp_count_out, n * mp * K * sizeof(int32_t));
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  for (int k = 0; k < 4; ++k)                                   // the slots past a frame's last plane stay zero
    if (slot_host[k] && hipMemset(S.ptr<char>(h_slot[k]), 0, slot_bytes[k]) != hipSuccess) return FGO_ENUM;
  PxArgs A;
  A.n = n_frames; A.W = width; A.NP = (int)np;
  A.depth = S.ptr<uint16_t>(h_depth);
  A.fx = P.fx; A.fy = P.fy; A.cx = P.cx; A.cy = P.cy; A.z_scale = P.z_scale; A.z_min = P.z_min; A.z_max = P.z_max;
  A.max_dist = P.max_dist; A.min_area = P.min_area; A.s_px2 = P.sigma_px * P.sigma_px;
  A.sz0 = P.sigma_z[0]; A.sz1 = P.sigma_z[1]; A.sz2 = P.sigma_z[2];
  A.K = P.hypotheses; A.min_pixels = P.min_pixels; A.max_planes = P.max_planes; A.refine_rounds = P.refine_rounds;
  A.seed = P.seed;
  A.pts = S.ptr<double>(h_pts); A.cand = S.ptr<int32_t>(h_cand); A.inset = S.ptr<uint8_t>(h_set);
  A.res = S.ptr<fgo_plane_extract_result>(h_res);
  A.abcd = S.ptr<double>(h_slot[0]); A.cov16 = S.ptr<double>(h_slot[1]); A.ut6 = S.ptr<double>(h_slot[2]);
  A.plane = S.ptr<fgo_plane_extract_plane>(h_slot[3]);
  A.label = S.ptr<int8_t>(h_label);
  A.hyp = S.ptr<int32_t>(h_hyp);
  KernelTimer timer;
  if (!timer.start()) return FGO_ENUM;
  hipLaunchKernelGGL(k_plane_extract, dim3((unsigned)n_frames), dim3(PX_T), 0, 0, A);
  timer.stop();
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  g_kernel_ms = timer.ms();
  return S.download();
}
