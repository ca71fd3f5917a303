// Plane propagation between depth frames on the MI355X (gfx950, f64, wave64): part 1 of CGraphGT::predictPlaneNode with computeSdj,
// inThisPlane, intensityTol and regionGrow (gtsam/gtsam_graph.cpp:725-1041) -- the planes of frame i are carried through the
// relative pose into frame j, their pixels are re-projected as seeds and tested against the predicted plane under the propagated
// variance of its distance, a plane that keeps enough of its support is grown over the intensity image and fitted again -- for ONE
// pair of frames.  include/fgo.h states the semantics, tests/plane_propagate_reference.py restates them in numpy.  The pairs are
// independent: fgo_plane_propagate_batch runs ONE WORKGROUP (PX_T threads) PER PAIR and all pairs in one launch.
//
//   flags    one byte per pixel of frame j, shared by the planes of the pair: free, claimed by plane l (1 + l), REJECTED; while a
//            plane grows also ELIGIBLE (free and in the plane) and the bit IN_E (reached).  The flag byte and the intensity byte
//            live in LDS when the frame has at most 65536 pixels and in the pair's device scratch (the flags) and the input (the
//            intensities) above that: the template parameter selects.
//   points   every pixel of frame j is back-projected once into the pair's scratch (3 doubles per pixel), as the extraction does.
//   seeds    the lanes stride the pixels of frame i; a pixel of plane l projects to nine candidates; the outcome of a candidate
//            depends on the candidate and the plane alone, so lanes that meet on one byte store the same value.
//   growth   a monotone fixed point.  The in-plane test of every free pixel is made once, in parallel (ELIGIBLE); a sweep is then
//            four directional scans over bytes -- a thread per row left to right and right to left, a barrier, a thread per column
//            down and up -- and the sweeps repeat until a workgroup-wide OR of "changed" is zero.  Every productive sweep adds a
//            pixel to E, so the loop ends within W H + 1 sweeps; there is no other cap.  A thread owns its row (its column), and
//            the fixed point does not depend on the order of the scans.
//   refit    plane_fit_device.hpp: the fit and the covariance of the extraction, on the plane's final pixels.
// Every barrier is outside every branch that is not uniform over the workgroup: the plane loop, the kept / dropped decision and
// the status are uniform.  Sums: per lane in pixel order, a butterfly, the waves in wave order; no atomics.
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

constexpr int PP_MAX_PIXELS = 1 << 24;
constexpr int PP_LDS_PIXELS = 65536;             // the largest frame whose flag and intensity bytes are kept in LDS (128 KB of 160)
constexpr uint8_t PP_FREE = 0, PP_REJECTED = 9, PP_ELIGIBLE = 10, PP_IN_E = 0x80;      // 1 + l: claimed by plane l
constexpr double PP_HUGE_PX = 1073741824.0;      // 2^30

struct PpArgs {
  int64_t n;
  int W, H, NP;
  const uint16_t *depth;
  const uint8_t *inten;
  const int8_t *label;
  const int32_t *n_planes;
  const double *abcd, *cov16;
  const int64_t *fi, *fj;
  const double *pose, *info, *cov;
  double fx, fy, cx, cy, z_scale, z_min, z_max, s_px2, sz0, sz1, sz2, dfl2, keep_ratio;
  int tol, rest_thresh;
  double *pts;                                  // scratch: n x NP x 3
  uint8_t *flag;                                // scratch: n x NP, only when the frame does not fit in LDS
  fgo_plane_propagate_result *res;
  double *abcd_out, *cov16_out, *ut6;           // ut6, plane, pred and label_out may be NULL
  fgo_plane_propagate_plane *plane;
  fgo_plane_propagate_pred *pred;
  int8_t *label_out;
};

template <bool LDS>
__global__ __launch_bounds__(PX_T) void k_plane_propagate(PpArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_bytes[];   // LDS: the flags, then the intensities
  __shared__ double red_d[PX_WAVES * PX_NSUM];
  __shared__ int red_i[PX_WAVES * 2];
  __shared__ Pl s_pred[FGO_PX_MAX_PLANES];                            // the predicted planes
  __shared__ double s_sdj[FGO_PX_MAX_PLANES];
  __shared__ int s_slot[FGO_PX_MAX_PLANES];                           // the output slot of a kept plane, -4 for a dropped one
  const int64_t pair = blockIdx.x;
  if (pair >= A.n) return;
  const int tid = threadIdx.x, W = A.W, H = A.H, NP = A.NP;
  const int64_t fi = A.fi[pair], fj = A.fj[pair];
  const uint16_t *__restrict__ dep_i = A.depth + fi * NP, *__restrict__ dep_j = A.depth + fj * NP;
  const int8_t *__restrict__ lab_i = A.label + fi * NP;
  const uint8_t *__restrict__ int_j = A.inten + fj * NP;
  double *__restrict__ pts = A.pts + 3 * pair * NP;
  uint8_t *flag = LDS ? s_bytes : A.flag + pair * NP;
  const uint8_t *inten = LDS ? s_bytes + ((NP + 15) & ~15) : int_j;
  const int npl = A.n_planes[fi];
  constexpr int MP = FGO_PX_MAX_PLANES;
  double *abcd = A.abcd_out + pair * MP * 4, *cov16 = A.cov16_out + pair * MP * 16;
  double *u6 = A.ut6 ? A.ut6 + pair * MP * 6 : nullptr;
  fgo_plane_propagate_plane *po = A.plane ? A.plane + pair * MP : nullptr;
  fgo_plane_propagate_pred *pr = A.pred ? A.pred + pair * MP : nullptr;

  // ---- S_t, in every thread: the status is uniform without a broadcast
  double S[21];
  int status = FGO_PP_OK;
  if (A.cov) {
    const double *__restrict__ c = A.cov + 36 * pair;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int k = r; k < 6; ++k) S[ut6(r, k)] = c[r * 6 + k];
  } else if (!inv6(A.info + 21 * pair, S)) status = FGO_PP_NUM;
  const M3 Svv = block3(S, 3, 3);
  const double *__restrict__ ps = A.pose + 7 * pair;
  const V3 t = {ps[0], ps[1], ps[2]};
  const double qn = sqrt(ps[3] * ps[3] + ps[4] * ps[4] + ps[5] * ps[5] + ps[6] * ps[6]);
  const M3 R = qmat(Q4{ps[3] / qn, ps[4] / qn, ps[5] / qn, ps[6] / qn});

  // ---- prediction: thread l carries plane l over (the arithmetic of k_plane_check)
  int bad = 0;
  if (status == FGO_PP_OK && tid < npl) {
    const double *__restrict__ a = A.abcd + (fi * MP + tid) * 4, *__restrict__ c = A.cov16 + (fi * MP + tid) * 16;
    const PlaneIn P = load_plane(a, c);
    const V3 np = mtv(R, P.n);
    const double dp = dot3(P.n, t) + P.d, sdj = predicted_sdj(P, t, Svv);
    s_pred[tid] = {{np.x, np.y, np.z}, dp};
    s_sdj[tid] = sdj;
    bad = !(sdj >= 0 && finite(sdj));
  }
  if (__syncthreads_or(bad)) status = FGO_PP_NUM;

  int kept = 0, num_added = 0;
  if (status == FGO_PP_OK) {
    // ---- points, flags, intensities
    for (int pix = tid; pix < NP; pix += PX_T) {
      const int v = pix / W, u = pix - v * W;
      const double z = (double)dep_j[pix] * A.z_scale;
      pts[3 * (int64_t)pix] = ((double)u - A.cx) * z / A.fx;
      pts[3 * (int64_t)pix + 1] = ((double)v - A.cy) * z / A.fy;
      pts[3 * (int64_t)pix + 2] = z;
      flag[pix] = PP_FREE;
      if (LDS) s_bytes[((NP + 15) & ~15) + pix] = int_j[pix];
    }
    __syncthreads();
    const PxNoise noise = {A.fx, A.fy, A.s_px2, A.sz0, A.sz1, A.sz2};

    for (int l = 0; l < npl; ++l) {
      const Pl Pj = s_pred[l];
      const double sdj = s_sdj[l];
      const uint8_t mine = (uint8_t)(1 + l);
      // ---- seeds
      int cnt[2] = {0, 0};                         // n_prev, n_seed
      for (int pix = tid; pix < NP; pix += PX_T) {
        if (lab_i[pix] != l) continue;
        ++cnt[0];
        const int v = pix / W, u = pix - v * W;
        const double z = (double)dep_i[pix] * A.z_scale;
        const double x = ((double)u - A.cx) * z / A.fx, y = ((double)v - A.cy) * z / A.fy;
        const V3 q = mtv(R, V3{x - t.x, y - t.y, z - t.z});
        if (!(q.z > 0)) continue;
        const double uf = A.fx * q.x / q.z + A.cx, vf = A.fy * q.y / q.z + A.cy;
        if (!(fabs(uf) < PP_HUGE_PX) || !(fabs(vf) < PP_HUGE_PX)) continue;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          const int uj = (int)(uf + 0.5 * (m - 1));
          if (uj < 0 || uj >= W) continue;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const int vj = (int)(vf + 0.5 * (k - 1));
            if (vj < 0 || vj >= H) continue;
            const int c = vj * W + uj;
            if (flag[c] != PP_FREE) continue;
            const double *p = pts + 3 * (int64_t)c;
            const double zz = p[2];
            uint8_t f = PP_REJECTED;
            if (zz > A.z_min && zz < A.z_max) {
              const double e = pdist(Pj, p[0], p[1], zz), e2 = e * e;
              if (e2 <= sdj || e2 <= A.dfl2) f = mine;
            }
            flag[c] = f;
          }
        }
      }
      __syncthreads();
      for (int pix = tid; pix < NP; pix += PX_T) cnt[1] += flag[pix] == mine;
      bsum<PX_WAVES>(cnt, red_i);
      const int n_prev = cnt[0], n_seed = cnt[1];
      const bool keep = n_seed > (int)(A.keep_ratio * (double)n_prev);
      if (tid == 0 && pr) pr[l] = {{Pj.n[0], Pj.n[1], Pj.n[2], Pj.d}, sdj, n_prev, n_seed, keep ? 1 : 0, 0};
      if (!keep) {
        if (tid == 0) s_slot[l] = -4;
        num_added += n_seed;
        continue;
      }

      // ---- growth: the seeds are in E, every free pixel in the plane is eligible
      for (int pix = tid; pix < NP; pix += PX_T) {
        const uint8_t f = flag[pix];
        if (f == mine) flag[pix] = mine | PP_IN_E;
        else if (f == PP_FREE) {
          const double *p = pts + 3 * (int64_t)pix;
          const double e = pdist(Pj, p[0], p[1], p[2]), e2 = e * e;
          if (e2 <= sdj || e2 <= A.dfl2) flag[pix] = PP_ELIGIBLE;
        }
      }
      __syncthreads();
      int changed;
      auto scan = [&](int idx, int step, int count) {
        bool carry = false;
        int prev = 0;
        for (int k = 0; k < count; ++k, idx += step) {
          const uint8_t f = flag[idx];
          const int I = inten[idx];
          bool in_e = (f & PP_IN_E) != 0;
          if (!in_e && carry && abs(I - prev) <= A.tol && ((f >= 1 && f <= MP) || f == PP_ELIGIBLE)) {
            flag[idx] = f | PP_IN_E;
            in_e = true;
            changed = 1;
          }
          carry = in_e;
          prev = I;
        }
      };
      do {
        changed = 0;
        for (int r = tid; r < H; r += PX_T) { scan(r * W, 1, W); scan(r * W + W - 1, -1, W); }
        __syncthreads();
        for (int c = tid; c < W; c += PX_T) { scan(c, W, H); scan((H - 1) * W + c, -W, H); }
      } while (__syncthreads_or(changed));
      int joined[1] = {0};
      for (int pix = tid; pix < NP; pix += PX_T) {
        const uint8_t f = flag[pix];
        if (f == (PP_ELIGIBLE | PP_IN_E)) { flag[pix] = mine; ++joined[0]; }
        else if (f == PP_ELIGIBLE) flag[pix] = PP_FREE;
        else if (f & PP_IN_E) flag[pix] = f & (uint8_t)~PP_IN_E;
      }
      bsum<PX_WAVES>(joined, red_i);               // its barriers publish the flags
      const int n_pixels = n_seed + joined[0];
      num_added += n_pixels;

      // ---- refit
      Pl P;
      double cen[3], b1[3], b2[3], C[9], rmse;
      int N;
      fit_plane(pts, NP, [&](int pix) { return flag[pix] == mine ? pix : -1; }, red_d, P, cen, N);
      if (!fit_covariance(pts, NP, [&](int pix) { return flag[pix] == mine; }, P, cen, N, noise, red_d, b1, b2, C, rmse)) {
        status = FGO_PP_NUM;
        break;
      }
      if (tid == 0) {
        store_plane(P, b1, b2, C, abcd + 4 * kept, cov16 + 16 * kept, u6 ? u6 + 6 * kept : nullptr);
        if (po) po[kept] = {n_pixels, n_seed, l, 0, rmse, {cen[0], cen[1], cen[2]}};
        s_slot[l] = kept;
      }
      ++kept;
    }
  }
  __syncthreads();                                 // s_slot, the flags, and thread 0's writes of the planes

  if (status == FGO_PP_OK) {
    if (A.label_out) {
      int8_t *__restrict__ lo = A.label_out + pair * NP;
      for (int pix = tid; pix < NP; pix += PX_T) {
        const uint8_t f = flag[pix];
        const double z = pts[3 * (int64_t)pix + 2];
        lo[pix] = (int8_t)(f == PP_FREE ? (z > A.z_min && z < A.z_max ? -1 : -2) : f == PP_REJECTED ? -3 : s_slot[f - 1]);
      }
    }
    if (tid == 0) A.res[pair] = {FGO_PP_OK, kept, num_added, num_added > A.rest_thresh ? 0 : num_added == 0 ? 2 : 1};
  } else {
    // ---- a pair that failed numerically: zero outputs, labels of -2 / -1 only
    if (A.label_out) {
      int8_t *__restrict__ lo = A.label_out + pair * NP;
      for (int pix = tid; pix < NP; pix += PX_T) {
        const double z = (double)dep_j[pix] * A.z_scale;
        lo[pix] = z > A.z_min && z < A.z_max ? -1 : -2;
      }
    }
    for (int e = tid; e < 4 * MP; e += PX_T) abcd[e] = 0;
    for (int e = tid; e < 16 * MP; e += PX_T) cov16[e] = 0;
    if (u6)
      for (int e = tid; e < 6 * MP; e += PX_T) u6[e] = 0;
    if (po)
      for (int e = tid; e < MP; e += PX_T) po[e] = {0, 0, 0, 0, 0.0, {0.0, 0.0, 0.0}};
    if (pr)
      for (int e = tid; e < MP; e += PX_T) pr[e] = {{0.0, 0.0, 0.0, 0.0}, 0.0, 0, 0, 0, 0};
    if (tid == 0) A.res[pair] = {FGO_PP_NUM, 0, 0, 2};
  }
}

double g_pp_kernel_ms = 0.0;

}  // namespace
}  // namespace fgo

extern "C" double fgo_debug_plane_propagate_kernel_ms(void) { return fgo::g_pp_kernel_ms; }

extern "C" void fgo_plane_propagate_params_default(fgo_plane_propagate_params *p) {
  if (!p) return;
  p->fx = p->fy = 250.5773;
  p->cx = 90.0; p->cy = 70.0;
  p->z_scale = 0.001;
  p->z_min = 0.1; p->z_max = 5.0;
  p->sigma_px = 1.0;
  p->sigma_z[0] = 0.014; p->sigma_z[1] = 0.0; p->sigma_z[2] = 0.0;
  p->d_floor = 0.014;
  p->intensity_tol = 5;
  p->keep_ratio = 0.7;
  p->rest_ratio = 0.5;
}

extern "C" int fgo_plane_propagate_batch(int device, int64_t n_frames, int width, int height, const uint16_t *depth, const uint8_t *intensity,
                                         const int8_t *label, const int32_t *n_planes, const double *abcd, const double *cov16,
                                         int64_t n_pairs, const int64_t *frame_i, const int64_t *frame_j, const double *pose_ij7,
                                         const double *info_ut21, const double *cov36, const fgo_plane_propagate_params *params,
                                         fgo_plane_propagate_result *result, double *abcd_out, double *cov16_out, double *cov_ut6_out,
                                         fgo_plane_propagate_plane *plane_out, fgo_plane_propagate_pred *pred_out, int8_t *label_out) {
  using namespace fgo;
  fgo_plane_propagate_params P;
  fgo_plane_propagate_params_default(&P);
  if (params) P = *params;
  if (n_frames < 0 || n_frames > INT_MAX || n_pairs < 0 || n_pairs > INT_MAX) return FGO_EINVAL;
  if (width < 1 || height < 1 || (int64_t)width * height > PP_MAX_PIXELS) return FGO_EINVAL;
  if (!(P.fx > 0) || !(P.fy > 0) || !(P.z_scale > 0) || !(P.sigma_px > 0)) return FGO_EINVAL;
  if (!(P.z_min < P.z_max) || !(fabs(P.cx) < HUGE_VAL) || !(fabs(P.cy) < HUGE_VAL)) return FGO_EINVAL;
  if (!(P.sigma_z[0] >= 0) || !(P.sigma_z[1] >= 0) || !(P.sigma_z[2] >= 0) || !(P.sigma_z[0] + P.sigma_z[1] + P.sigma_z[2] > 0)) return FGO_EINVAL;
  if (!(P.d_floor >= 0) || !(P.d_floor < HUGE_VAL) || P.intensity_tol < 0) return FGO_EINVAL;
  if (!(P.keep_ratio >= 0 && P.keep_ratio <= 1) || !(P.rest_ratio >= 0 && P.rest_ratio <= 1)) return FGO_EINVAL;
  if (n_pairs == 0) return FGO_OK;
  if (!depth || !intensity || !label || !n_planes || !abcd || !cov16 || !frame_i || !frame_j || !pose_ij7 || !result || !abcd_out || !cov16_out)
    return FGO_EINVAL;
  if ((info_ut21 != nullptr) == (cov36 != nullptr)) return FGO_EINVAL;
  constexpr int MP = FGO_PX_MAX_PLANES;
  for (int64_t f = 0; f < n_frames; ++f) {
    if (n_planes[f] < 0 || n_planes[f] > MP) return FGO_EINVAL;
    for (int k = 0; k < n_planes[f]; ++k) {
      const double *a = abcd + (f * MP + k) * 4, nn = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
      if (!(nn > 0) || !std::isfinite(nn)) return FGO_EINVAL;
    }
  }
  for (int64_t p = 0; p < n_pairs; ++p) {
    if (frame_i[p] < 0 || frame_i[p] >= n_frames || frame_j[p] < 0 || frame_j[p] >= n_frames) return FGO_EINVAL;
    if (!quat_ok(pose_ij7 + 7 * p + 3)) return FGO_EINVAL;
  }
  if (int rc = select_device(device)) return rc;
  const size_t nf = (size_t)n_frames, n = (size_t)n_pairs, np = (size_t)width * (size_t)height, D = sizeof(double);
  const bool lds = np <= (size_t)PP_LDS_PIXELS;
  // the frames and the pairs; scratch: the points, and the flags of a frame too large for LDS; then the outputs
  Staged S;
  const int h_depth = S.in(depth, nf * np * sizeof(uint16_t)), h_int = S.in(intensity, nf * np), h_lab = S.in(label, nf * np);
  const int h_npl = S.in(n_planes, nf * sizeof(int32_t)), h_abcd = S.in(abcd, 4 * nf * MP * D), h_c16 = S.in(cov16, 16 * nf * MP * D);
  const int h_fi = S.in(frame_i, n * sizeof(int64_t)), h_fj = S.in(frame_j, n * sizeof(int64_t));
  const int h_pose = S.in(pose_ij7, 7 * n * D), h_info = S.in(info_ut21, 21 * n * D), h_cov = S.in(cov36, 36 * n * D);
  const int h_pts = S.out(nullptr, 3 * n * np * D, true), h_flag = lds ? -1 : S.out(nullptr, n * np, true);
  const int h_res = S.out(result, n * sizeof(fgo_plane_propagate_result));
  void *const slot_host[5] = {abcd_out, cov16_out, cov_ut6_out, plane_out, pred_out};
  const size_t slot_bytes[5] = {4 * n * MP * D, 16 * n * MP * D, 6 * n * MP * D, n * MP * sizeof(fgo_plane_propagate_plane),
                                n * MP * sizeof(fgo_plane_propagate_pred)};
  int h_slot[5];
  for (int k = 0; k < 5; ++k) h_slot[k] = S.out(slot_host[k], slot_bytes[k]);
  const int h_label = S.out(label_out, n * np);
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  for (int k = 0; k < 5; ++k)                                   // the slots past a pair's last plane stay zero
    if (slot_host[k] && hipMemset(S.ptr<char>(h_slot[k]), 0, slot_bytes[k]) != hipSuccess) return FGO_ENUM;
  PpArgs A;
  A.n = n_pairs; A.W = width; A.H = height; A.NP = (int)np;
  A.depth = S.ptr<uint16_t>(h_depth); A.inten = S.ptr<uint8_t>(h_int); A.label = S.ptr<int8_t>(h_lab);
  A.n_planes = S.ptr<int32_t>(h_npl); A.abcd = S.ptr<double>(h_abcd); A.cov16 = S.ptr<double>(h_c16);
  A.fi = S.ptr<int64_t>(h_fi); A.fj = S.ptr<int64_t>(h_fj);
  A.pose = S.ptr<double>(h_pose); A.info = S.ptr<double>(h_info); A.cov = S.ptr<double>(h_cov);
  A.fx = P.fx; A.fy = P.fy; A.cx = P.cx; A.cy = P.cy; A.z_scale = P.z_scale; A.z_min = P.z_min; A.z_max = P.z_max;
  A.s_px2 = P.sigma_px * P.sigma_px; A.sz0 = P.sigma_z[0]; A.sz1 = P.sigma_z[1]; A.sz2 = P.sigma_z[2];
  A.dfl2 = P.d_floor * P.d_floor; A.keep_ratio = P.keep_ratio;
  A.tol = P.intensity_tol; A.rest_thresh = (int)(P.rest_ratio * (double)np);
  A.pts = S.ptr<double>(h_pts); A.flag = lds ? nullptr : S.ptr<uint8_t>(h_flag);
  A.res = S.ptr<fgo_plane_propagate_result>(h_res);
  A.abcd_out = S.ptr<double>(h_slot[0]); A.cov16_out = S.ptr<double>(h_slot[1]); A.ut6 = S.ptr<double>(h_slot[2]);
  A.plane = S.ptr<fgo_plane_propagate_plane>(h_slot[3]); A.pred = S.ptr<fgo_plane_propagate_pred>(h_slot[4]);
  A.label_out = S.ptr<int8_t>(h_label);
  const size_t lds_bytes = lds ? 2 * ((np + 15) & ~(size_t)15) : 0;
  if (lds && hipFuncSetAttribute(reinterpret_cast<const void *>(&k_plane_propagate<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds_bytes) != hipSuccess)
    return FGO_ENUM;
  KernelTimer timer;
  if (!timer.start()) return FGO_ENUM;
  if (lds) hipLaunchKernelGGL(k_plane_propagate<true>, dim3((unsigned)n_pairs), dim3(PX_T), lds_bytes, 0, A);
  else hipLaunchKernelGGL(k_plane_propagate<false>, dim3((unsigned)n_pairs), dim3(PX_T), 0, 0, A);
  timer.stop();
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  g_pp_kernel_ms = timer.ms();
  return S.download();
}
