// Descriptor matching of key-frame pairs on the MI355X (gfx950, wave64): CCameraNode::matchNodePair before its RANSAC
// (g2o/g2o_graph.cpp:174,210-211, gtsam/gtsam_graph.cpp:1730-1731) and the pose-guided matchNodePairBA of CGraphGT::vroAdjust
// (gtsam/gtsam_graph.cpp:450-498) -- nearest and second-nearest neighbour over 128-byte descriptors, the ratio test, an absolute cap
// and the cross-check -- for ONE pair of frames.  include/fgo.h states the semantics, tests/feature_match_reference.py restates them
// in numpy.  The pairs are independent: fgo_match_features_batch runs ONE WORKGROUP (FM_T threads, four waves) PER PAIR and all
// pairs in one launch, after one launch over the features (k_match_norms: the integer norm of a descriptor, -1 for a feature
// without a usable point).
//
//   distance  exact integers.  A descriptor byte u is read as the int8 u ^ 0x80 = u - 128; a common shift changes no distance, and
//             d(a, b) = |a'|^2 + |b'|^2 - 2 a'.b' with a'.b' on v_mfma_i32_16x16x64_i8: two K-steps per 16 x 16 tile, |a'.b'| <= 2^21.
//             Lane l holds bytes [64 s + 16 (l >> 4), + 16) of row (l & 15) in K-step s for A (queries) and B (trains) alike, so the
//             placement of k inside a fragment cannot change the sum; D: train column l & 15, query row 4 (l >> 4) + reg.
//   queries   blocks of FM_QB = 256 queries: a wave owns four 16-query strips whose A fragments, norms, best, second and index stay
//             in registers while the trains go by; a B fragment is read once and serves the four strips.
//   trains    chunks of FM_TC = 128 descriptors staged in LDS (16 KB), 16-byte slot c of row r stored at slot c ^ (r & 7): the
//             ds_read_b128 of a B fragment puts every 16-lane group on 16 different slots.  With the chunk: the train norms (-1: not
//             a candidate of any query) and, for a guided pair, the train's point in frame j and its projection, in f64; the
//             points and pixels of the block's queries are staged with the block's first chunk.
//   rows      a lane keeps (d1, b1, d2) for its 4 rows of a strip -- the trains reach it in ascending b, so a strict compare
//             keeps the lowest index of a tie -- and the 16 lanes of a row are merged after the last chunk by a butterfly on
//             (d, b), compared lexicographically: second = min(the loser's best, the winner's second).
//   columns   for the cross-check, an LDS array of N_i packed keys (d << 32 | a) under 64-bit integer atomicMin: the minimum of a
//             set, whatever the order.  A wave first reduces its 64 rows of the column (16 per lane, then the four lane groups by
//             two shuffles), and one lane per column issues the atomic.
//   verdict   after the last block the threads stride the queries: reason 0 .. 5 from (d1, b1, d2) and the column minimum of b1.
// No floating-point atomics; every barrier is outside every branch that is not uniform over the workgroup (the block loop, the
// chunk loop and the guided flag are uniform); loop bounds are fixed before the loops.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <climits>
#include <cmath>
#include <vector>
#include "../../include/fgo.h"
#include "batch_call.hpp"

namespace fgo {
namespace {

constexpr int FM_T = 256, FM_WAVES = 4, FM_STRIPS = 4;      // threads, waves, 16-query strips per wave
constexpr int FM_QB = 16 * FM_STRIPS * FM_WAVES;            // queries per block: 256
constexpr int FM_TC = 128;                                  // trains per LDS chunk
static_assert(FM_QB == FM_T, "a thread stages one query of the block");
constexpr int FM_NONE = INT_MAX;                            // "no distance": larger than any (<= 8 323 200)
constexpr unsigned long long FM_NOKEY = ~0ull;

typedef int v4i __attribute__((ext_vector_type(4)));

struct FmArgs {
  const int64_t *feat_ptr, *fi, *fj, *q_ptr, *dist_ptr;
  const uint8_t *desc;
  const double *xyz, *uv, *pose;
  const uint8_t *guided;
  const int32_t *nrm;
  int32_t *best, *d1, *d2, *dist;                           // dist may be NULL
  uint8_t *reason;
  double fx, fy, cx, cy, radius2, max3d2, r2;
  int ratio_test, cross_check, max_desc;
};

__device__ inline bool usable_point(const double *p) {
  return fabs(p[0]) < HUGE_VAL && fabs(p[1]) < HUGE_VAL && fabs(p[2]) < HUGE_VAL && p[2] > 0;     // a NaN fails every compare
}

// one thread per feature: |u - 128|^2 summed over the 128 bytes (<= 128 * 128^2 = 2^21), -1 for a feature that never matches
__global__ __launch_bounds__(256) void k_match_norms(int64_t F, const uint8_t *__restrict__ desc, const double *__restrict__ xyz,
                                                      int32_t *__restrict__ nrm) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  int s = -1;
  if (usable_point(xyz + 3 * f)) {
    const uint4 *__restrict__ row = reinterpret_cast<const uint4 *>(desc + f * FGO_FM_DIM);
    s = 0;
#pragma unroll
    for (int c = 0; c < FGO_FM_DIM / 16; ++c) {
      const uint4 w = row[c];
      const uint32_t v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int e = (int)((v[k] >> (8 * b)) & 255u) - 128;
          s += e * e;
        }
    }
  }
  nrm[f] = s;
}

__device__ inline v4i flip(uint4 w) {
  return v4i{(int)(w.x ^ 0x80808080u), (int)(w.y ^ 0x80808080u), (int)(w.z ^ 0x80808080u), (int)(w.w ^ 0x80808080u)};
}

__global__ __launch_bounds__(FM_T, 2) void k_match(FmArgs A) {
  __shared__ __attribute__((aligned(16))) uint8_t s_desc[FM_TC * FGO_FM_DIM];      // the train chunk, slots swizzled
  __shared__ unsigned long long s_col[FGO_FM_MAX_FEATURES];                        // column minima (d << 32 | a)
  __shared__ int s_nb[FM_TC];                                                      // train norms of the chunk, -1: no candidate
  __shared__ double s_tp[5][FM_TC];                                                // guided: p.x, p.y, p.z, u, v of the train in frame j
  __shared__ double s_pose[12];                                                   // guided: R (row major), t
  __shared__ double s_q[5][FM_QB];                                                 // guided: x, y, z, u, v of the block's queries
  const int64_t pair = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lg = lane >> 4;
  const int64_t fi = A.fi[pair], fj = A.fj[pair];
  const int64_t i0 = A.feat_ptr[fi], j0 = A.feat_ptr[fj], q0 = A.q_ptr[pair];
  const int Ni = (int)(A.feat_ptr[fi + 1] - i0), Nj = (int)(A.feat_ptr[fj + 1] - j0);
  const bool guided = A.guided[pair] != 0;
  int32_t *__restrict__ dist = A.dist ? A.dist + A.dist_ptr[pair] : nullptr;

  // ---- the pose of a guided pair: p_j = R^T (p_i - t); read after the first barrier of the chunk loop
  if (guided && tid == 0) {
    const double *__restrict__ ps = A.pose + 7 * pair;
    const double qn = sqrt(ps[3] * ps[3] + ps[4] * ps[4] + ps[5] * ps[5] + ps[6] * ps[6]);
    const double x = ps[3] / qn, y = ps[4] / qn, z = ps[5] / qn, w = ps[6] / qn;
    double *R = s_pose, *t = s_pose + 9;
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
    t[0] = ps[0]; t[1] = ps[1]; t[2] = ps[2];
  }
  for (int b = tid; b < Ni; b += FM_T) s_col[b] = FM_NOKEY;

  const int n_blocks = (Nj + FM_QB - 1) / FM_QB, n_chunks = (Ni + FM_TC - 1) / FM_TC;
  for (int qb = 0; qb < n_blocks; ++qb) {
    // ---- the wave's strips: A fragments, norms, and the running (d1, b1, d2) of the lane's 4 rows
    const int w0 = qb * FM_QB + wave * 16 * FM_STRIPS;       // first query of the wave in this block
    v4i a0[FM_STRIPS], a1[FM_STRIPS];
    int na[FM_STRIPS][4], d1[FM_STRIPS][4], b1[FM_STRIPS][4], d2[FM_STRIPS][4];
#pragma unroll
    for (int s = 0; s < FM_STRIPS; ++s) {
      const int a = w0 + 16 * s + lc;                        // the row this lane loads
      a0[s] = a1[s] = v4i{0, 0, 0, 0};
      if (a < Nj) {
        const uint4 *__restrict__ row = reinterpret_cast<const uint4 *>(A.desc + (j0 + a) * FGO_FM_DIM);
        a0[s] = flip(row[lg]);
        a1[s] = flip(row[4 + lg]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ar = w0 + 16 * s + 4 * lg + r;             // the rows this lane receives
        na[s][r] = ar < Nj ? A.nrm[j0 + ar] : -1;
        d1[s][r] = FM_NONE; b1[s][r] = FM_NONE; d2[s][r] = FM_NONE;
      }
    }

    for (int ch = 0; ch < n_chunks; ++ch) {
      const int c0 = ch * FM_TC;
      __syncthreads();                                       // the chunk before this one has been read
      // ---- stage: 1024 16-byte slots, four per thread; rows past N_i are zero
#pragma unroll
      for (int k = 0; k < FM_TC * 8 / FM_T; ++k) {
        const int slot = tid + k * FM_T, r = slot >> 3, c = slot & 7;
        v4i v = {0, 0, 0, 0};
        if (c0 + r < Ni) v = flip(reinterpret_cast<const uint4 *>(A.desc + (i0 + c0 + r) * FGO_FM_DIM)[c]);
        *reinterpret_cast<v4i *>(s_desc + r * FGO_FM_DIM + ((c ^ (r & 7)) << 4)) = v;
      }
      if (guided && ch == 0) {                               // one query per thread: FM_QB == FM_T
        const int64_t f = j0 + min(qb * FM_QB + tid, Nj - 1);
        s_q[0][tid] = A.xyz[3 * f]; s_q[1][tid] = A.xyz[3 * f + 1]; s_q[2][tid] = A.xyz[3 * f + 2];
        s_q[3][tid] = A.uv[2 * f]; s_q[4][tid] = A.uv[2 * f + 1];
      }
      if (tid < FM_TC) {
        const int b = c0 + tid;
        int nb = b < Ni ? A.nrm[i0 + b] : -1;
        if (guided && nb >= 0) {
          const double *__restrict__ x = A.xyz + 3 * (i0 + b), *R = s_pose, *t = s_pose + 9;
          const double e0 = x[0] - t[0], e1 = x[1] - t[1], e2 = x[2] - t[2];
          const double px = R[0] * e0 + R[3] * e1 + R[6] * e2, py = R[1] * e0 + R[4] * e1 + R[7] * e2, pz = R[2] * e0 + R[5] * e1 + R[8] * e2;
          if (pz > 0) {
            s_tp[0][tid] = px; s_tp[1][tid] = py; s_tp[2][tid] = pz;
            s_tp[3][tid] = A.fx * px / pz + A.cx; s_tp[4][tid] = A.fy * py / pz + A.cy;
          } else nb = -1;
        }
        s_nb[tid] = nb;
      }
      __syncthreads();

      const int n_tiles = w0 < Nj ? (min(Ni - c0, FM_TC) + 15) >> 4 : 0;     // uniform over the wave; no barrier below
      for (int tile = 0; tile < n_tiles; ++tile) {
        const int row = 16 * tile + lc;                      // the train this lane loads and receives
        const v4i f0 = *reinterpret_cast<const v4i *>(s_desc + row * FGO_FM_DIM + ((lg ^ (row & 7)) << 4));
        const v4i f1 = *reinterpret_cast<const v4i *>(s_desc + row * FGO_FM_DIM + (((4 + lg) ^ (row & 7)) << 4));
        const int nb = s_nb[row], b = c0 + row;
        int cm = FM_NONE, ca = 0;                            // the column over the wave's rows: (d, a), the lowest a of a tie
#pragma unroll
        for (int s = 0; s < FM_STRIPS; ++s) {
          const int r0 = w0 + 16 * s;
          if (r0 >= Nj) continue;                            // uniform over the wave
          const int abase = r0 + 4 * lg;                     // the lane's first row
          const int ql = wave * 16 * FM_STRIPS + 16 * s + 4 * lg;   // the same row in the block
          v4i acc = {0, 0, 0, 0};
          acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0[s], f0, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1[s], f1, acc, 0, 0, 0);
          int dd[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) dd[r] = (nb >= 0 && na[s][r] >= 0) ? na[s][r] + nb - 2 * acc[r] : FM_NONE;
          if (guided && nb >= 0) {
            const double px = s_tp[0][row], py = s_tp[1][row], pz = s_tp[2][row], pu = s_tp[3][row], pv = s_tp[4][row];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const double du = pu - s_q[3][ql + r], dv = pv - s_q[4][ql + r];
              bool in = du * du + dv * dv <= A.radius2;
              if (A.max3d2 > 0) {
                const double ex = px - s_q[0][ql + r], ey = py - s_q[1][ql + r], ez = pz - s_q[2][ql + r];
                in = in && ex * ex + ey * ey + ez * ez <= A.max3d2;
              }
              if (!in) dd[r] = FM_NONE;
            }
          }
          if (dist && b < Ni) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (abase + r < Nj) dist[(int64_t)(abase + r) * Ni + b] = dd[r] == FM_NONE ? -1 : dd[r];
          }
          // rows: strict compare, the trains come in ascending b; column: strict compare, the rows come in ascending a
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int d = dd[r];
            const bool better = d < d1[s][r];
            d2[s][r] = better ? d1[s][r] : min(d2[s][r], d);
            b1[s][r] = better ? b : b1[s][r];
            d1[s][r] = better ? d : d1[s][r];
            if (d < cm) { cm = d; ca = abase + r; }
          }
          __builtin_amdgcn_sched_barrier(0);                 // the strips one after the other: the form that was measured
        }
        // the four lane groups hold other rows of the same column: merge on (d, a); one lane per column goes to LDS, and only
        // with a distance that is not above the one already there (the stored d never grows, so a stale read only costs an atomic)
#pragma unroll
        for (int m = 16; m < 64; m <<= 1) {
          const int ym = __shfl_xor(cm, m), ya = __shfl_xor(ca, m);
          const bool other = ym < cm || (ym == cm && ya < ca);
          cm = other ? ym : cm;
          ca = other ? ya : ca;
        }
        if (lg == 0 && cm != FM_NONE && (unsigned)cm <= reinterpret_cast<const volatile unsigned *>(&s_col[b])[1])
          atomicMin(&s_col[b], ((unsigned long long)(unsigned)cm << 32) | (unsigned)ca);
      }
    }

    // ---- merge the 16 lanes of a row: lexicographic (d, b); then lane 0 of the row group writes its 4 rows
#pragma unroll
    for (int s = 0; s < FM_STRIPS; ++s) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int x1 = d1[s][r], xb = b1[s][r], x2 = d2[s][r];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
          const int y1 = __shfl_xor(x1, m), yb = __shfl_xor(xb, m), y2 = __shfl_xor(x2, m);
          const bool other = y1 < x1 || (y1 == x1 && yb < xb);
          x2 = other ? min(x1, y2) : min(x2, y1);
          x1 = other ? y1 : x1;
          xb = other ? yb : xb;
        }
        const int a = w0 + 16 * s + 4 * lg + r;
        if (lc == 0 && a < Nj) {
          A.best[q0 + a] = x1 == FM_NONE ? -1 : xb;
          A.d1[q0 + a] = x1 == FM_NONE ? -1 : x1;
          A.d2[q0 + a] = x2 == FM_NONE ? -1 : x2;
        }
      }
    }
  }
  __syncthreads();                                           // the column minima and the workgroup's own writes of best, d1, d2

  // ---- verdict
  for (int a = tid; a < Nj; a += FM_T) {
    const int bb = A.best[q0 + a], x1 = A.d1[q0 + a], x2 = A.d2[q0 + a];
    uint8_t why = 0;
    if (A.nrm[j0 + a] < 0) why = 1;
    else if (bb < 0) why = 2;
    else if (A.ratio_test && x2 >= 0 && !((double)x1 < A.r2 * (double)x2)) why = 3;
    else if (x1 > A.max_desc) why = 4;
    else if (A.cross_check && (int)(s_col[bb] & 0xffffffffull) != a) why = 5;
    A.reason[q0 + a] = why;
  }
}

double g_fm_kernel_ms = 0.0;

}  // namespace
}  // namespace fgo

extern "C" double fgo_debug_match_kernel_ms(void) { return fgo::g_fm_kernel_ms; }

extern "C" void fgo_match_params_default(fgo_match_params *p) {
  if (!p) return;
  p->ratio = 0.5;
  p->ratio_test = 1;
  p->cross_check = 1;
  p->max_desc_dist2 = INT32_MAX;
  p->min_matches = 12;
  p->radius_px = 10.0;
  p->max_dist_3d = 0.0;
  p->fx = p->fy = 250.5773;
  p->cx = 90.0; p->cy = 70.0;
}

extern "C" int fgo_match_features_batch(int device, int64_t n_frames, const int64_t *feat_ptr, const uint8_t *desc, const double *xyz,
                                        const double *uv, int64_t n_pairs, const int64_t *frame_i, const int64_t *frame_j,
                                        const double *pose_ij7, const uint8_t *guided, const fgo_match_params *params,
                                        fgo_match_result *result, int64_t *q_ptr_out, int32_t *best_out, int32_t *d1_out, int32_t *d2_out,
                                        uint8_t *reason_out, int64_t *match_ptr_out, int64_t *idx_i_out, int64_t *idx_j_out,
                                        double *xyz_i_out, double *xyz_j_out, double *uv_i_out, double *uv_j_out, int32_t *dist_out) {
  using namespace fgo;
  fgo_match_params P;
  fgo_match_params_default(&P);
  if (params) P = *params;
  if (n_frames < 0 || n_frames > INT_MAX || n_pairs < 0 || n_pairs > INT_MAX) return FGO_EINVAL;
  if (!(P.ratio > 0 && P.ratio <= 1) || !(P.radius_px > 0) || !(P.fx > 0) || !(P.fy > 0)) return FGO_EINVAL;
  if (!(P.radius_px < HUGE_VAL) || !(P.fx < HUGE_VAL) || !(P.fy < HUGE_VAL) || !(fabs(P.cx) < HUGE_VAL) || !(fabs(P.cy) < HUGE_VAL)) return FGO_EINVAL;
  if (!(P.max_dist_3d >= 0) || !(P.max_dist_3d < HUGE_VAL) || P.max_desc_dist2 < 0 || P.min_matches < 0) return FGO_EINVAL;
  if (n_pairs == 0) return FGO_OK;
  if (!feat_ptr || !desc || !xyz || !uv || !frame_i || !frame_j || !result || !match_ptr_out || !idx_i_out || !idx_j_out) return FGO_EINVAL;
  if (!csr_ptr_ok(feat_ptr, n_frames, FGO_FM_MAX_FEATURES)) return FGO_EINVAL;
  for (int64_t p = 0; p < n_pairs; ++p) {
    if (frame_i[p] < 0 || frame_i[p] >= n_frames || frame_j[p] < 0 || frame_j[p] >= n_frames) return FGO_EINVAL;
    if (pose_ij7 && (!guided || guided[p]) && !quat_ok(pose_ij7 + 7 * p + 3)) return FGO_EINVAL;
  }
  const size_t n = (size_t)n_pairs, nf = (size_t)n_frames;
  const int64_t F = feat_ptr[n_frames];                                // the arrays are indexed by feat_ptr's own values
  std::vector<int64_t> q_ptr(n + 1), dist_ptr(n + 1);
  std::vector<uint8_t> g(n);
  q_ptr[0] = dist_ptr[0] = 0;
  for (size_t p = 0; p < n; ++p) {
    const int64_t Ni = feat_ptr[frame_i[p] + 1] - feat_ptr[frame_i[p]], Nj = feat_ptr[frame_j[p] + 1] - feat_ptr[frame_j[p]];
    q_ptr[p + 1] = q_ptr[p] + Nj;
    dist_ptr[p + 1] = dist_ptr[p] + Nj * Ni;
    g[p] = pose_ij7 && (!guided || guided[p]) ? 1 : 0;
  }
  const size_t Q = (size_t)q_ptr[n];
  if (int rc = select_device(device)) return rc;

  // outputs the packing needs whether or not the caller wants them
  std::vector<int32_t> best_own;
  std::vector<uint8_t> reason_own;
  if (!best_out) { best_own.resize(Q ? Q : 1); best_out = best_own.data(); }
  if (!reason_out) { reason_own.resize(Q ? Q : 1); reason_out = reason_own.data(); }
  Staged S;
  const size_t D = sizeof(double), I8 = sizeof(int64_t);
  const int h_fp = S.in(feat_ptr, (nf + 1) * I8), h_desc = S.in(desc, (size_t)F * FGO_FM_DIM), h_xyz = S.in(xyz, 3 * (size_t)F * D);
  const int h_uv = S.in(uv, 2 * (size_t)F * D), h_fi = S.in(frame_i, n * I8), h_fj = S.in(frame_j, n * I8);
  const int h_pose = S.in(pose_ij7, 7 * n * D), h_g = S.in(g.data(), n), h_q = S.in(q_ptr.data(), (n + 1) * I8);
  const int h_dp = S.in(dist_ptr.data(), (n + 1) * I8);
  const int h_nrm = S.out(nullptr, (size_t)F * sizeof(int32_t), true);
  const int h_best = S.out(best_out, Q * sizeof(int32_t)), h_d1 = S.out(d1_out, Q * sizeof(int32_t), true);
  const int h_d2 = S.out(d2_out, Q * sizeof(int32_t), true), h_why = S.out(reason_out, Q);
  const int h_dist = S.out(dist_out, (size_t)dist_ptr[n] * sizeof(int32_t));
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  FmArgs A;
  A.feat_ptr = S.ptr<int64_t>(h_fp); A.fi = S.ptr<int64_t>(h_fi); A.fj = S.ptr<int64_t>(h_fj);
  A.q_ptr = S.ptr<int64_t>(h_q); A.dist_ptr = S.ptr<int64_t>(h_dp);
  A.desc = S.ptr<uint8_t>(h_desc); A.xyz = S.ptr<double>(h_xyz); A.uv = S.ptr<double>(h_uv); A.pose = S.ptr<double>(h_pose);
  A.guided = S.ptr<uint8_t>(h_g); A.nrm = S.ptr<int32_t>(h_nrm);
  A.best = S.ptr<int32_t>(h_best); A.d1 = S.ptr<int32_t>(h_d1); A.d2 = S.ptr<int32_t>(h_d2); A.dist = S.ptr<int32_t>(h_dist);
  A.reason = S.ptr<uint8_t>(h_why);
  A.fx = P.fx; A.fy = P.fy; A.cx = P.cx; A.cy = P.cy;
  A.radius2 = P.radius_px * P.radius_px; A.max3d2 = P.max_dist_3d * P.max_dist_3d; A.r2 = P.ratio * P.ratio;
  A.ratio_test = P.ratio_test; A.cross_check = P.cross_check; A.max_desc = P.max_desc_dist2;
  KernelTimer timer;
  if (!timer.start()) return FGO_ENUM;
  if (F > 0) hipLaunchKernelGGL(k_match_norms, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, 0, F, A.desc, A.xyz, S.ptr<int32_t>(h_nrm));
  hipLaunchKernelGGL(k_match, dim3((unsigned)n_pairs), dim3(FM_T), 0, 0, A);
  timer.stop();
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  g_fm_kernel_ms = timer.ms();
  if (int rc = S.download()) return rc;

  // ---- the host packs: the kept queries of a pair in ascending a, the counts of the pair
  std::vector<int32_t> n_usable(nf);
  for (size_t f = 0; f < nf; ++f) {
    int c = 0;
    for (int64_t k = feat_ptr[f]; k < feat_ptr[f + 1]; ++k) {
      const double *x = xyz + 3 * k;
      c += std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]) && x[2] > 0;
    }
    n_usable[f] = c;
  }
  int64_t m = 0;
  match_ptr_out[0] = 0;
  for (size_t p = 0; p < n; ++p) {
    const int64_t i0 = feat_ptr[frame_i[p]], j0 = feat_ptr[frame_j[p]];
    fgo_match_result r = {FGO_FM_OK, n_usable[frame_j[p]], n_usable[frame_i[p]], 0, 0, 0};
    for (int64_t q = q_ptr[p]; q < q_ptr[p + 1]; ++q) {
      r.n_ratio += reason_out[q] == 3;
      r.n_cross += reason_out[q] == 5;
      if (reason_out[q] != 0) continue;
      const int64_t ki = i0 + best_out[q], kj = j0 + (q - q_ptr[p]);
      idx_i_out[m] = ki; idx_j_out[m] = kj;
      for (int c = 0; c < 3; ++c) {
        if (xyz_i_out) xyz_i_out[3 * m + c] = xyz[3 * ki + c];
        if (xyz_j_out) xyz_j_out[3 * m + c] = xyz[3 * kj + c];
      }
      for (int c = 0; c < 2; ++c) {
        if (uv_i_out) uv_i_out[2 * m + c] = uv[2 * ki + c];
        if (uv_j_out) uv_j_out[2 * m + c] = uv[2 * kj + c];
      }
      ++m; ++r.n_matches;
    }
    if (r.n_matches < P.min_matches) r.status = FGO_FM_TOO_FEW;
    result[p] = r;
    match_ptr_out[p + 1] = m;
  }
  if (q_ptr_out)
    for (size_t p = 0; p <= n; ++p) q_ptr_out[p] = q_ptr[p];
  return FGO_OK;
}
