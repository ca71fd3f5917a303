// Hand-written HIP kernels for gfx950 (MI355X, wave64) -- the graph side of the optimiser hot path:
//   k_linearize      EdgeSE3::computeError + linearizeOplus + constructQuadraticForm   (HOT LOOP 1+2)
//   k_update         VertexSE3::oplusImpl over all vertices + the LM 'scale' reduction
//   k_chi2           computeActiveErrors + chi2
//   k_reduce, k_maxdiag, and the one-line utility kernels (zero, copy, mix, scatter, pack, fetch, mask) that keep a trial capturable
// replacing what the reference reaches through mp_optimizer->optimize() (g2o/g2o_graph.cpp:246-249)
// and computeActiveErrors()/chi2() (g2o/g2o_graph.cpp:256-257).  The factor sweep is in kernels_factor.hip, the triangular solves
// in kernels_solve.hip, the launch thresholds in launch_select.cpp.
//
// Determinism: no floating-point atomics anywhere.  H and b are produced in "gather" form (every
// output block is written once by one lane group that sums its incident half-edges in a fixed order);
// Cholesky targets are owned by one wave; reductions are two-pass with a fixed tree.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_plan.hpp"
#include "fgo_internal.hpp"
#include "se3_device.hpp"
#include "small_dense_device.hpp"
#include "sweep_device.hpp"

namespace fgo {
using namespace dev;

// block-level deterministic sum: wave shuffles, then LDS across waves (fixed order)
template <int NW>
__device__ __forceinline__ double block_sum(double v, double *sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double s = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) s += sh[i];
  }
  __syncthreads();
  return s;   // valid on thread 0
}

// edge record (device_plan.hpp: EDGE_REC doubles, 256-byte aligned): 16-byte loads
__device__ __forceinline__ Pose load_ainv(const double *__restrict__ ainv, int64_t, int64_t e) {
  const double2 *__restrict__ r = reinterpret_cast<const double2 *>(ainv + EDGE_REC * e);
  const double2 a = r[0], b = r[1], c = r[2], d = r[3];
  Pose A;
  A.t = {a.x, a.y, b.x};
  A.q = {b.y, c.x, c.y, d.x};
  return A;
}

struct Info3 { M3 tt, tq, qq; };   // Omega = [[tt, tq], [tq^T, qq]]
__device__ __forceinline__ Info3 load_info(const double *__restrict__ info, int64_t, int64_t e) {
  double u[22];
  const double2 *__restrict__ r = reinterpret_cast<const double2 *>(info + EDGE_REC * e);
#pragma unroll
  for (int c = 0; c < 11; ++c) { const double2 v = r[c]; u[2 * c] = v.x; u[2 * c + 1] = v.y; }
  // upper-triangular row-major: row0: 0..5, row1: 6..10, row2: 11..14, row3: 15..17, row4: 18..19, row5: 20
  Info3 W;
  W.tt = {{u[0], u[1], u[2], u[1], u[6], u[7], u[2], u[7], u[11]}};
  W.tq = {{u[3], u[4], u[5], u[8], u[9], u[10], u[12], u[13], u[14]}};
  W.qq = {{u[15], u[16], u[17], u[16], u[18], u[19], u[17], u[19], u[20]}};
  return W;
}

// ------------------------------------------------------------------------------------------------
// Linearise + assemble, gather form.  G lanes cooperate on one pose: its incident half-edges are dealt
// round-robin to the G lanes, each lane evaluates residual + Jacobians of its half-edges and keeps
// J_s^T Omega J_s and -J_s^T Omega e in registers; a fixed xor-tree over the G lanes finishes the sum.
// The j-side half-edge of an edge also owns its off-diagonal block J_i^T Omega J_j and its chi2 term.
// HBM traffic per launch: one 256-byte edge record (two whole lines) per half-edge, poses gathered (64 B each),
// H diag/off-diag + b written once.
// HUB = true: a pose with more than HUB_DEG half-edges (skipped by the HUB = false launch) gets a whole 256-thread
// workgroup (blockIdx -> P.hub_list) instead of G lanes; the partial sums go through a fixed shuffle tree + LDS.
template <int G, bool HUB>
__global__ __launch_bounds__(256) void k_linearize(DevPlan P, const double *__restrict__ poses,
                                                   double *__restrict__ Hblk, double *__restrict__ bvec,
                                                   double *__restrict__ chi_partial) {
  __shared__ double sh[4];
  __shared__ double red[4][33];
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t v = HUB ? (int64_t)P.hub_list[blockIdx.x] : tid / G;
  const int hs = HUB ? P.hub_slice[blockIdx.x] : 0x10000;          // slice | slices << 16
  const int sl = hs & 0xffff, ns = hs >> 16;
  const int g = HUB ? sl * 256 + (int)threadIdx.x : (int)(tid % G);
  const int STRIDE = HUB ? 256 * ns : G;
  M3 Dtt = mzero(), Dtq = mzero(), Dqq = mzero();
  double gt[3] = {0, 0, 0}, gq[3] = {0, 0, 0};
  double chi = 0;
  bool live = v < P.n_poses;
  if (!HUB && live && P.n_hubs > 0 && P.he_ptr[v + 1] - P.he_ptr[v] > P.hub_deg) live = false;
  if (live) {
    const int64_t p0 = P.he_ptr[v], p1 = P.he_ptr[v + 1];
    for (int64_t p = p0 + g; p < p1; p += STRIDE) {
      const int he = P.he[p];
      const int64_t e = he >> 1;
      const int side = he & 1;                 // 1: this pose is vertex j of the edge
      const int vi = P.edge_i[e], vj = P.edge_j[e];
      const Pose Xi = load_pose(poses + 8 * (int64_t)vi), Xj = load_pose(poses + 8 * (int64_t)vj);
      const Pose A = load_ainv(P.ainv, P.edge_stride, e);
      const Info3 W = load_info(P.info, P.edge_stride, e);
      EdgeLin L;
      edge_se3<true>(Xi, Xj, A, L);
      const V3 et = {L.e[0], L.e[1], L.e[2]}, eq = {L.e[3], L.e[4], L.e[5]};
      const V3 Wt = mv(W.tt, et) + mv(W.tq, eq);          // (Omega e)_t
      const V3 Wq = mtv(W.tq, et) + mv(W.qq, eq);         // (Omega e)_q
      if (side) {
        chi += et.x * Wt.x + et.y * Wt.y + et.z * Wt.z + eq.x * Wq.x + eq.y * Wq.y + eq.z * Wq.z;
        // X = Omega Jj, Jj = [[Aj, 0], [0, Cj]]
        const M3 X11 = mm(W.tt, L.Aj), X21 = mtm(W.tq, L.Aj), X12 = mm(W.tq, L.Cj), X22 = mm(W.qq, L.Cj);
        Dtt = madd(Dtt, mtm(L.Aj, X11));
        Dtq = madd(Dtq, mtm(L.Aj, X12));
        Dqq = madd(Dqq, mtm(L.Cj, X22));
        const V3 a = mtv(L.Aj, Wt), c = mtv(L.Cj, Wq);
        gt[0] -= a.x; gt[1] -= a.y; gt[2] -= a.z;
        gq[0] -= c.x; gq[1] -= c.y; gq[2] -= c.z;
        const int slot = P.edge_slot[e];
        if (slot >= 0) {
          // O = Ji^T X  (rows: tangent of i, cols: tangent of j)
          const M3 Ott = mtm(L.Ai, X11), Otq = mtm(L.Ai, X12);
          const M3 Oqt = madd(mtm(L.Bi, X11), mtm(L.Ci, X21)), Oqq = madd(mtm(L.Bi, X12), mtm(L.Ci, X22));
          // the block in registers first, then 18 sixteen-byte stores in address order (whole lines leave the L2 once)
          double blk[36];
          if ((slot & 1) == 0) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
              for (int c2 = 0; c2 < 3; ++c2) {
                blk[r * 6 + c2] = Ott.m[r * 3 + c2]; blk[r * 6 + 3 + c2] = Otq.m[r * 3 + c2];
                blk[(3 + r) * 6 + c2] = Oqt.m[r * 3 + c2]; blk[(3 + r) * 6 + 3 + c2] = Oqq.m[r * 3 + c2];
              }
          } else {   // store O^T (block row = j)
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
              for (int c2 = 0; c2 < 3; ++c2) {
                blk[c2 * 6 + r] = Ott.m[r * 3 + c2]; blk[(3 + c2) * 6 + r] = Otq.m[r * 3 + c2];
                blk[c2 * 6 + 3 + r] = Oqt.m[r * 3 + c2]; blk[(3 + c2) * 6 + 3 + r] = Oqq.m[r * 3 + c2];
              }
          }
          double2 *__restrict__ o2 = reinterpret_cast<double2 *>(Hblk + 36 * (int64_t)(slot >> 1));
#pragma unroll
          for (int k = 0; k < 18; ++k) o2[k] = make_double2(blk[2 * k], blk[2 * k + 1]);
        }
      } else {
        // X = Omega Ji, Ji = [[Ai, Bi], [0, Ci]]
        const M3 X11 = mm(W.tt, L.Ai);
        const M3 X12 = madd(mm(W.tt, L.Bi), mm(W.tq, L.Ci));
        const M3 X22 = madd(mtm(W.tq, L.Bi), mm(W.qq, L.Ci));
        Dtt = madd(Dtt, mtm(L.Ai, X11));
        Dtq = madd(Dtq, mtm(L.Ai, X12));
        Dqq = madd(Dqq, madd(mtm(L.Bi, X12), mtm(L.Ci, X22)));
        const V3 a = mtv(L.Ai, Wt), c = mtv(L.Bi, Wt) + mtv(L.Ci, Wq);
        gt[0] -= a.x; gt[1] -= a.y; gt[2] -= a.z;
        gq[0] -= c.x; gq[1] -= c.y; gq[2] -= c.z;
      }
    }
  }
  // fixed xor tree over the G lanes of a pose (HUB: over the wave, then the four wave totals in a fixed order)
#pragma unroll
  for (int o = 1; o < (HUB ? 64 : G); o <<= 1) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      Dtt.m[k] += __shfl_xor(Dtt.m[k], o, WAVE);
      Dtq.m[k] += __shfl_xor(Dtq.m[k], o, WAVE);
      Dqq.m[k] += __shfl_xor(Dqq.m[k], o, WAVE);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { gt[k] += __shfl_xor(gt[k], o, WAVE); gq[k] += __shfl_xor(gq[k], o, WAVE); }
  }
  if (HUB) {
    if ((threadIdx.x & 63) == 0) {
      double *rw = red[threadIdx.x >> 6];
#pragma unroll
      for (int k = 0; k < 9; ++k) { rw[k] = Dtt.m[k]; rw[9 + k] = Dtq.m[k]; rw[18 + k] = Dqq.m[k]; }
#pragma unroll
      for (int k = 0; k < 3; ++k) { rw[27 + k] = gt[k]; rw[30 + k] = gq[k]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        Dtt.m[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
        Dtq.m[k] = ((red[0][9 + k] + red[1][9 + k]) + red[2][9 + k]) + red[3][9 + k];
        Dqq.m[k] = ((red[0][18 + k] + red[1][18 + k]) + red[2][18 + k]) + red[3][18 + k];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        gt[k] = ((red[0][27 + k] + red[1][27 + k]) + red[2][27 + k]) + red[3][27 + k];
        gq[k] = ((red[0][30 + k] + red[1][30 + k]) + red[2][30 + k]) + red[3][30 + k];
      }
    }
  }
  if (HUB && ns > 1) {                         // one slice of several: the partial sums go to k_hub_combine
    if (threadIdx.x == 0) {
      double *o = P.hub_part + (int64_t)blockIdx.x * HUB_PART;
#pragma unroll
      for (int k = 0; k < 9; ++k) { o[k] = Dtt.m[k]; o[9 + k] = Dtq.m[k]; o[18 + k] = Dqq.m[k]; }
#pragma unroll
      for (int k = 0; k < 3; ++k) { o[27 + k] = gt[k]; o[30 + k] = gq[k]; }
    }
  } else if (live && (HUB ? threadIdx.x == 0 : g == 0)) {
    const int col = P.pose_col[v];
    if (col >= 0) {
      double *d = Hblk + 36 * (int64_t)col;
      const double slot_diag = v >= P.n_real ? 1.0 : 0.0;       // an unclaimed growth slot: identity block, zero gradient
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          d[r * 6 + c] = Dtt.m[r * 3 + c] + (r == c ? slot_diag : 0.0); d[r * 6 + 3 + c] = Dtq.m[r * 3 + c];
          d[(3 + r) * 6 + c] = Dtq.m[c * 3 + r]; d[(3 + r) * 6 + 3 + c] = Dqq.m[r * 3 + c] + (r == c ? slot_diag : 0.0);
        }
      double *b = bvec + 6 * (int64_t)col;
      b[0] = gt[0]; b[1] = gt[1]; b[2] = gt[2]; b[3] = gq[0]; b[4] = gq[1]; b[5] = gq[2];
    }
  }
  const double s = block_sum<4>(chi, sh);
  if (threadIdx.x == 0) chi_partial[blockIdx.x] = s;
}

// hubs linearised in several slices: the slices' partial sums in entry order, then the diagonal block and gradient
__global__ __launch_bounds__(64) void k_hub_combine(DevPlan P, double *__restrict__ Hblk, double *__restrict__ bvec) {
  __shared__ double sum[HUB_PART];
  const int v = P.hubm[3 * blockIdx.x], e0 = P.hubm[3 * blockIdx.x + 1], ns = P.hubm[3 * blockIdx.x + 2];
  if (threadIdx.x < 33) {
    double a = 0;
    for (int q = 0; q < ns; ++q) a += P.hub_part[(int64_t)(e0 + q) * HUB_PART + threadIdx.x];
    sum[threadIdx.x] = a;
  }
  __syncthreads();
  const int col = P.pose_col[v];
  if (col < 0) return;
  if (threadIdx.x < 36) {
    const int r = threadIdx.x / 6, c = threadIdx.x % 6;
    double x;
    if (r < 3 && c < 3) x = sum[r * 3 + c];
    else if (r < 3) x = sum[9 + r * 3 + (c - 3)];
    else if (c < 3) x = sum[9 + c * 3 + (r - 3)];
    else x = sum[18 + (r - 3) * 3 + (c - 3)];
    Hblk[36 * (int64_t)col + threadIdx.x] = x;
  } else if (threadIdx.x < 42) {
    bvec[6 * (int64_t)col + (threadIdx.x - 36)] = sum[27 + (threadIdx.x - 36)];
  }
}

// Off-diagonal blocks shared by several edges (same vertex pair added more than once): one lane per
// group sums the members serially and overwrites the slot.  Rare; keeps the common path write-once.
__global__ void k_dup_offdiag(DevPlan P, const double *__restrict__ poses, double *__restrict__ Hblk) {
  const int64_t gidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gidx >= P.n_dup_groups) return;
  double acc[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0;
  int slot = -1;
  for (int64_t p = P.dup_ptr[gidx]; p < P.dup_ptr[gidx + 1]; ++p) {
    const int64_t e = P.dup_edges[p];
    const int vi = P.edge_i[e], vj = P.edge_j[e];
    const Pose Xi = load_pose(poses + 8 * (int64_t)vi), Xj = load_pose(poses + 8 * (int64_t)vj);
    const Pose A = load_ainv(P.ainv, P.edge_stride, e);
    const Info3 W = load_info(P.info, P.edge_stride, e);
    EdgeLin L;
    edge_se3<true>(Xi, Xj, A, L);
    const M3 X11 = mm(W.tt, L.Aj), X21 = mtm(W.tq, L.Aj), X12 = mm(W.tq, L.Cj), X22 = mm(W.qq, L.Cj);
    const M3 Ott = mtm(L.Ai, X11), Otq = mtm(L.Ai, X12);
    const M3 Oqt = madd(mtm(L.Bi, X11), mtm(L.Ci, X21)), Oqq = madd(mtm(L.Bi, X12), mtm(L.Ci, X22));
    const int s = P.dup_slot[p];     // (block index << 1) | transpose, per member edge
    slot = s >> 1;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        if ((s & 1) == 0) {
          acc[r * 6 + c] += Ott.m[r * 3 + c]; acc[r * 6 + 3 + c] += Otq.m[r * 3 + c];
          acc[(3 + r) * 6 + c] += Oqt.m[r * 3 + c]; acc[(3 + r) * 6 + 3 + c] += Oqq.m[r * 3 + c];
        } else {
          acc[c * 6 + r] += Ott.m[r * 3 + c]; acc[(3 + c) * 6 + r] += Otq.m[r * 3 + c];
          acc[c * 6 + 3 + r] += Oqt.m[r * 3 + c]; acc[(3 + c) * 6 + 3 + r] += Oqq.m[r * 3 + c];
        }
      }
  }
  if (slot >= 0)
    for (int k = 0; k < 36; ++k) Hblk[36 * (int64_t)slot + k] = acc[k];
}

// chi2 only (CGraphG2O::error): edge-parallel, coalesced SoA reads
__global__ __launch_bounds__(256) void k_chi2(DevPlan P, const double *__restrict__ poses,
                                              double *__restrict__ chi_partial) {
  __shared__ double sh[4];
  double chi = 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < P.n_edges; e += (int64_t)gridDim.x * blockDim.x) {
    const Pose Xi = load_pose(poses + 8 * (int64_t)P.edge_i[e]), Xj = load_pose(poses + 8 * (int64_t)P.edge_j[e]);
    const Pose A = load_ainv(P.ainv, P.edge_stride, e);
    const Info3 W = load_info(P.info, P.edge_stride, e);
    EdgeLin L;
    edge_se3<false>(Xi, Xj, A, L);
    const V3 et = {L.e[0], L.e[1], L.e[2]}, eq = {L.e[3], L.e[4], L.e[5]};
    const V3 Wt = mv(W.tt, et) + mv(W.tq, eq);
    const V3 Wq = mtv(W.tq, et) + mv(W.qq, eq);
    chi += et.x * Wt.x + et.y * Wt.y + et.z * Wt.z + eq.x * Wq.x + eq.y * Wq.y + eq.z * Wq.z;
  }
  const double s = block_sum<4>(chi, sh);
  if (threadIdx.x == 0) chi_partial[blockIdx.x] = s;
}

// final pass of the two-pass reductions: one workgroup, fixed order.  mode 0: sum, 1: max
__global__ __launch_bounds__(256) void k_reduce(const double *__restrict__ partial, int64_t n, double *out, int mode) {
  __shared__ double sh[4];
  double acc = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) acc = mode ? fmax(acc, partial[i]) : acc + partial[i];
  if (mode) {
    acc = wave_max(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) *out = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
  } else {
    const double s = block_sum<4>(acc, sh);
    if (threadIdx.x == 0) *out = s;
  }
}

// computeLambdaInit: max |H_kk| over the diagonal blocks of the REAL variables -- the unclaimed slots of growth mode carry an identity
// block that is no part of the problem (with information far below 1 it would set lambda_0: ADVICE r5)
__global__ __launch_bounds__(256) void k_maxdiag(const double *__restrict__ Hblk, const int *__restrict__ pose_col, int64_t n_real, double *partial) {
  __shared__ double sh[4];
  double m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_real * 6; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / 6; const int r = (int)(i % 6);
    const int k = pose_col[v];
    if (k >= 0) m = fmax(m, fabs(Hblk[36 * (int64_t)k + 7 * r]));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// SparseOptimizer::update (oplus on every free vertex) into the candidate pose buffer, plus the
// LM 'scale' = sum_k x_k (lambda x_k + b_k)  (OptimizationAlgorithmLevenberg::computeScale)
__global__ __launch_bounds__(256) void k_update(DevPlan P, const double *__restrict__ poses,
                                                double *__restrict__ cand, const double *__restrict__ x,
                                                const double *__restrict__ b, const double *__restrict__ lambda_p,
                                                double *__restrict__ scale_partial) {
  __shared__ double sh[4];
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double sc = 0;
  if (v < P.n_poses) {
    Pose X = load_pose(poses + 8 * v);
    const int col = P.pose_col[v];
    if (col >= 0 && v < P.n_real) {                           // (growth slots hold no pose yet)
      const double lambda = *lambda_p;
      double d[6];
      const bool mine = !P.var_mine || P.var_mine[v];      // distributed: every column counted once (x of foreign domains is 0)
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        d[k] = x[6 * (int64_t)col + k];
        if (mine) sc += d[k] * (lambda * d[k] + b[6 * (int64_t)col + k]);
      }
      X = oplus(X, d);
    }
    store_pose(cand + 8 * v, X);
  }
  const double s = block_sum<4>(sc, sh);
  if (threadIdx.x == 0) scale_partial[blockIdx.x] = s;
}

// poses a rank is responsible for (its domain; rank 0: the top and the fixed ones), zeros elsewhere: the sum over the
// ranks is the complete estimate (end of fgo_optimize in distributed mode)
__global__ void k_mask_poses(int64_t n, const double *__restrict__ poses, double *__restrict__ out, const int *__restrict__ pose_group, int rank, int world) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 8) return;
  const int gq = pose_group[i >> 3];
  const bool mine = gq == rank || (rank == 0 && (gq < 0 || gq >= world));
  out[i] = mine ? poses[i] : 0.0;
}

// zero fill as a KERNEL: everything inside a captured LM trial is a kernel node.  (hipMemsetAsync nodes were seen to
// carry a garbage fill value -- 0x40404040 in the failure flag -- when a second host thread issued HIP calls while
// this thread's stream was being captured: tools/debug_dist.py)
__global__ void k_zero(double *__restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0.0;
}
__global__ void k_zero_int(int *__restrict__ p) { *p = 0; }

// partial sweep: the right-hand side of the columns that are re-solved, the saved forward solution y of all others
__global__ void k_mix_rhs(DevPlan P, const double *__restrict__ b, const double *__restrict__ ysaved, double *__restrict__ x, const unsigned char *__restrict__ col_dirty) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)P.nb * 6) return;
  x[i] = col_dirty[i / 6] ? b[i] : ysaved[i];
}
void launch_mix_rhs(const DevPlan &P, const double *b, const double *ysaved, double *x, const unsigned char *col_dirty, hipStream_t s) {
  hipLaunchKernelGGL(k_mix_rhs, dim3((unsigned)(((int64_t)P.nb * 6 + 255) / 256)), dim3(256), 0, s, P, b, ysaved, x, col_dirty);
}

// x (permuted) <- b (permuted): plain copy kept as a kernel so the whole trial is capturable in a hipGraph
__global__ void k_copy(const double *__restrict__ src, double *__restrict__ dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------
// host-callable launchers (no synchronisation, capturable)
void launch_zero(double *p, int64_t n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_zero, dim3(cdiv(n, 256) > 2048 ? 2048 : cdiv(n, 256)), dim3(256), 0, s, p, n);
}
__global__ void k_scatter_edges(const double *__restrict__ stage, int64_t n, int64_t e0, double *__restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 28) return;
  const int64_t e = i / 28; const int k = (int)(i - 28 * e);
  rec[EDGE_REC * (e0 + e) + (k < 7 ? k : k + 1)] = stage[i];            // [0..6] measurement, [8..28] information
}
void launch_scatter_edges(const double *stage, int64_t n, int64_t e0, double *rec, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_scatter_edges, dim3(cdiv(n * 28, 256)), dim3(256), 0, s, stage, n, e0, rec);
}
void launch_zero_flag(int *p, hipStream_t s) { hipLaunchKernelGGL(k_zero_int, dim3(1), dim3(1), 0, s, p); }
// distributed trial: [5] <- the failure flag, [6] <- the LM scale partial, next to [4] (chi2 partial): one collective for the three
// (host: pinned, device-visible host memory or NULL -- a single-GPU trial's three results go straight there: the 24-byte read-back as a blit
//  copy of its own cost ~18 us of stream time per trial, as did the 8-byte upload of lambda that k_fetch_scalar replaces; round 6)
__global__ void k_pack_scalars(double *__restrict__ scal, const int *__restrict__ fail, double *__restrict__ host) {
  const double f = (double)*fail, sc = scal[1];
  scal[5] = f; scal[6] = sc;
  if (host) { host[4] = scal[4]; host[5] = f; host[6] = sc; }
}
void launch_pack_scalars(double *scal, const int *fail, hipStream_t s, double *host) { hipLaunchKernelGGL(k_pack_scalars, dim3(1), dim3(1), 0, s, scal, fail, host); }
__global__ void k_fetch_scalar(double *__restrict__ dst, const double *__restrict__ src_host) { *dst = *reinterpret_cast<const volatile double *>(src_host); }
void launch_fetch_scalar(double *dst, const double *src_host, hipStream_t s) { hipLaunchKernelGGL(k_fetch_scalar, dim3(1), dim3(1), 0, s, dst, src_host); }

void launch_linearize(const DevPlan &P, const double *poses, double *Hblk, double *bvec, double *scalar_out,
                      hipStream_t s) {
  constexpr int G = 4;
  int blocks = cdiv(P.n_poses * G, 256);
  if (P.zero_offdiag)   // shard mode: off-diagonal blocks of edges owned by other ranks have no local writer
    launch_zero(Hblk + 36 * (int64_t)P.nb, 36 * (int64_t)(P.n_hblocks - P.nb), s);
  hipLaunchKernelGGL((k_linearize<G, false>), dim3(blocks), dim3(256), 0, s, P, poses, Hblk, bvec, P.partial);
  if (P.n_hubs > 0)
    hipLaunchKernelGGL((k_linearize<G, true>), dim3(P.n_hubs), dim3(256), 0, s, P, poses, Hblk, bvec, P.partial + blocks);
  if (P.n_hub_multi > 0) hipLaunchKernelGGL(k_hub_combine, dim3(P.n_hub_multi), dim3(64), 0, s, P, Hblk, bvec);
  blocks += P.n_hubs;
  if (P.n_dup_groups > 0)
    hipLaunchKernelGGL(k_dup_offdiag, dim3(cdiv(P.n_dup_groups, 64)), dim3(64), 0, s, P, poses, Hblk);
  hipLaunchKernelGGL(k_reduce, dim3(1), dim3(256), 0, s, P.partial, (int64_t)blocks, scalar_out, 0);
}
int linearize_blocks(const DevPlan &P) { return cdiv(P.n_poses * 4, 256) + P.n_hubs; }
void launch_reduce(const double *partial, int64_t n, double *out, int mode, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce, dim3(1), dim3(256), 0, s, partial, n, out, mode);
}

void launch_chi2(const DevPlan &P, const double *poses, double *scalar_out, hipStream_t s) {
  int blocks = cdiv(P.n_edges, 256);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_chi2, dim3(blocks), dim3(256), 0, s, P, poses, P.partial);
  hipLaunchKernelGGL(k_reduce, dim3(1), dim3(256), 0, s, P.partial, (int64_t)blocks, scalar_out, 0);
}

void launch_maxdiag(const DevPlan &P, const double *Hblk, double *scalar_out, hipStream_t s) {
  int blocks = cdiv((int64_t)P.n_real * 6, 256);
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_maxdiag, dim3(blocks), dim3(256), 0, s, Hblk, P.pose_col, (int64_t)P.n_real, P.partial);
  hipLaunchKernelGGL(k_reduce, dim3(1), dim3(256), 0, s, P.partial, (int64_t)blocks, scalar_out, 1);
}

void launch_update(const DevPlan &P, const double *poses, double *cand, const double *x, const double *b,
                   const double *lambda_p, double *scalar_out, hipStream_t s) {
  const int blocks = cdiv(P.n_poses, 256);
  hipLaunchKernelGGL(k_update, dim3(blocks), dim3(256), 0, s, P, poses, cand, x, b, lambda_p, P.partial);
  hipLaunchKernelGGL(k_reduce, dim3(1), dim3(256), 0, s, P.partial, (int64_t)blocks, scalar_out, 0);
}

void launch_copy_vec(const double *src, double *dst, int64_t n, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_copy, dim3((unsigned)std::min<int64_t>(1024, (n + 255) / 256)), dim3(256), 0, s, src, dst, n);
}

void launch_mask_poses(const DevPlan &P, const double *poses, double *out, const int *pose_group, int rank, int world, hipStream_t s) {
  hipLaunchKernelGGL(k_mask_poses, dim3(cdiv(P.n_poses * 8, 256)), dim3(256), 0, s, P.n_poses, poses, out, pose_group, rank, world);
}

}  // namespace fgo
