// Hand-written HIP kernels for gfx950 (MI355X, wave64) -- the block triangular solves on the factor of kernels_factor.hip:
//   k_solve_fwd/bwd                 level-scheduled solves of the generic levels, one workgroup per task
//   k_fwd_ext, k_fwd_tri            stand-alone forward solve of a panel level (the fused one rides in the factor sweep)
//   k_bwd_ext, k_bwd_tri            backward solve of a wide panel level;  k_bwd_fused: of a narrow one, in one launch
//   k_bwd_chain                     the narrow top levels in ONE launch
//   k_wild_decide, k_wild_mark      wildfire back-substitution
// and launch_solve / launch_fwd_level.  The panel kernels read the operand tiles that k_panel_tri* left in ptop (device_plan.hpp).
// Which instantiation a level runs: launch_select.cpp.
//
// Determinism: no floating-point atomics anywhere; partial sums are combined in a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_plan.hpp"
#include "fgo_internal.hpp"
#include "sweep_device.hpp"

namespace fgo {

// ------------------------------------------------------------------------------------------------
// Triangular solves on x (in place, permuted block order).  One workgroup per task, same lane mapping:
// lane group g takes one block of the row/column list, lane r one row (column) of it.
// forward: y_k = L_kk^-1 (b_k - sum_{j in row k} L_kj y_j)
template <int NW>
__global__ __launch_bounds__(NW * 64) void k_solve_fwd(DevPlan P, const double *__restrict__ Lv, double *__restrict__ x,
                                                       int task0) {
  __shared__ double sred[NW * 60];
  const int task = task0 + blockIdx.x;
  if (!task_runs(P, task)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / 6, r = lane - 6 * g;
  const int c_begin = P.task_ptr[task], c_end = P.task_ptr[task + 1];
  for (int ci = c_begin; ci < c_end; ++ci) {
    const int k = P.task_cols[ci];
    const int64_t r0 = (P.dist && k >= P.top_col0) ? P.top_row0[k - P.top_col0] : P.rowptr[k], r1 = P.rowptr[k + 1];
    // wave 0, lanes 0..5 prefetch their row of L_kk and b_k while the sums are formed
    Row6 ld = {{0, 0, 0, 0, 0, 0}};
    double rhs = 0;
    if (threadIdx.x < 6) { ld = load_row(Lv + 36 * P.colptr[k] + 6 * r); rhs = x[6 * (int64_t)k + r]; }
    double acc = 0;
    if (lane < 60)
    {
      // 4 independent (index -> block row, y) chains in flight per lane; fixed summation order
      int64_t e = r0 + wave * 10 + g;
      constexpr int64_t ST = NW * 10;
      for (; e + 3 * ST < r1; e += 4 * ST) {
        const int b0i = P.row_blk[e], b1i = P.row_blk[e + ST], b2i = P.row_blk[e + 2 * ST], b3i = P.row_blk[e + 3 * ST];
        const int c0i = P.row_col[e], c1i = P.row_col[e + ST], c2i = P.row_col[e + 2 * ST], c3i = P.row_col[e + 3 * ST];
        const Row6 l0 = load_row(Lv + 36 * (int64_t)b0i + 6 * r), l1 = load_row(Lv + 36 * (int64_t)b1i + 6 * r);
        const Row6 l2 = load_row(Lv + 36 * (int64_t)b2i + 6 * r), l3 = load_row(Lv + 36 * (int64_t)b3i + 6 * r);
        const Row6 y0 = load_row(x + 6 * (int64_t)c0i), y1 = load_row(x + 6 * (int64_t)c1i);
        const Row6 y2 = load_row(x + 6 * (int64_t)c2i), y3 = load_row(x + 6 * (int64_t)c3i);
        acc += l0.v[0] * y0.v[0] + l0.v[1] * y0.v[1] + l0.v[2] * y0.v[2] + l0.v[3] * y0.v[3] + l0.v[4] * y0.v[4] + l0.v[5] * y0.v[5];
        acc += l1.v[0] * y1.v[0] + l1.v[1] * y1.v[1] + l1.v[2] * y1.v[2] + l1.v[3] * y1.v[3] + l1.v[4] * y1.v[4] + l1.v[5] * y1.v[5];
        acc += l2.v[0] * y2.v[0] + l2.v[1] * y2.v[1] + l2.v[2] * y2.v[2] + l2.v[3] * y2.v[3] + l2.v[4] * y2.v[4] + l2.v[5] * y2.v[5];
        acc += l3.v[0] * y3.v[0] + l3.v[1] * y3.v[1] + l3.v[2] * y3.v[2] + l3.v[3] * y3.v[3] + l3.v[4] * y3.v[4] + l3.v[5] * y3.v[5];
      }
      for (; e < r1; e += ST) {
        const Row6 l = load_row(Lv + 36 * (int64_t)P.row_blk[e] + 6 * r);
        const Row6 y = load_row(x + 6 * (int64_t)P.row_col[e]);
        acc += l.v[0] * y.v[0] + l.v[1] * y.v[1] + l.v[2] * y.v[2] + l.v[3] * y.v[3] + l.v[4] * y.v[4] + l.v[5] * y.v[5];
      }
    }
    if (lane < 60) sred[wave * 60 + lane] = acc;
    __syncthreads();
    if (wave == 0) {                       // whole wave executes the shuffles; lanes 0..5 hold the result
      double s = rhs;
      if (lane < 6)
        for (int q = 0; q < NW * 10; ++q) s -= sred[q * 6 + lane];
      double y = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double yi = __shfl(s, i, WAVE) / __shfl(ld.v[i], i, WAVE);   // y_i = s_i / L_ii
        if (lane == i) y = yi;
        if (lane > i && lane < 6) s -= ld.v[i] * yi;                        // s_r -= L_ri y_i
      }
      if (lane < 6) x[6 * (int64_t)k + lane] = y;
    }
    __syncthreads();
  }
}
// backward: x_k = L_kk^-T (y_k - sum_{i in col k} L_ik^T x_i), tasks' columns in descending order
template <int NW>
__global__ __launch_bounds__(NW * 64) void k_solve_bwd(DevPlan P, const double *__restrict__ Lv, double *__restrict__ x,
                                                       int task0) {
  __shared__ double sred[NW * 60];
  const int task = task0 + blockIdx.x;
  if (!task_runs(P, task)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / 6, cc = lane - 6 * g;
  const int c_begin = P.task_ptr[task], c_end = P.task_ptr[task + 1];
  for (int ci = c_end - 1; ci >= c_begin; --ci) {
    const int k = P.task_cols[ci];
    const int64_t b0 = P.colptr[k] + 1, b1 = P.colptr[k + 1];
    // lanes 0..5 of wave 0 prefetch COLUMN cc of L_kk (row cc of L_kk^T) and y_k
    double lcol[6] = {0, 0, 0, 0, 0, 0};
    double rhs = 0;
    if (threadIdx.x < 6) {
      const double *Ld = Lv + 36 * P.colptr[k];
#pragma unroll
      for (int m = 0; m < 6; ++m) lcol[m] = Ld[m * 6 + cc];
      rhs = x[6 * (int64_t)k + cc];
    }
    double acc = 0;
    if (lane < 60)
      for (int64_t t = b0 + wave * 10 + g; t < b1; t += NW * 10) {
        const double *Lb = Lv + 36 * t + cc;
        const Row6 xi = load_row(x + 6 * (int64_t)P.rowidx[t]);
        acc += Lb[0] * xi.v[0] + Lb[6] * xi.v[1] + Lb[12] * xi.v[2] + Lb[18] * xi.v[3] + Lb[24] * xi.v[4] + Lb[30] * xi.v[5];
      }
    if (lane < 60) sred[wave * 60 + lane] = acc;
    __syncthreads();
    if (wave == 0) {
      double s = rhs;
      if (lane < 6)
        for (int q = 0; q < NW * 10; ++q) s -= sred[q * 6 + lane];
      double y = 0;
#pragma unroll
      for (int i = 5; i >= 0; --i) {
        const double yi = __shfl(s, i, WAVE) / __shfl(lcol[i], i, WAVE);   // x_i = s_i / L_ii
        if (lane == i) y = yi;
        // s_c -= L_ic x_i for c < i ; lane c holds column c of L: L_ic = lcol[i] on lane c
        if (lane < i) s -= lcol[i] * yi;
      }
      if (lane < 6) x[6 * (int64_t)k + lane] = y;
    }
    __syncthreads();
  }
}

// ---- panel solves.  Forward: the external part of every panel column's row list is summed by a wide kernel
// (FWD_CHUNK entries per workgroup, partial sums in a fixed order), then one wave per panel runs the in-panel
// substitution out of LDS.  Backward: same split; the external part runs over the panel's off-triangle rows.
__global__ __launch_bounds__(256) void k_fwd_ext(DevPlan P, const double *__restrict__ Lv, const double *__restrict__ x, int chunk0) {
  __shared__ double sred[240];
  const int ch = chunk0 + blockIdx.x;
  const int k = P.pp.fchunk_col[ch];
  const int64_t e0 = P.pp.fchunk_e0[ch];
  const int64_t rm = P.pp.row_mid[k];
  const int64_t e1 = e0 + FWD_CHUNK < rm ? e0 + FWD_CHUNK : rm;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / 6, r = lane - 6 * g;
  const int gid = wave * 10 + g;
  double acc = 0;
  if (lane < 60) {
    for (int64_t e = e0 + gid; e < e1; e += 160) {
      int bi[4], ci[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t ee = e + 40 * q;
        const bool in = ee < e1;
        bi[q] = in ? P.row_blk[ee] : P.zero_blk;
        ci[q] = in ? P.row_col[ee] : 0;
      }
      Row6 l[4], y[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { l[q] = load_row(Lv + 36 * (int64_t)bi[q] + 6 * r); y[q] = load_row(x + 6 * (int64_t)ci[q]); }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc += l[q].v[0] * y[q].v[0] + l[q].v[1] * y[q].v[1] + l[q].v[2] * y[q].v[2] + l[q].v[3] * y[q].v[3] + l[q].v[4] * y[q].v[4] + l[q].v[5] * y[q].v[5];
    }
    sred[gid * 6 + r] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double s = 0;
    for (int q = 0; q < 40; ++q) s += sred[q * 6 + threadIdx.x];
    P.pp.fpart[6 * (int64_t)ch + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(64) void k_fwd_tri(DevPlan P, double *__restrict__ x, int pn0) {
  // stand-alone forward solve (factor already resident): y_T = T^-1 s from the operand tiles, blocked on the 16x16 tiles:
  // w_J = s_J + sum_{I<J} (-T_JI) y_I, y_J = Dinv_J w_J.  A tile is column-major, so a row of it is a stride-16 walk:
  // lane (p, i) takes columns 4p .. 4p+3 of row i, two xor-shuffles finish the sum.
  __shared__ __attribute__((aligned(16))) double sb[16 * NJMAX], wb[16 * NJMAX], yb[16 * NJMAX];
  const int pn = pn0 + blockIdx.x;
  const PanelDesc d = P.pp.pdesc[pn];
  const int n = 6 * d.m, nJ = (n + 15) >> 4;
  const int *__restrict__ cols = P.task_cols + d.cols0;
  const int lane = threadIdx.x, i = lane & 15, p = lane >> 4;
  const double *__restrict__ tp = P.pp.ptop + (int64_t)d.top * 256;
  for (int c = lane; c < 16 * NJMAX; c += 64) {
    double sv = 0.0;
    if (c < n) {
      const int k = c / 6, cc = c - 6 * k;
      sv = x[6 * (int64_t)cols[k] + cc];
      const int64_t ce = (int64_t)pn * PM + k;
      const int f0 = P.pp.pcol_fchunk0[ce], fn = P.pp.pcol_fchunkn[ce];
      for (int q = 0; q < fn; ++q) sv -= P.pp.fpart[6 * (int64_t)(f0 + q) + cc];
    }
    sb[c] = sv;
  }
  __builtin_amdgcn_wave_barrier();
  for (int J = 0; J < nJ; ++J) {
    double acc = 0.0;
    for (int I = 0; I < J; ++I) {
      const double *__restrict__ t = tp + (J * (J - 1) / 2 + I) * 256 + i;
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += t[16 * (4 * p + u)] * yb[16 * I + 4 * p + u];
    }
    acc += __shfl_xor(acc, 16, WAVE);
    acc += __shfl_xor(acc, 32, WAVE);
    if (p == 0) wb[16 * J + i] = sb[16 * J + i] + acc;
    __builtin_amdgcn_wave_barrier();
    const double *__restrict__ dt = tp + (NLT + J) * 256 + i;
    double a2 = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) a2 += dt[16 * (4 * p + u)] * wb[16 * J + 4 * p + u];
    a2 += __shfl_xor(a2, 16, WAVE);
    a2 += __shfl_xor(a2, 32, WAVE);
    if (p == 0) yb[16 * J + i] = a2;
    __builtin_amdgcn_wave_barrier();
  }
  for (int c = lane; c < n; c += 64) x[6 * (int64_t)cols[c / 6] + (c - 6 * (c / 6))] = yb[c];
}

__global__ __launch_bounds__(64) void k_bwd_ext(DevPlan P, const double *__restrict__ Lv, const double *__restrict__ x, int chunk0) {
  __shared__ double red[PANEL_ROWS * PM * 6];
  const int ch = chunk0 + blockIdx.x;
  const BwdChunk bc = P.pp.bchunks[ch];
  if (P.task_dirty && !P.task_dirty[P.pp.pdesc[bc.pn].task]) return;      // (wildfire back-substitution: panel not re-solved)
  const int m = bc.m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / 6, cc = lane - 6 * g;
  const int gid = wave * 10 + g;
  const bool on = lane < 60 && gid < bc.nrows;
  const int ri = bc.row0 + (on ? gid : 0);
  const int *__restrict__ rb = P.pp.prow_blk + (int64_t)ri * PM;
  Row6 xi = {{0, 0, 0, 0, 0, 0}};
  if (on) xi = load_row(x + 6 * (int64_t)P.pp.prow_idx[ri]);
#pragma unroll
  for (int k = 0; k < PM; ++k) {
    double c = 0;
    if (on && k < m) {
      const int t = rb[k];
      if (t >= 0) {
        const double *Lb = Lv + 36 * (int64_t)t + cc;
        c = Lb[0] * xi.v[0] + Lb[6] * xi.v[1] + Lb[12] * xi.v[2] + Lb[18] * xi.v[3] + Lb[24] * xi.v[4] + Lb[30] * xi.v[5];
      }
    }
    if (lane < 60) red[(gid * PM + k) * 6 + cc] = c;
  }
  __syncthreads();
  for (int q2 = threadIdx.x; q2 < m * 6; q2 += 64) {
    const int k = q2 / 6, c = q2 - 6 * k;
    double s = 0;
    for (int q = 0; q < PANEL_ROWS; ++q) s += red[(q * PM + k) * 6 + c];
    P.pp.bpart[((int64_t)ch * PM + k) * 6 + c] = s;
  }
}

// ---- Shared pieces of the panel backward kernels (k_bwd_tri, k_bwd_fused, k_bwd_chain).
//
// In-panel backward substitution x_T = T^-T s from the panel's operand tiles (k_panel_tri): one wave, blocked on the
// 16x16 tiles.  A tile in operand order is simply column-major (element (i, j) at 16 j + i), so (T_IJ)^T x_I and
// Dinv_J^T w are dot products of contiguous columns: lane (p, j) takes rows 4p .. 4p+3 of column j, two xor-shuffles
// finish the sum.  The tiles of tile column J (those below the diagonal + the inverted diagonal tile) are loaded one
// step ahead of their use.  IMG: the tiles are read from the workgroup's LDS image (bwd_tiles_to_lds) instead of ptop.
constexpr int LT_COL = 18, LT_TILE = 16 * LT_COL;      // LDS image of a tile: columns padded to 18 doubles, so that the 16 lanes of a p read 16 different 16-byte slots
template <bool IMG>
__device__ __forceinline__ void bwd_panel_subst(const double *__restrict__ tp, int nJ, int lane, const double *__restrict__ sb, double *__restrict__ wb,
                                                double *__restrict__ xb) {
  constexpr int TS = IMG ? LT_TILE : 256, CS = IMG ? LT_COL : 16;
  const int j = lane & 15, p = lane >> 4;
  // tile column J: lower tiles (I, J), I = J+1 .. nJ-1, into slots I, the diagonal tile into slot J
  auto load_tile_col = [&](int J, double (&A)[NJMAX][4]) {
#pragma unroll
    for (int I = 0; I < NJMAX; ++I) {
      const bool need = I >= J && I < nJ;                      // wave-uniform
      if (need) {
        const int t = I == J ? NLT + J : I * (I - 1) / 2 + J;
        const double2 lo = *reinterpret_cast<const double2 *>(tp + t * TS + CS * j + 4 * p);
        const double2 hi = *reinterpret_cast<const double2 *>(tp + t * TS + CS * j + 4 * p + 2);
        A[I][0] = lo.x; A[I][1] = lo.y; A[I][2] = hi.x; A[I][3] = hi.y;
      }
    }
  };
  double Abuf[2][NJMAX][4];
#pragma unroll
  for (int J = NJMAX - 1; J >= 0; --J)
    if (J < nJ) {
      double (&A)[NJMAX][4] = Abuf[J & 1];
      if (J == nJ - 1) load_tile_col(J, A);                     // first step: nothing was prefetched (static register indices only)
      if (J > 0) load_tile_col(J - 1, Abuf[(J - 1) & 1]);
      double acc = 0.0;
#pragma unroll
      for (int I = J + 1; I < NJMAX; ++I)
        if (I < nJ) {
#pragma unroll
          for (int u = 0; u < 4; ++u) acc += A[I][u] * xb[16 * I + 4 * p + u];      // strictly-lower tile (I, J), stored negated
        }
      acc += __shfl_xor(acc, 16, WAVE);
      acc += __shfl_xor(acc, 32, WAVE);
      if (p == 0) wb[16 * J + j] = sb[16 * J + j] + acc;
      __builtin_amdgcn_wave_barrier();
      double a2 = 0.0;
#pragma unroll
      for (int u = 0; u < 4; ++u) a2 += A[J][u] * wb[16 * J + 4 * p + u];
      a2 += __shfl_xor(a2, 16, WAVE);
      a2 += __shfl_xor(a2, 32, WAVE);
      if (p == 0) xb[16 * J + j] = a2;
      __builtin_amdgcn_wave_barrier();
    }
}

__global__ __launch_bounds__(64) void k_bwd_tri(DevPlan P, double *__restrict__ x, int pn0) {
  __shared__ __attribute__((aligned(16))) double sb[16 * NJMAX], wb[16 * NJMAX], xb[16 * NJMAX];
  const int pn = pn0 + blockIdx.x;
  const PanelDesc d = P.pp.pdesc[pn];
  if (!task_runs(P, d.task)) return;
  const int n = 6 * d.m, nJ = (n + 15) >> 4;
  const int *__restrict__ cols = P.task_cols + d.cols0;
  const int lane = threadIdx.x;
  const double *__restrict__ tp = P.pp.ptop + (int64_t)d.top * 256;
  for (int c = lane; c < 16 * NJMAX; c += 64) {
    double s = 0.0;
    if (c < n) {
      s = x[6 * (int64_t)cols[c / 6] + (c - 6 * (c / 6))];
      for (int q = 0; q < d.nchunks; ++q) s -= P.pp.bpart[(int64_t)(d.chunk0 + q) * (6 * PM) + c];
    }
    sb[c] = s;
  }
  __builtin_amdgcn_wave_barrier();
  bwd_panel_subst<false>(tp, nJ, lane, sb, wb, xb);
  for (int c = lane; c < n; c += 64) x[6 * (int64_t)cols[c / 6] + (c - 6 * (c / 6))] = xb[c];
}

// ---- The 16-wave backward solve of a panel (k_bwd_fused, k_bwd_chain) in its parts.
constexpr int BWD_NW = 16;
constexpr int BWD_KB = 4;                              // block columns per LDS exchange of the row phase
constexpr int BWD_ROWBUF = BWD_KB * 60;                // a wave's exchange slab [BWD_KB][60]; its first 6 PM doubles hold the wave's totals afterwards
static_assert(PM % BWD_KB == 0 && 6 * BWD_KB <= 64 && 6 * PM <= BWD_ROWBUF && 6 * PM <= 128, "row phase layout");

// What a workgroup can fetch before anything of the levels above is known: a wave's first chunk of rows (x index and block
// ids of one row per lane group) ...
struct BwdFirst { int idx; int tb[PM]; };
__device__ __forceinline__ void bwd_first_chunk(const DevPlan &P, const PanelDesc &d, int wave, int lane, BwdFirst &f) {
  const int g = lane / 6, r0 = 10 * wave;
  const bool on = lane < 60 && r0 + g < d.nrows;
  const int ri = d.prow0 + r0 + (on ? g : 0);
  f.idx = 0;
#pragma unroll
  for (int k = 0; k < PM; ++k) f.tb[k] = -1;
  if (r0 < d.nrows) {
    const int *__restrict__ rb = P.pp.prow_blk + (int64_t)ri * PM;
    if (on) f.idx = P.pp.prow_idx[ri];
#pragma unroll
    for (int k = 0; k < PM; ++k) f.tb[k] = (on && k < d.m) ? rb[k] : -1;
  }
}
// ... the panel's operand tiles (final once the factor sweep is over), by all threads into the LDS image: the loads are
// issued together, the LDS writes follow where the caller has other work in between ...
constexpr int BWD_TILE_REGS = (NTILE * 128 + BWD_NW * 64 - 1) / (BWD_NW * 64);
struct BwdTiles { double2 v[BWD_TILE_REGS]; };
__device__ __forceinline__ bool bwd_tile_needed(int e, int nJ) {
  const int t = e >> 7;                                      // double2 e & 127 of tile slot t
  return e < NTILE * 128 && (t < nJ * (nJ - 1) / 2 || (t >= NLT && t < NLT + nJ));
}
__device__ __forceinline__ void bwd_tiles_load(const double *__restrict__ tp, int nJ, BwdTiles &r) {
#pragma unroll
  for (int q = 0; q < BWD_TILE_REGS; ++q) {
    const int e = (int)threadIdx.x + q * BWD_NW * 64;
    r.v[q] = double2{0.0, 0.0};
    if (bwd_tile_needed(e, nJ)) r.v[q] = *reinterpret_cast<const double2 *>(tp + 2 * e);
  }
}
__device__ __forceinline__ void bwd_tiles_to_lds(const BwdTiles &r, int nJ, double *__restrict__ img) {
#pragma unroll
  for (int q = 0; q < BWD_TILE_REGS; ++q) {
    const int e = (int)threadIdx.x + q * BWD_NW * 64, t = e >> 7, w = e & 127;      // column w >> 3, rows 2 (w & 7), 2 (w & 7) + 1
    if (bwd_tile_needed(e, nJ)) *reinterpret_cast<double2 *>(img + t * LT_TILE + LT_COL * (w >> 3) + 2 * (w & 7)) = r.v[q];
  }
}
// ... and the panel's own right-hand side: its y of the forward solve, which no other panel writes (lane l of wave 0
// keeps entries l and l + 64 and their offsets in x).
struct BwdOwn { int64_t off[2]; double y[2]; };
__device__ __forceinline__ void bwd_own_rhs(const int *__restrict__ cols, int n, int lane, const double *__restrict__ x, BwdOwn &o) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    o.off[h] = 0; o.y[h] = 0.0;
    if (c < n) {
      o.off[h] = 6 * (int64_t)cols[c / 6] + (c - 6 * (c / 6));
      o.y[h] = x[o.off[h]];
    }
  }
}

// one lane's term of s_k -= L_ik^T x_i: column cc of block t against the lane group's row of x
__device__ __forceinline__ double bwd_row_term(const double *__restrict__ Lv, int t, int cc, const Row6 &xi) {
  double c = 0.0;
  if (t >= 0) {
    const double *Lb = Lv + 36 * (int64_t)t + cc;
    c = Lb[0] * xi.v[0] + Lb[6] * xi.v[1] + Lb[12] * xi.v[2] + Lb[18] * xi.v[3] + Lb[24] * xi.v[4] + Lb[30] * xi.v[5];
  }
  return c;
}

// Row phase: wave w takes the panel's off-triangle rows in chunks of 10 (one row per lane group), chunks w, w + 16, ...
// The ten lane groups' terms of BWD_KB block columns go through the wave's slab in ONE exchange: lane 6 k' + cc sums the ten
// values of column k' of the batch (q = 0 .. 9 from 0.0, the order of the one-column-per-exchange form) and keeps the wave's
// running total of that column over the chunks.  On return buf[6 k + cc] holds the wave's total of block column k, entry cc.
// agent_x: agent-scope loads of x instead of an acquire fence (k_bwd_chain, mode bit 1).
__device__ __forceinline__ void bwd_rows(const DevPlan &P, const PanelDesc &d, const double *__restrict__ Lv, const double *x, const BwdFirst &f,
                                         bool agent_x, int wave, int lane, double *__restrict__ buf) {
  const int m = d.m;
  const int g = lane / 6, cc = lane - 6 * g;
  double tot[PM / BWD_KB];
#pragma unroll
  for (int b = 0; b < PM / BWD_KB; ++b) tot[b] = 0.0;
  for (int r0 = 10 * wave; r0 < d.nrows; r0 += 10 * BWD_NW) {
    const bool first = r0 == 10 * wave;
    const bool on = lane < 60 && r0 + g < d.nrows;
    const int ri = d.prow0 + r0 + (on ? g : 0);
    const int *__restrict__ rb = P.pp.prow_blk + (int64_t)ri * PM;
    Row6 xi = {{0, 0, 0, 0, 0, 0}};
    if (on) {
      const double *xp = x + 6 * (int64_t)(first ? f.idx : P.pp.prow_idx[ri]);
      if (agent_x) {
#pragma unroll
        for (int c = 0; c < 6; ++c) xi.v[c] = __hip_atomic_load(xp + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else xi = load_row(xp);
    }
    int tb[PM];
#pragma unroll
    for (int k = 0; k < PM; ++k) tb[k] = first ? f.tb[k] : ((on && k < m) ? rb[k] : -1);
#pragma unroll
    for (int k0 = 0; k0 < PM; k0 += BWD_KB)
      if (k0 < m) {                                          // wave-uniform
        double c[BWD_KB];
#pragma unroll
        for (int u = 0; u < BWD_KB; ++u) c[u] = bwd_row_term(Lv, tb[k0 + u], cc, xi);      // (columns >= m: block id -1, 0.0)
        if (lane < 60) {
#pragma unroll
          for (int u = 0; u < BWD_KB; ++u) buf[60 * u + lane] = c[u];
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < 6 * BWD_KB && k0 + g < m) {               // lane 6 k' + cc: g == k'
          double sacc = 0.0;
#pragma unroll
          for (int q = 0; q < 10; ++q) sacc += buf[60 * g + 6 * q + cc];
          tot[k0 / BWD_KB] += sacc;
        }
        __builtin_amdgcn_wave_barrier();
      }
  }
  if (lane < 6 * BWD_KB) {
#pragma unroll
    for (int b = 0; b < PM / BWD_KB; ++b) if (BWD_KB * b + g < m) buf[6 * BWD_KB * b + lane] = tot[b];
  }
}

// wave 0, after the workgroup barrier behind bwd_rows: s = own y minus the waves' totals in the order of the waves, then
// the substitution from the LDS image of the tiles.  Leaves x_T in xb.
__device__ __forceinline__ void bwd_finish(const double *__restrict__ rowbuf, const double *__restrict__ img, int n, int nJ, int lane, const BwdOwn &o,
                                           double *__restrict__ sb, double *__restrict__ wb, double *__restrict__ xb) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    if (c < 16 * NJMAX) {
      double s = 0.0;
      if (c < n) {
        s = o.y[h];
        for (int w = 0; w < BWD_NW; ++w) s -= rowbuf[w * BWD_ROWBUF + c];
      }
      sb[c] = s;
    }
  }
  __builtin_amdgcn_wave_barrier();
  bwd_panel_subst<true>(img, nJ, lane, sb, wb, xb);
}

// Backward solve of a panel in ONE kernel, for levels with few panels (the top of the tree): everything that depends on the
// structure and the factor alone -- the waves' first chunks of row indices, the panel's own right-hand side, all of its
// operand tiles (into LDS) -- is requested first, so it is in flight while x of the rows arrives.  Then the 16 waves take
// the off-triangle rows (bwd_rows), keep their partial sums s_k -= L_ik^T x_i in registers across chunks, combine them
// through LDS in a fixed order (chunks of a wave, then waves 0 .. 15), and wave 0 finishes with the in-panel substitution
// x_T = T^-T s (bwd_finish), the arithmetic of k_bwd_tri.  One launch and no round trip of the partial sums through memory
// instead of two launches per level.  80 KB of LDS: two workgroups per CU.
__global__ __launch_bounds__(BWD_NW * 64) void k_bwd_fused(DevPlan P, const double *__restrict__ Lv, double *__restrict__ x, int pn0) {
  __shared__ __attribute__((aligned(16))) double rowbuf[BWD_NW * BWD_ROWBUF];
  __shared__ __attribute__((aligned(16))) double img[NTILE * LT_TILE];
  __shared__ __attribute__((aligned(16))) double sb[16 * NJMAX], wb[16 * NJMAX], xb[16 * NJMAX];
  const int pn = pn0 + blockIdx.x;
  const PanelDesc d = P.pp.pdesc[pn];
  if (!task_runs(P, d.task)) return;                       // (the wildfire mask: launch_solve passes task_dirty = run, k_wild_mark restores x of a task left out)
  const int n = 6 * d.m, nJ = (n + 15) >> 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int *__restrict__ cols = P.task_cols + d.cols0;
  BwdFirst f;
  bwd_first_chunk(P, d, wave, lane, f);
  BwdOwn own = {{0, 0}, {0.0, 0.0}};
  if (wave == 0) bwd_own_rhs(cols, n, lane, x, own);
  BwdTiles tiles;
  bwd_tiles_load(P.pp.ptop + (int64_t)d.top * 256, nJ, tiles);
  bwd_rows(P, d, Lv, x, f, false, wave, lane, rowbuf + wave * BWD_ROWBUF);
  bwd_tiles_to_lds(tiles, nJ, img);
  __syncthreads();
  if (wave > 0) return;
  bwd_finish(rowbuf, img, n, nJ, lane, own, sb, wb, xb);
#pragma unroll
  for (int h = 0; h < 2; ++h) if (lane + 64 * h < n) x[own.off[h]] = xb[lane + 64 * h];
}

// ---- Backward solve of the TOP LEVELS in one launch.  The ~24 narrow levels of cfg 2 cost ~19 us each as k_bwd_fused launches:
// ~4 us of launch floor, the descriptor / index / tile round trips, then the dependent part.  Here every panel of those levels
// is a workgroup of ONE launch, ordered root level first; a workgroup does everything that does not depend on x of the levels
// above (descriptors, its first chunks of row indices, its own right-hand side, all of its operand tiles into LDS) and then
// waits until the `need` panels above it have published their part of x (one counter, release / acquire at agent scope --
// the decoupled look-back idiom).  Behind the wait only x of the ancestors and the L blocks of the rows are loaded.
// Workgroups are dispatched in index order and wait only for smaller indices, so the launch cannot deadlock whatever the
// residency: that holds for any LDS footprint, since a workgroup that is not resident yet is never waited for by a resident
// one (at 80 KB of LDS one or two workgroups share a CU; with more items than slots the later items start as the earlier ones
// retire and merely lose their head start).  Same arithmetic, same order of operations as k_bwd_fused: bit-identical x.
__global__ __launch_bounds__(BWD_NW * 64) void k_bwd_chain(DevPlan P, const double *__restrict__ Lv, double *__restrict__ x, int n_items, int mode) {
  const ChainItem it = P.pp.bchain[blockIdx.x];
  __shared__ __attribute__((aligned(16))) double rowbuf[BWD_NW * BWD_ROWBUF];
  __shared__ __attribute__((aligned(16))) double img[NTILE * LT_TILE];
  __shared__ __attribute__((aligned(16))) double sb[16 * NJMAX], wb[16 * NJMAX], xb[16 * NJMAX];
  const PanelDesc d = P.pp.pdesc[it.pn];
  const int n = 6 * d.m, nJ = (n + 15) >> 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int *__restrict__ cols = P.task_cols + d.cols0;
  unsigned *__restrict__ done = P.pp.bchain_done;
  BwdFirst f;
  bwd_first_chunk(P, d, wave, lane, f);
  BwdOwn own = {{0, 0}, {0.0, 0.0}};
  if (wave == 0) bwd_own_rhs(cols, n, lane, x, own);
  BwdTiles tiles;
  bwd_tiles_load(P.pp.ptop + (int64_t)d.top * 256, nJ, tiles);
  if (mode & 4) {                                            // pull the L blocks of the first chunks towards this XCD's L2 while the levels above run
    const int cc = lane - 6 * (lane / 6);
    double warm = 0.0;
#pragma unroll
    for (int k = 0; k < PM; ++k) if (f.tb[k] >= 0) warm += Lv[36 * (int64_t)f.tb[k] + cc];
    if (warm == 123.456e300) sb[0] = warm;
  }
  bwd_tiles_to_lds(tiles, nJ, img);
  // ---- wait for the levels above
  if (it.need > 0) {
    if (threadIdx.x == 0) {
      while (__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)it.need) __builtin_amdgcn_s_sleep(2);
    }
    __syncthreads();
    if (!(mode & 1)) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  bwd_rows(P, d, Lv, x, f, (mode & 1) != 0, wave, lane, rowbuf + wave * BWD_ROWBUF);
  __syncthreads();
  if (wave > 0) return;
  bwd_finish(rowbuf, img, n, nJ, lane, own, sb, wb, xb);
  if (mode & 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) if (lane + 64 * h < n) __hip_atomic_store(x + own.off[h], xb[lane + 64 * h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");            // (the stores are acknowledged before the counter moves)
  } else {
#pragma unroll
    for (int h = 0; h < 2; ++h) if (lane + 64 * h < n) x[own.off[h]] = xb[lane + 64 * h];
    // ---- publish: this panel's part of x is visible at agent scope before the counter moves; the last panel re-arms the counter
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  }
  if (lane == 0) {
    const unsigned prev = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev + 1 == (unsigned)n_items) __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- wildfire back-substitution (ISAM2 option, fgo_isam2_set_wildfire): below the backward chain a task is solved again only
// if it was re-factored or an x it reads changed by >= thr against the previous update's solution; the others keep that solution.
// decide: one wave per task of a level -> run[task];  mark: after the level, changed[column] for its columns (and the old
// solution back into x where the task was not run: x held the forward solution there).
__global__ __launch_bounds__(64) void k_wild_decide(DevPlan P, const unsigned char *__restrict__ dirty, const unsigned char *__restrict__ chg,
                                                    unsigned char *__restrict__ run, int task0, int is_panel) {
  const int task = task0 + blockIdx.x;
  const int lane = threadIdx.x;
  bool any = dirty[task] != 0;
  if (!any) {
    if (is_panel) {
      const PanelDesc d = P.pp.pdesc[P.pp.task_panel[task]];
      for (int q = lane; q < d.nrows && !any; q += 64) any = chg[P.pp.prow_idx[d.prow0 + q]] != 0;
    } else {
      const int c0 = P.task_ptr[task], c1 = P.task_ptr[task + 1];
      const int k_last = P.task_cols[c1 - 1];
      for (int ci = c0; ci < c1; ++ci) {
        const int k = P.task_cols[ci];
        for (int64_t b = P.colptr[k] + 1 + lane; b < P.colptr[k + 1] && !any; b += 64) { const int i = P.rowidx[b]; any = i > k_last && chg[i] != 0; }
      }
    }
  }
  any = __any(any);
  if (lane == 0) run[task] = any;
}
__global__ __launch_bounds__(64) void k_wild_mark(DevPlan P, double *__restrict__ x, const double *__restrict__ xprev, const unsigned char *__restrict__ run,
                                                  unsigned char *__restrict__ chg, double thr, int task0, const ChainItem *__restrict__ items) {
  // items != nullptr: the panels of the backward chain (always solved), blockIdx -> item; else task0 + blockIdx
  const int task = items ? P.pp.pdesc[items[blockIdx.x].pn].task : task0 + blockIdx.x;
  const bool ran = !run || run[task];
  const int c0 = P.task_ptr[task], c1 = P.task_ptr[task + 1];
  for (int ci = c0 + (int)threadIdx.x; ci < c1; ci += 64) {       // one column per lane
    const int k = P.task_cols[ci];
    bool big = false;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      const double xo = xprev[6 * (int64_t)k + e];
      if (ran) big |= fabs(x[6 * (int64_t)k + e] - xo) >= thr;
      else x[6 * (int64_t)k + e] = xo;
    }
    chg[k] = big;
  }
}

void launch_fwd_level(const DevPlan &P, const HostSchedule &H, const double *Lv, double *x, int l, hipStream_t s, LaunchCensus *cz) {
  const int t0 = H.level_ptr[l], nt = H.level_ptr[l + 1] - t0;
  switch (select_fwd(H, l)) {
    case LF_FWD1: FGO_LAUNCH(cz, LF_FWD1, nt, k_solve_fwd<1>, dim3(nt), dim3(64), 0, s, P, Lv, x, t0); break;
    case LF_FWD4: FGO_LAUNCH(cz, LF_FWD4, nt, k_solve_fwd<4>, dim3(nt), dim3(256), 0, s, P, Lv, x, t0); break;
    default: FGO_LAUNCH(cz, LF_FWD16, nt, k_solve_fwd<16>, dim3(nt), dim3(1024), 0, s, P, Lv, x, t0); break;
  }
}

// fwd_done: x already holds y (forward solve fused into launch_factor); only the backward sweep runs
void launch_solve(const DevPlan &P, const HostSchedule &H, const double *Lv, const double *b, double *x, hipStream_t s, bool fwd_done, int phase,
                  const Wildfire *wf, LaunchCensus *cz) {
  if (!fwd_done) {                                            // stand-alone forward solve: single-GPU entry points only
    if (!cz) launch_copy_vec(b, x, (int64_t)P.nb * 6, s);
    for (int l = 0; l < H.n_levels; ++l) {
      if (!seg_runs(H, l, PHASE_ALL)) continue;
      const int t0 = H.level_ptr[l], nt = H.level_ptr[l + 1] - t0;
      if (H.level_panel[l]) {
        const int c0 = H.fchunk_ptr[l], nc = H.fchunk_ptr[l + 1] - c0;
        if (nc > 0) FGO_LAUNCH(cz, LF_FWD_EXT, nc, k_fwd_ext, dim3(nc), dim3(256), 0, s, P, Lv, x, c0);
        FGO_LAUNCH(cz, LF_FWD_TRI, nt, k_fwd_tri, dim3(nt), dim3(64), 0, s, P, x, H.level_pn0[l]);
        continue;
      }
      launch_fwd_level(P, H, Lv, x, l, s, cz);
    }
  }
  // backward sweep.  Distributed: the top first (replicated on every rank), then this rank's own domain -- a domain
  // column needs x of its ancestors only (top + own domain), so no communication
  // (distributed: the chain is the replicated top's, part of the PHASE_TOP pass)
  const bool chain = (phase == PHASE_ALL || phase == PHASE_TOP) && H.bchain_low >= 0 && H.bchain_n > 0;
  static const int chain_mode = (int)tune("bwd_chain_mode", 5);   // 1: agent-scope loads of x instead of an acquire fence (no L2 invalidation), 2: agent-scope stores + store-acknowledge wait instead of the release fence, 4: the L blocks of the first row chunks touched before the wait (the operand tiles are always brought on chip there).  cfg 2 backward sweep: no chain 0.799, modes 0 / 1 / 3 / 7: 0.815 / 0.747 / 0.737 / 0.735 ms
  if (cz) { cz->chain_on = chain ? 1 : 0; cz->chain_mode = chain_mode; }
  if (chain) {
    // the progress counter starts every launch at zero whatever happened to the launch before (an aborted launch would leave
    // it armed and let every later wait pass early): a 4-byte kernel node in front, part of the captured trial
    if (!cz) launch_zero_flag(reinterpret_cast<int *>(P.pp.bchain_done), s);
    FGO_LAUNCH(cz, LF_BWD_CHAIN, H.bchain_n, k_bwd_chain, dim3(H.bchain_n), dim3(BWD_NW * 64), 0, s, P, Lv, x, H.bchain_n, chain_mode);      // (items: root level first)
  }
  const bool wild = wf && chain && phase == PHASE_ALL && !cz;       // (the chain's levels are always solved: they are the dirty root paths)
  DevPlan Pw = P;
  if (wild) {
    Pw.task_dirty = wf->run;
    hipLaunchKernelGGL(k_wild_mark, dim3(H.bchain_n), dim3(64), 0, s, P, x, wf->xprev, (const unsigned char *)nullptr, wf->chg, wf->thr, 0, P.pp.bchain);
  }
  const DevPlan &PL = wild ? Pw : P;
  for (int pass = 0; pass < (phase == PHASE_ALL ? 1 : 2); ++pass)
  for (int l = H.n_levels - 1; l >= 0; --l) {
    if (!seg_runs(H, l, phase == PHASE_ALL ? PHASE_ALL : (pass == 0 ? PHASE_TOP : PHASE_DOMAIN))) continue;
    if (chain && l >= H.bchain_low && (!P.dist || H.seg_group[l] == H.world)) continue;      // solved by the chain launch
    const int t0 = H.level_ptr[l], nt = H.level_ptr[l + 1] - t0;
    // wildfire: which tasks of the level are solved again -- before its kernels; afterwards which of its columns moved
    auto level_done = [&]() { if (wild) hipLaunchKernelGGL(k_wild_mark, dim3(nt), dim3(64), 0, s, P, x, wf->xprev, wf->run, wf->chg, wf->thr, t0, (const ChainItem *)nullptr); };
    if (wild) hipLaunchKernelGGL(k_wild_decide, dim3(nt), dim3(64), 0, s, P, wf->dirty, wf->chg, wf->run, t0, H.level_panel[l] ? 1 : 0);
    switch (select_bwd(H, l)) {
      case LF_BWD_FUSED: FGO_LAUNCH(cz, LF_BWD_FUSED, nt, k_bwd_fused, dim3(nt), dim3(BWD_NW * 64), 0, s, PL, Lv, x, H.level_pn0[l]); break;
      case LF_BWD_EXT: {
        const int c0 = H.pchunk_ptr[l], nc = H.pchunk_ptr[l + 1] - c0;
        if (nc > 0) FGO_LAUNCH(cz, LF_BWD_EXT, nc, k_bwd_ext, dim3(nc), dim3(64), 0, s, PL, Lv, x, c0);
        FGO_LAUNCH(cz, LF_BWD_TRI, nt, k_bwd_tri, dim3(nt), dim3(64), 0, s, PL, x, H.level_pn0[l]);
        break;
      }
      case LF_BWD1: FGO_LAUNCH(cz, LF_BWD1, nt, k_solve_bwd<1>, dim3(nt), dim3(64), 0, s, PL, Lv, x, t0); break;
      case LF_BWD4: FGO_LAUNCH(cz, LF_BWD4, nt, k_solve_bwd<4>, dim3(nt), dim3(256), 0, s, PL, Lv, x, t0); break;
      default: FGO_LAUNCH(cz, LF_BWD8, nt, k_solve_bwd<8>, dim3(nt), dim3(512), 0, s, PL, Lv, x, t0); break;
    }
    level_done();
  }
}

}  // namespace fgo
