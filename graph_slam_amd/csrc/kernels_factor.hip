// Hand-written HIP kernels for gfx950 (MI355X, wave64) -- the factor sweep (block-sparse left-looking Cholesky, 6x6 f64 micro-blocks):
//   k_chol_acc       external updates of a level's columns, gather form; k_chol_acc2: the column-group form; both carry the external
//                    part of the fused forward solve (fwd_role, k_fwd_combine)
//   k_chol_fact      the generic one-workgroup-per-task level kernel
//   k_chol_leaf      light sub-trees of the elimination tree factored (and forward-solved) inside LDS   (HOT LOOP 3)
//   k_panel_tri/rows dense part of a panel (<= 16 columns of the skinny top of the tree) on f64 MFMA tiles; they leave the operand tiles
//                    (device_plan.hpp "ptop") that the panel solves of kernels_solve.hip read
//   k_dist_acc/rhs   multi-GPU: a rank's contribution to the top of the factor
// and launch_factor, which walks the levels.  Which instantiation a level runs: launch_select.cpp.
//
// Determinism: no floating-point atomics anywhere.  Cholesky targets are owned by one wave; partial sums are combined in a fixed order.
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>
#include <stdint.h>
#include "device_plan.hpp"
#include "fgo_internal.hpp"
#include "sweep_device.hpp"

namespace fgo {

typedef double d4_t __attribute__((ext_vector_type(4)));

// acc -= Arow * B^T, B a full 6x6 block in memory
__device__ __forceinline__ void row_update(Row6 &acc, const Row6 &a, const double *__restrict__ B) {
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const Row6 b = load_row(B + 6 * c);
    acc.v[c] -= a.v[0] * b.v[0] + a.v[1] * b.v[1] + a.v[2] * b.v[2] + a.v[3] * b.v[3] + a.v[4] * b.v[4] + a.v[5] * b.v[5];
  }
}
// row r of the H block feeding target t (+ lambda on the diagonal of a diagonal block), or zeros (fill-in)
__device__ __forceinline__ Row6 load_A_row(const DevPlan &P, const double *__restrict__ Hblk, int64_t t, int r, double lambda) {
  const int a = P.asrc[t];
  Row6 x = {{0, 0, 0, 0, 0, 0}};
  if (a >= 0) {
    x = load_row(Hblk + 36 * (int64_t)a + 6 * r);
    if (a < P.nb) {                                   // setLambda: H_pp diagonal += lambda
#pragma unroll
      for (int c = 0; c < 6; ++c) x.v[c] += (c == r) ? lambda : 0.0;   // static indexing keeps x in VGPRs
    }
  }
  return x;
}
// where an accumulate target's value starts (AccDesc::a): row r of H block a (+ lambda on the diagonal of a diagonal block), zeros, or its value in L
__device__ __forceinline__ Row6 acc_start_row(const DevPlan &P, const double *__restrict__ Hblk, const double *__restrict__ Lv, const AccDesc &d, int r, double lambda) {
  Row6 x = {{0, 0, 0, 0, 0, 0}};
  if (d.a == -2) x = load_row(Lv + 36 * (int64_t)d.t + 6 * r);
  else if (d.a >= 0) {
    x = load_row(Hblk + 36 * (int64_t)d.a + 6 * r);
    if (d.a < P.nb) {
#pragma unroll
      for (int c = 0; c < 6; ++c) x.v[c] += (c == r) ? lambda : 0.0;
    }
  }
  return x;
}
// Apply ops [o0, o1) with stride `step` to this lane's row, in wave-uniform batches of OPB ops.
// Memory-level parallelism is the point: per batch every lane first issues the index loads of the NEXT batch,
// then 6*OPB independent 16-byte loads (its row of each L_a and ONE row of each L_b); the other five rows of
// L_b come from the five sibling lanes through a wave-private LDS tile (in-order DS pipe, no barrier).
// Lanes that ran out of ops (or idle lanes) read the all-zero block P.zero_blk, which changes nothing.
constexpr int OPB = 2;
__device__ __forceinline__ void apply_ops(const DevPlan &P, const double *__restrict__ Lv, Row6 &acc, int g, int r,
                                          int64_t o0, int64_t o1, int step, double *__restrict__ tile) {
  int64_t o = o0;
  int ia[OPB], ib[OPB];
#pragma unroll
  for (int k = 0; k < OPB; ++k) {
    const int64_t q = o + (int64_t)k * step;
    const bool in = q < o1;
    ia[k] = in ? P.op_a[q] : P.zero_blk;
    ib[k] = in ? P.op_b[q] : P.zero_blk;
  }
  double *mine = tile + 36 * g;
  while (__any(o < o1)) {
    o += (int64_t)OPB * step;
    int na[OPB], nb2[OPB];
#pragma unroll
    for (int k = 0; k < OPB; ++k) {            // next batch's indices first: they complete before the rows below
      const int64_t q = o + (int64_t)k * step;
      const bool in = q < o1;
      na[k] = in ? P.op_a[q] : P.zero_blk;
      nb2[k] = in ? P.op_b[q] : P.zero_blk;
    }
    Row6 a[OPB], b[OPB];
#pragma unroll
    for (int k = 0; k < OPB; ++k) {
      a[k] = load_row(Lv + 36 * (int64_t)ia[k] + 6 * r);
      b[k] = load_row(Lv + 36 * (int64_t)ib[k] + 6 * r);
    }
#pragma unroll
    for (int k = 0; k < OPB; ++k) {
      store_row(mine + 6 * r, b[k]);
      __builtin_amdgcn_wave_barrier();
      row_update(acc, a[k], mine);
      __builtin_amdgcn_wave_barrier();
      ia[k] = na[k]; ib[k] = nb2[k];
    }
  }
}

// Workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  Neighbouring work items (targets of one
// column, row chunks of one panel) read the same source blocks / operand tiles, so work item ids are assigned such
// that every XCD gets a CONTIGUOUS range of them: the shared blocks then hit in that XCD's L2 instead of being
// fetched once per XCD (rocprofv3 FETCH_SIZE of the accumulate kernel: profiles/).
__device__ __forceinline__ int xcd_contiguous(int b, int n) {
  const int q = n >> 3, r = n & 7, x = b & 7;
  return x * q + (x < r ? x : r) + (b >> 3);
}

// The right-hand side as one more row of the matrix: external part of the forward solve of a panel column,
// x_k <- b_k - sum_{j outside the panel} L_kj y_j, by the forward-solve workgroups of the accumulate launches (NW waves,
// fixed summation order).  Work item w of the level (DevPlan::fwg_*) is either a whole panel column (chunk < 0) or ONE CHUNK
// of FWD_CHUNK entries of a long row -- a hub column's row holds tens of thousands of entries (cfg 4: 54 k = 15 MB for one
// workgroup, 630 us); its chunks are summed by separate workgroups into fpart, and k_fwd_combine -- one more launch, only at
// levels that have such rows -- subtracts them from x in chunk order.  (Doing that inside this launch by "the last workgroup to
// arrive" was tried: the agent-scope fences it needs write back the XCD's L2 while the accumulate workgroups are filling it
// with dirty blocks -- 100 us for 340 chunk workgroups.)  One code path for both forms (the chunked one must not cost the
// accumulate kernels registers: k_chol_acc2<1> runs 7 waves per SIMD).
template <int NW>
__device__ __forceinline__ void fwd_role(const DevPlan &P, const double *__restrict__ Lv, double *__restrict__ x, int base, int off, double *__restrict__ sred) {
  // base >= 0: a level without split rows -- item `off` is entry base + off of task_cols (no table look-up on the launch's
  // critical path); base < 0: items -1 - base + off of the work-item table
  const int ci = base >= 0 ? base + off : P.fwg_ci[-1 - base + off], ch = base >= 0 ? -1 : P.fwg_ch[-1 - base + off];
  if (P.task_dirty && !P.task_dirty[P.tcol_task[ci]]) return;
  const int k = P.task_cols[ci];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / 6, r = lane - 6 * g;
  const int gid = wave * 10 + g;
  constexpr int ST = NW * 10;
  const int64_t rm = P.pp.row_mid[k];
  // whole row: from its first external entry (top: the domain part arrived by all-reduce); chunk: its FWD_CHUNK entries
  const int64_t e0 = ch >= 0 ? P.pp.fchunk_e0[ch] : ((P.dist && k >= P.top_col0) ? P.top_row0[k - P.top_col0] : P.rowptr[k]);
  const int64_t e1 = (ch >= 0 && e0 + FWD_CHUNK < rm) ? e0 + FWD_CHUNK : rm;
  double acc = 0;
  if (lane < 60) {
    for (int64_t e = e0 + gid; e < e1; e += 4 * ST) {
      int bi[4], cj[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t ee = e + ST * q;
        const bool in = ee < e1;
        bi[q] = in ? P.row_blk[ee] : P.zero_blk;
        cj[q] = in ? P.row_col[ee] : 0;
      }
      Row6 l[4], y[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) { l[q] = load_row(Lv + 36 * (int64_t)bi[q] + 6 * r); y[q] = load_row(x + 6 * (int64_t)cj[q]); }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc += l[q].v[0] * y[q].v[0] + l[q].v[1] * y[q].v[1] + l[q].v[2] * y[q].v[2] + l[q].v[3] * y[q].v[3] + l[q].v[4] * y[q].v[4] + l[q].v[5] * y[q].v[5];
    }
    sred[gid * 6 + r] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double sv = ch >= 0 ? 0.0 : x[6 * (int64_t)k + threadIdx.x];
    for (int q = 0; q < ST; ++q) sv -= sred[q * 6 + threadIdx.x];
    if (ch >= 0) P.pp.fpart[6 * (int64_t)ch + threadIdx.x] = -sv; else x[6 * (int64_t)k + threadIdx.x] = sv;
  }
}

// x_k -= the chunk sums of a split row, in chunk order (one wave per split column; launched between the accumulate and the
// triangle launch of a level that has such rows).  The partial sums are fetched by the whole wave, then subtracted one
// after the other: the order is fixed.
__global__ __launch_bounds__(64) void k_fwd_combine(DevPlan P, double *__restrict__ x, int s0) {
  __shared__ double buf[360];
  const int ci = P.fsplit_ci[s0 + blockIdx.x];
  if (P.task_dirty && !P.task_dirty[P.tcol_task[ci]]) return;
  const int k = P.task_cols[ci], f0 = P.fwd_f0[ci], fn = P.fwd_fn[ci];
  double sv = threadIdx.x < 6 ? x[6 * (int64_t)k + threadIdx.x] : 0.0;
  for (int q0 = 0; q0 < fn; q0 += 60) {
    const int nq = fn - q0 < 60 ? fn - q0 : 60;
    __syncthreads();
    for (int i = threadIdx.x; i < 6 * nq; i += 64) buf[i] = P.pp.fpart[6 * (int64_t)(f0 + q0) + i];
    __syncthreads();
    if (threadIdx.x < 6) for (int q = 0; q < nq; ++q) sv -= buf[6 * q + threadIdx.x];
  }
  if (threadIdx.x < 6) x[6 * (int64_t)k + threadIdx.x] = sv;
}

// wide accumulate: external sources only.  One workgroup (4 waves) per 10 target blocks; the 4 waves
// split each target's source list (split-K) and wave 0 combines the partial rows from LDS in a fixed order.
// Workgroups beyond n_acc_wg (panel levels with a fused forward solve) take one panel column of the right-hand
// side each: same dependencies as the accumulation, so it rides in the same launch.
template <int SPLIT>
__global__ __launch_bounds__(SPLIT * 64) void k_chol_acc(DevPlan P, const double *__restrict__ Hblk, double *__restrict__ Lv,
                                                         int64_t first, int64_t count, const double *__restrict__ lambda_p,
                                                         double *__restrict__ x, int n_acc_wg, int col0, int n_long, int64_t long0) {
  __shared__ __attribute__((aligned(16))) double tile[SPLIT][360];
  __shared__ __attribute__((aligned(16))) double part[SPLIT][60][6];
  if ((int)blockIdx.x >= n_acc_wg + n_long) {
    fwd_role<SPLIT>(P, Lv, x, col0, (int)blockIdx.x - n_acc_wg - n_long, &part[0][0][0]);      // col0: first forward work item of the level (fwd_role)
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / 6, r = lane - 6 * g;
  if ((int)blockIdx.x >= n_acc_wg) {
    // a target with a long source list (hub column, top separator): all SPLIT*10 lane groups of the workgroup stride
    // through ITS list, then the partial blocks are summed in a fixed order
    // (n_acc_wg is a multiple of 8 when there are long targets, so the XCD of this workgroup is (blockIdx - n_acc_wg) & 7:
    //  every XCD takes a CONTIGUOUS range of the long targets -- the targets of a column / panel share their sources)
    const int64_t ti = long0 + xcd_contiguous((int)blockIdx.x - n_acc_wg, n_long);      // (long0 = first + count in a full sweep)
    if (P.task_dirty && !P.task_dirty[P.acc_task[ti]]) return;
    // (AccDesc, structure_upload.cpp: riders have applied the head of the list -> continue from the value in L, or, for a hub target, from H: its
    //  riders left their sums in scratch blocks that the rest of the list subtracts; a top block's value (incl. the domains' updates) sits in L)
    const AccDesc dsc = P.acc_desc[ti];
    const int64_t t = dsc.t;
    const int gid = wave * 10 + g;
    Row6 acc = {{0, 0, 0, 0, 0, 0}};
    if (lane < 60) {
      if (gid == 0) acc = acc_start_row(P, Hblk, Lv, dsc, r, *lambda_p);
      apply_ops(P, Lv, acc, g, r, dsc.o0 + gid, dsc.o1, SPLIT * 10, tile[wave]);
#pragma unroll
      for (int c = 0; c < 6; ++c) part[wave][lane][c] = acc.v[c];
    }
    __syncthreads();
    if (threadIdx.x < 36) {
      const double *pf = &part[0][0][0];               // [(wave * 10 + g) * 36 + 6 r + c]
      double s = 0;
      for (int q = 0; q < SPLIT * 10; ++q) s += pf[q * 36 + threadIdx.x];
      Lv[36 * t + threadIdx.x] = s;
    }
    return;
  }
  const int64_t idx = (int64_t)xcd_contiguous(blockIdx.x, n_acc_wg) * 10 + g;
  bool on = lane < 60 && idx < count;
  if (P.task_dirty) {                                       // partial sweep: targets of clean tasks keep their value
    if (on && !P.task_dirty[P.acc_task[first + idx]]) on = false;      // (the same decision on every wave of the workgroup)
    if (!__syncthreads_or(on)) return;
  }
  Row6 acc = {{0, 0, 0, 0, 0, 0}};
  int64_t t = 0;
  if (on) {
    const AccDesc dsc = P.acc_desc[first + idx];
    t = dsc.t;
    if (wave == 0) acc = acc_start_row(P, Hblk, Lv, dsc, r, *lambda_p);
    apply_ops(P, Lv, acc, g, r, dsc.o0 + wave, dsc.o1, SPLIT, tile[wave]);
    if (wave > 0) {
#pragma unroll
      for (int c = 0; c < 6; ++c) part[wave][lane][c] = acc.v[c];
    }
  }
  __syncthreads();
  if (on && wave == 0) {
    for (int w = 1; w < SPLIT; ++w)            // fixed order: deterministic
#pragma unroll
      for (int c = 0; c < 6; ++c) acc.v[c] += part[w][lane][c];
    store_row(Lv + 36 * t + 6 * r, acc);
  }
}

// Column-group accumulate: one workgroup (SPLIT waves) per group of <= 10 targets of ONE column k; lane group g owns
// target (i_g, k), lane r its row r.  The group's entries are the external source columns j, ascending; per entry the B
// operand L(k, j) is the same for every lane of the wave -- its address is wave-uniform, so it is fetched with SCALAR
// loads into SGPRs and costs no vector memory traffic and no LDS exchange -- and lane group g reads only its own A block
// L(i_g, j) (the zero block where row i_g is not in pattern(j)).  Per update 288 bytes instead of 576 and 3 vector loads
// instead of 6 + an LDS round trip; the updates of a target arrive in the same ascending source order and with the same
// arithmetic as in the gather form, so with SPLIT == 1 the factor is bit-identical to k_chol_acc<1> applying whole lists (no
// riders, no long-list role).  SPLIT > 1 splits the GROUP's entry list across the waves (short dependent chains at the skinny
// top), partial rows combined from LDS in a fixed order: a target's updates then fall to other waves than under the gather
// form's split of its own list, and the two agree to rounding only.
template <int SPLIT>
__global__ __launch_bounds__(SPLIT * 64) void k_chol_acc2(DevPlan P, const double *__restrict__ Hblk, double *__restrict__ Lv,
                                                          const double *__restrict__ Lsrc, int64_t group0, int n_groups,
                                                          const double *__restrict__ lambda_p, double *__restrict__ x, int col0) {
  __shared__ __attribute__((aligned(16))) double part[SPLIT][60][6];
  if ((int)blockIdx.x >= n_groups) {                      // fused forward solve: one panel column's external part
    fwd_role<SPLIT>(P, Lv, x, col0, (int)blockIdx.x - n_groups, &part[0][0][0]);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / 6, r = lane - 6 * g;
  const int64_t grp = group0 + xcd_contiguous(blockIdx.x, n_groups);
  if (P.task_dirty && !P.task_dirty[P.g2_task[grp]]) return;
  const int64_t t = lane < 60 ? (int64_t)P.g2_tgt[grp * ACC2_G + g] : -1;
  const bool on = t >= 0;
  Row6 acc = {{0, 0, 0, 0, 0, 0}};
  if (on && wave == 0) acc = (P.dist && t >= P.top_blk0) ? load_row(Lv + 36 * t + 6 * r) : load_A_row(P, Hblk, t, r, *lambda_p);
  const int64_t e0 = P.g2_ptr[grp], e1 = P.g2_ptr[grp + 1];
  const int gg = lane < 60 ? g : 0;
  // two entries in flight: the indices of the next pair are requested before the rows of this pair are used
  int64_t e = e0 + wave;
  int ia0 = e < e1 ? P.g2_a[e * ACC2_G + gg] : P.zero_blk, ib0 = e < e1 ? P.g2_b[e] : P.zero_blk;
  int ia1 = e + SPLIT < e1 ? P.g2_a[(e + SPLIT) * ACC2_G + gg] : P.zero_blk, ib1 = e + SPLIT < e1 ? P.g2_b[e + SPLIT] : P.zero_blk;
  while (e < e1) {
    const int64_t en = e + 2 * SPLIT;
    const int na0 = en < e1 ? P.g2_a[en * ACC2_G + gg] : P.zero_blk, nb0 = en < e1 ? P.g2_b[en] : P.zero_blk;
    const int na1 = en + SPLIT < e1 ? P.g2_a[(en + SPLIT) * ACC2_G + gg] : P.zero_blk, nb1 = en + SPLIT < e1 ? P.g2_b[en + SPLIT] : P.zero_blk;
    const Row6 a0 = load_row(Lsrc + 36 * (int64_t)ia0 + 6 * r), a1 = load_row(Lsrc + 36 * (int64_t)ia1 + 6 * r);
    const double *__restrict__ B0 = Lsrc + 36 * (int64_t)__builtin_amdgcn_readfirstlane(ib0);
    const double *__restrict__ B1 = Lsrc + 36 * (int64_t)__builtin_amdgcn_readfirstlane(ib1);
#pragma unroll
    for (int c = 0; c < 6; ++c)
      acc.v[c] -= a0.v[0] * B0[6 * c] + a0.v[1] * B0[6 * c + 1] + a0.v[2] * B0[6 * c + 2] + a0.v[3] * B0[6 * c + 3] + a0.v[4] * B0[6 * c + 4] + a0.v[5] * B0[6 * c + 5];
#pragma unroll
    for (int c = 0; c < 6; ++c)
      acc.v[c] -= a1.v[0] * B1[6 * c] + a1.v[1] * B1[6 * c + 1] + a1.v[2] * B1[6 * c + 2] + a1.v[3] * B1[6 * c + 3] + a1.v[4] * B1[6 * c + 4] + a1.v[5] * B1[6 * c + 5];
    ia0 = na0; ib0 = nb0; ia1 = na1; ib1 = nb1;
    e = en;
  }
  if (SPLIT > 1) {
    if (on && wave > 0) {
#pragma unroll
      for (int c = 0; c < 6; ++c) part[wave][lane][c] = acc.v[c];
    }
    __syncthreads();
    if (on && wave == 0) {
      for (int w = 1; w < SPLIT; ++w)
#pragma unroll
        for (int c = 0; c < 6; ++c) acc.v[c] += part[w][lane][c];
    }
  }
  if (on && wave == 0) store_row(Lv + 36 * t + 6 * r, acc);
}


// ------------------------------------------------------------------------------------------------
// 1 / sqrt(d): hardware estimate (v_rsq_f64: about 2^-23 relative) + ONE third-order step
//   y1 = y0 (1 + e/2 + 3 e^2/8),  e = 1 - d y0^2      (error ~ e^3: below the rounding of the result)
// arranged as a chain of four dependent operations (t, e, {p | y0 e}, fma) -- the factor kernels are latency chains of
// these: two Newton steps cost eight, a correctly rounded sqrt followed by a correctly rounded division three times as many.
__device__ __forceinline__ double rsqrt_nr(double d) {
  const double y = __builtin_amdgcn_rsq(d);
  const double t = d * y;
  const double e = fma(-t, y, 1.0);              // 1 - d y^2
  const double p = fma(0.375, e, 0.5);
  const double ye = y * e;
  return fma(ye, p, y);
}
// scalar Cholesky of a 6x6 read from LDS (every lane computes the same factor: no second barrier needed).
// L packed lower: index(i,j) = i(i+1)/2 + j; invd[j] = 1 / L_jj.
// RIGHT-LOOKING: column j is scaled, then the trailing triangle is updated at once, so the dependent chain from one pivot
// to the next is rsqrt -> one multiply -> one FMA (about 9 operations per column) instead of the j-deep dot products of
// the left-looking form (these factorisations sit on the critical path of every column of every panel and leaf task).
__device__ __forceinline__ bool chol6_lds(const double *__restrict__ sd, double L[21], double invd[6]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) if (j <= i) L[i * (i + 1) / 2 + j] = sd[i * 6 + j];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double d = L[j * (j + 1) / 2 + j];
    if (!(d > 0.0)) ok = false;
    const double inv = rsqrt_nr(d);
    invd[j] = inv;
    L[j * (j + 1) / 2 + j] = d * inv;
#pragma unroll
    for (int i = 0; i < 6; ++i) if (i > j) L[i * (i + 1) / 2 + j] *= inv;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int k = 0; k < 6; ++k)
        if (i > j && k > j && k <= i) L[i * (i + 1) / 2 + k] = fma(-L[i * (i + 1) / 2 + j], L[k * (k + 1) / 2 + j], L[i * (i + 1) / 2 + k]);
  }
  return ok;
}
// x = u * L^-T for one row, right-looking as well: x_c = u_c / L_cc, then u_c' -= x_c L_c'c for c' > c
__device__ __forceinline__ Row6 trsm_row(const Row6 &u, const double L[21], const double invd[6]) {
  Row6 x, w = u;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    x.v[c] = w.v[c] * invd[c];
#pragma unroll
    for (int c2 = 0; c2 < 6; ++c2) if (c2 > c) w.v[c2] = fma(-x.v[c], L[c2 * (c2 + 1) / 2 + c], w.v[c2]);
  }
  return x;
}

// one workgroup per task: its columns in ascending order; internal updates, 6x6 Cholesky, block TRSM.
// Up to MAXP*NW*10 blocks of a column stay in registers between the update and the TRSM; larger columns
// take extra passes through HBM/L2.
template <int NW, int MAXP>
__global__ __launch_bounds__(NW * 64) void k_chol_fact(DevPlan P, const double *__restrict__ Hblk,
                                                       double *__restrict__ Lv, int task0,
                                                       const double *__restrict__ lambda_p, int *__restrict__ fail_flag) {
  __shared__ __attribute__((aligned(16))) double tile[NW][360];
  __shared__ double sdiag[36];
  const int task = task0 + blockIdx.x;
  if (!task_runs(P, task)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / 6, r = lane - 6 * g;
  const bool lane_on = lane < 60;
  const double lambda = *lambda_p;
  const int c_begin = P.task_ptr[task], c_end = P.task_ptr[task + 1];
  constexpr int PER_PASS = NW * 10;
  for (int ci = c_begin; ci < c_end; ++ci) {
    const int k = P.task_cols[ci];
    const int64_t b0 = P.colptr[k], b1 = P.colptr[k + 1];
    Row6 acc[MAXP];
    // phase 1: finish the accumulation of every block of column k
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      const int64_t t = b0 + (int64_t)(p * NW + wave) * 10 + g;
      if (lane_on && t < b1) {
        const int64_t om = P.op_mid[t];
        acc[p] = (om == P.op_ptr[t] && !(P.dist && t >= P.top_blk0)) ? load_A_row(P, Hblk, t, r, lambda) : load_row(Lv + 36 * t + 6 * r);
        apply_ops(P, Lv, acc[p], g, r, om, P.op_ptr[t + 1], 1, tile[wave]);
        if (t == b0) {
#pragma unroll
          for (int c = 0; c < 6; ++c) sdiag[6 * r + c] = acc[p].v[c];
        }
      }
    }
    for (int64_t t = b0 + (int64_t)(MAXP * NW + wave) * 10 + g; lane_on && t < b1; t += PER_PASS) {   // overflow passes
      const int64_t om = P.op_mid[t];
      Row6 a = (om == P.op_ptr[t] && !(P.dist && t >= P.top_blk0)) ? load_A_row(P, Hblk, t, r, lambda) : load_row(Lv + 36 * t + 6 * r);
      apply_ops(P, Lv, a, g, r, om, P.op_ptr[t + 1], 1, tile[wave]);
      store_row(Lv + 36 * t + 6 * r, a);
    }
    __syncthreads();
    // phase 2: every lane factors the diagonal block (same arithmetic everywhere), then scales its rows
    double Lk[21], invd[6];
    const bool ok = chol6_lds(sdiag, Lk, invd);
    if (!ok && threadIdx.x == 0) atomicOr(fail_flag, 1);
#pragma unroll
    for (int p = 0; p < MAXP; ++p) {
      const int64_t t = b0 + (int64_t)(p * NW + wave) * 10 + g;
      if (lane_on && t < b1) {
        Row6 x;
        if (t == b0) {
#pragma unroll
          for (int rr = 0; rr < 6; ++rr)       // static indices only: Lk must stay in registers
            if (rr == r) {
#pragma unroll
              for (int c = 0; c < 6; ++c) x.v[c] = (c <= rr) ? Lk[rr * (rr + 1) / 2 + c] : 0.0;
            }
        } else {
          x = trsm_row(acc[p], Lk, invd);
        }
        store_row(Lv + 36 * t + 6 * r, x);
      }
    }
    for (int64_t t = b0 + (int64_t)(MAXP * NW + wave) * 10 + g; lane_on && t < b1; t += PER_PASS) {
      const Row6 u = load_row(Lv + 36 * t + 6 * r);
      store_row(Lv + 36 * t + 6 * r, trsm_row(u, Lk, invd));
    }
    __syncthreads();
  }
}

// Leaf levels: a task is a self-contained light sub-tree -- contiguous columns, hence ONE contiguous range of L blocks,
// no updates from outside.  The whole range lives in LDS under local indices (block t -> t - base) while the task is
// factored: every update reads its two source blocks from LDS instead of L2 / HBM (the generic kernel re-reads each
// block ~20 times; at cfg 5 level 0 alone moved 40 GB per sweep through the caches), and L goes to memory once, as
// one coalesced copy.  The task's op lists are staged in LDS too (16-bit local ids), so the column loop touches no
// global memory at all (with the indices streamed from memory the kernel was bound by two dependent loads per column).
template <int NW>
__global__ __launch_bounds__(NW * 64) void k_chol_leaf(DevPlan P, const double *__restrict__ Hblk, double *__restrict__ Lv, int task0,
                                                       const double *__restrict__ lambda_p, int *__restrict__ fail_flag, int lds_blocks,
                                                       int lds_cols, double *__restrict__ x) {
  // [lds_blocks][36] blocks of L | the diagonal block being factored | right-hand side r and forward solution y of the
  // task's columns | op list offsets | local column of every block's row (0xffff: outside the task) | ops as
  // (a << 16 | b), local ids.  With x != nullptr the forward solve L y = b of the task's columns rides along (x holds b
  // on entry): once column k is final every lane knows L_kk, computes y_k and subtracts L_ik y_k from the rows i of its
  // own blocks -- column-oriented substitution with no extra barrier and no extra pass over L.
  extern __shared__ __attribute__((aligned(16))) double Ls[];
  // one descriptor per task (structure_upload.cpp "LeafDesc"): in a full sweep the level's tasks by descending work, in a partial sweep
  // (a task range) in task order
  const LeafDesc dsc = (P.task_dirty ? P.pp.leaf_desc : P.pp.leaf_lpt)[task0 + blockIdx.x];
  const int task = dsc.task;
  if (!task_runs(P, task)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / 6, r = lane - 6 * g;
  const bool lane_on = lane < 60;
  const double lambda = *lambda_p;
  const int m = dsc.m;
  const int k0 = dsc.k0;
  const int64_t base = dsc.base;
  const int nblk = dsc.nblk;
  double *__restrict__ sdiag = Ls + 36 * lds_blocks;
  double *__restrict__ xr = sdiag + 36;                              // [lds_cols][6] running right-hand side
  double *__restrict__ yr = xr + 6 * lds_cols;                       // [lds_cols][6] forward solution
  int *__restrict__ lcolp = reinterpret_cast<int *>(yr + 6 * lds_cols);   // [lds_cols + 2] first block of every column (local), staged once: the column loop reads it from LDS
  int *__restrict__ lptr = lcolp + lds_cols + 2;
  unsigned short *__restrict__ lrow = reinterpret_cast<unsigned short *>(lptr + lds_blocks + 1);
  unsigned *__restrict__ lop = reinterpret_cast<unsigned *>(lrow + 2 * ((lds_blocks + 1) / 2));
  const int64_t obase = dsc.obase;
  const int nops = dsc.nops;
  for (int q = threadIdx.x; q <= m; q += NW * 64) lcolp[q] = (int)(P.colptr[k0 + q] - base);
  for (int q = threadIdx.x; q <= nblk; q += NW * 64) lptr[q] = (int)(P.op_ptr[base + q] - obase);
  if (x) {
    for (int q = threadIdx.x; q < nblk; q += NW * 64) { const int i = P.rowidx[base + q] - k0; lrow[q] = (unsigned short)(i < m ? i : 0xffff); }
    for (int i = threadIdx.x; i < 6 * m; i += NW * 64) xr[i] = x[6 * (int64_t)k0 + i];
  }
  for (int i = threadIdx.x; i < nops; i += NW * 64)
    lop[i] = ((unsigned)(P.op_a[obase + i] - (int)base) << 16) | (unsigned)(P.op_b[obase + i] - (int)base);
  for (int q = wave * 10 + g; lane_on && q < nblk; q += NW * 10) store_row(Ls + 36 * q + 6 * r, load_A_row(P, Hblk, base + q, r, lambda));
  __syncthreads();
  for (int ci = 0; ci < m; ++ci) {
    const int b0 = lcolp[ci], b1 = lcolp[ci + 1];
    for (int q = b0 + wave * 10 + g; lane_on && q < b1; q += NW * 10) {
      Row6 acc = load_row(Ls + 36 * q + 6 * r);
      int o = lptr[q];
      const int o1 = lptr[q + 1];
      for (; o + 1 < o1; o += 2) {
        const unsigned p0 = lop[o], p1 = lop[o + 1];
        const Row6 a0 = load_row(Ls + 36 * (int)(p0 >> 16) + 6 * r), a1 = load_row(Ls + 36 * (int)(p1 >> 16) + 6 * r);
        row_update(acc, a0, Ls + 36 * (int)(p0 & 0xffffu));
        row_update(acc, a1, Ls + 36 * (int)(p1 & 0xffffu));
      }
      if (o < o1) { const unsigned p0 = lop[o]; row_update(acc, load_row(Ls + 36 * (int)(p0 >> 16) + 6 * r), Ls + 36 * (int)(p0 & 0xffffu)); }
      store_row(Ls + 36 * q + 6 * r, acc);                              // sources are blocks of earlier columns: no hazard
      if (q == b0) store_row(sdiag + 6 * r, acc);
    }
    __syncthreads();
    double Lk[21], invd[6];
    const bool ok = chol6_lds(sdiag, Lk, invd);
    if (!ok && threadIdx.x == 0) atomicOr(fail_flag, 1);
    double yk[6] = {0, 0, 0, 0, 0, 0};
    if (x) {                                                            // y_k = L_kk^-1 r_k, the same arithmetic on every lane
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) {
        double sv = xr[6 * ci + rr];
#pragma unroll
        for (int c = 0; c < 6; ++c) if (c < rr) sv -= Lk[rr * (rr + 1) / 2 + c] * yk[c];
        yk[rr] = sv * invd[rr];
      }
    }
    for (int q = b0 + wave * 10 + g; lane_on && q < b1; q += NW * 10) {
      Row6 lq;
      if (q == b0) {
#pragma unroll
        for (int rr = 0; rr < 6; ++rr)                                  // static indices only: Lk must stay in registers
          if (rr == r) {
#pragma unroll
            for (int c = 0; c < 6; ++c) lq.v[c] = (c <= rr) ? Lk[rr * (rr + 1) / 2 + c] : 0.0;
          }
        if (x) {
#pragma unroll
          for (int rr = 0; rr < 6; ++rr) if (rr == r) yr[6 * ci + rr] = yk[rr];
        }
      } else {
        lq = trsm_row(load_row(Ls + 36 * q + 6 * r), Lk, invd);
        if (x) {
          const int i2 = lrow[q];
          if (i2 != 0xffff)                                             // rows inside the task; the others gather later
            xr[6 * i2 + r] -= lq.v[0] * yk[0] + lq.v[1] * yk[1] + lq.v[2] * yk[2] + lq.v[3] * yk[3] + lq.v[4] * yk[4] + lq.v[5] * yk[5];
        }
      }
      store_row(Ls + 36 * q + 6 * r, lq);
    }
    __syncthreads();
  }
  if (x) for (int i = threadIdx.x; i < 6 * m; i += NW * 64) x[6 * (int64_t)k0 + i] = yr[i];
  double2 *__restrict__ dst = reinterpret_cast<double2 *>(Lv + 36 * base);
  const double2 *__restrict__ src = reinterpret_cast<const double2 *>(Ls);
  for (int i = threadIdx.x; i < nblk * 18; i += NW * 64) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------------
// Panels (the skinny top of the elimination tree).  A panel = m <= PM columns forming a path of the tree: a dense
// m x m lower triangle of blocks plus off-triangle rows that all start at some column and run to the last one.
// External updates were already applied by k_chol_acc.  k_panel_tri factors the triangle on chip (packed triangle in
// LDS, trailing matrix in f64 MFMA accumulator tiles, one barrier per column) and leaves it behind as 16x16 operand
// tiles; k_panel_rows then finishes the off-triangle rows as a blocked TRSM on MFMA (16 scalar rows per wave, the
// right-hand side riding along as one more row); k_bwd_ext / k_bwd_tri do the backward solve from the same tiles.
struct PairTab { unsigned char a[PM * (PM + 1) / 2], b[PM * (PM + 1) / 2]; };    // (a, b), b <= a, a ascending
constexpr PairTab make_pairs() {
  PairTab t{};
  int q = 0;
  for (int a = 0; a < PM; ++a)
    for (int b = 0; b <= a; ++b) { t.a[q] = (unsigned char)a; t.b[q] = (unsigned char)b; ++q; }
  return t;
}
__constant__ PairTab PAIRS = make_pairs();
#define PAIR_A PAIRS.a
#define PAIR_B PAIRS.b
// packed lower triangle of 6x6 blocks in LDS: block (rr, kk), kk <= rr
#define TRI(rr, kk) ((((rr) * ((rr) + 1)) / 2 + (kk)) * 36)

template <bool FROM_LDS>
__device__ __forceinline__ Row6 trsm_row_blk(const Row6 &u, const double *__restrict__ L) {   // L: 6x6 row-major, lower
  Row6 x;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double s = u.v[c];
#pragma unroll
    for (int m = 0; m < 6; ++m) if (m < c) s -= x.v[m] * L[6 * c + m];
    x.v[c] = s / L[7 * c];
  }
  return x;
}

// Rider role of a 16-wave k_panel_tri launch (symbolic.cpp "riders"): workgroup wg takes items 4 wg .. 4 wg + 3, four waves
// each -- the 40 lane groups stride the item's op range like the long-list role of k_chol_acc, partial blocks are summed in
// a fixed order, and the target's value so far goes (back) to L.  smem: 16 x 360 doubles (a wave's exchange tile, then its
// partial rows).
__device__ __forceinline__ void ride_items16(const DevPlan &P, const double *__restrict__ Hblk, double *__restrict__ Lv,
                                             const double *__restrict__ lambda_p, int item0, int nitems, int wg, double *__restrict__ smem) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / 6, r = lane - 6 * g;
  const int part = wave >> 2, w4 = wave & 3;
  const int ii = RIDE_PER_WG * wg + part;
  const bool have = ii < nitems;
  const RideItem it = P.ride_items[item0 + (have ? ii : 0)];
  const bool run = have && (!P.task_dirty || P.task_dirty[it.task]);
  double *__restrict__ tile = smem + 360 * wave;
  if (run && lane < 60) {
    const int gid = w4 * 10 + g;
    Row6 acc = {{0, 0, 0, 0, 0, 0}};
    if (gid == 0 && it.first != 2) acc = it.first ? load_A_row(P, Hblk, it.t, r, *lambda_p) : load_row(Lv + 36 * (int64_t)it.t + 6 * r);
    apply_ops(P, Lv, acc, g, r, it.o0 + gid, it.o0 + it.n, 40, tile);
#pragma unroll
    for (int c = 0; c < 6; ++c) tile[6 * lane + c] = acc.v[c];       // (the wave's own tile: its DS operations are in order)
  }
  __syncthreads();
  const int tl = (int)threadIdx.x - 256 * part;
  if (run && tl < 36) {
    const double *pf = smem + 1440 * part;                            // [(w4 * 10 + g) * 36 + 6 r + c]
    double sum = 0;
    for (int q = 0; q < 40; ++q) sum += pf[q * 36 + tl];
    Lv[36 * (int64_t)it.t + tl] = it.first == 2 ? -sum : sum;         // (a hub piece: the scratch block receives + sum L_a L_b^T)
  }
}

// Dense Cholesky of a panel's triangle (<= PM block columns, <= 6 PM scalar columns), entirely on chip.  The packed
// lower triangle of 6x6 blocks sits in LDS (PM = 32: 528 blocks = 152 KB); the trailing matrix lives in registers as
// 16x16 f64 MFMA accumulator tiles spread over waves 1 .. NW-1.  Wave 0 runs the sequential pivot chain, one block
// column per phase and one barrier per phase:
//   wave 0, phase k:   column k (staged in LDS with the updates of columns < k-1) gets the update of column k-1, the
//                      6x6 diagonal block is factored, the rows below are scaled -> V(k) (final L blocks) in LDS
//   the others:        rank-6 update C -= V(k-1) V(k-1)^T (two MFMAs per tile), then they stage column k+1 (now
//                      carrying the updates of columns <= k-1) for the phase after next
// so the MFMA work and the staging hide behind the pivot chain instead of alternating with it.  Epilogue: L blocks to
// global memory, and the same triangle once more as 16x16 tiles in MFMA operand order (strictly-lower tiles negated,
// diagonal tiles inverted) for k_panel_rows and the panel solves.
template <int NW>
__global__ __launch_bounds__(NW * 64) void k_panel_tri(DevPlan P, const double *__restrict__ Hblk, double *__restrict__ Lv, int pn0,
                                                    const double *__restrict__ lambda_p, int *__restrict__ fail_flag, int n_pn, int ride0, int n_ride, int n_real) {
  __shared__ __attribute__((aligned(16))) double T[PM * (PM + 1) / 2 * 36];
  if (NW == 16) {
    // workgroups beyond the level's panels: riders (early accumulate work of later levels, while the pivot chains run)
    __shared__ __attribute__((aligned(16))) double ride_smem[NW == 16 ? 16 * 360 : 2];
    if ((int)blockIdx.x >= n_pn) {
      // every XCD takes a contiguous range of the items (n_pn is padded to a multiple of 8 by the launcher when riders exist, so
      // the XCD of a rider workgroup is (blockIdx - n_pn) & 7): items of neighbouring targets share their source blocks
      const int nwg = (int)gridDim.x - n_pn;
      ride_items16(P, Hblk, Lv, lambda_p, ride0, n_ride, P.ride_xcd ? xcd_contiguous((int)blockIdx.x - n_pn, nwg) : (int)blockIdx.x - n_pn, ride_smem);
      return;
    }
  }
  const long long t_begin = __builtin_readcyclecounter();
  if ((int)blockIdx.x >= n_real) return;                       // padding between the panels and the riders
  // (NW == 8: the throughput form of a wide level -- panels in width order in a full sweep, PanelPlan::tri_order; a partial sweep launches a task range)
  const int pn = (NW == 8 && !P.task_dirty) ? P.pp.tri_order[pn0 + blockIdx.x] : pn0 + (int)blockIdx.x;
  const PanelDesc dsc = P.pp.pdesc[pn];
  if (!task_runs(P, dsc.task)) return;
  const int m = dsc.m;
  const int64_t tri0 = (int64_t)pn * (PM * PM);
  const int *__restrict__ tb = P.pp.ptri_blk + tri0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / 6, r = lane - 6 * g;
  const bool lane_on = lane < 60;
  const int gid = wave * 10 + g;
  const double lambda = *lambda_p;
  const int npair = m * (m + 1) / 2;
  for (int gq = gid; lane_on && gq < npair; gq += NW * 10) {
    const int rr = PAIR_A[gq], kk = PAIR_B[gq];
    const int sc = P.pp.ptri_src[tri0 + rr * PM + kk];
    const double *base = sc >= 0 ? Lv + 36 * (int64_t)sc : (sc <= -2 ? Hblk + 36 * (int64_t)(-2 - sc) : Lv + 36 * (int64_t)P.zero_blk);
    Row6 x = load_row(base + 6 * r);
    if (sc <= -2 && rr == kk) {                         // setLambda on a diagonal block that comes straight from H
#pragma unroll
      for (int c = 0; c < 6; ++c) x.v[c] += (c == r) ? lambda : 0.0;
    }
    store_row(&T[36 * gq + 6 * r], x);                  // PAIR order == packed order
  }
  __syncthreads();
  // (Two separate loops with matching barrier counts: the register allocator then sees max(pivot chain, worker),
  //  not their union, which at 16 waves per workgroup -- 128 VGPRs -- is the difference between fitting and spilling.)
  const int n = 6 * m, nJ = (n + 15) >> 4;
  // profiling hook (FGO_TRI_PROF): stamps of the pivot wave of a single-panel launch, 5 per column + 4 for the kernel
  long long *__restrict__ stamp = (P.prof_tri && n_real == 1 && m == PM) ? reinterpret_cast<long long *>(P.partial) : nullptr;
  if (stamp && threadIdx.x == 0) { stamp[0] = t_begin; stamp[1] = __builtin_readcyclecounter(); }
  if (wave == 0) {
    constexpr int HMAX = (PM + 9) / 10;
    for (int k = 0; k < m; ++k) {
      if (stamp && lane == 0) stamp[8 + 5 * k] = __builtin_readcyclecounter();
      // rows rr = k + g (+10 h): update with column k-1, then the diagonal block goes back to LDS for the 6x6 factor.
      // The update runs over the inner index j on the outside, so that the six accumulators of a row advance together
      // (six independent FMA chains instead of six dot products one after the other: the wave is a latency chain here).
      Row6 acc[HMAX];
#pragma unroll
      for (int h = 0; h < HMAX; ++h) {
        const int rr = k + g + 10 * h;
        if (lane_on && rr < m) {
          acc[h] = load_row(&T[TRI(rr, k) + 6 * r]);
          if (k > 0) {
            const Row6 a = load_row(&T[TRI(rr, k - 1) + 6 * r]);
            const double *__restrict__ B = &T[TRI(k, k - 1)];
#pragma unroll
            for (int j = 0; j < 6; ++j)
#pragma unroll
              for (int c = 0; c < 6; ++c) acc[h].v[c] = fma(-a.v[j], B[6 * c + j], acc[h].v[c]);
          }
        }
      }
      if (lane_on && g == 0) store_row(&T[TRI(k, k) + 6 * r], acc[0]);
      __builtin_amdgcn_wave_barrier();
      if (stamp && lane == 0) stamp[8 + 5 * k + 1] = __builtin_readcyclecounter();
      double Lk[21], invd[6];
      const bool ok = chol6_lds(&T[TRI(k, k)], Lk, invd);
      if (!ok && lane == 0) atomicOr(fail_flag, 1);
      __builtin_amdgcn_wave_barrier();                    // everybody has read the diagonal block before it is overwritten
      if (stamp && lane == 0) stamp[8 + 5 * k + 2] = __builtin_readcyclecounter() + (long long)(Lk[0] == 12345.678);
#pragma unroll
      for (int h = 0; h < HMAX; ++h) {
        const int rr = k + g + 10 * h;
        if (lane_on && rr < m) {
          // (the rows of the diagonal block take the same path: row r of D L^-T IS row r of L -- equal to the wave's Lk up to
          //  the last bit, with the entries right of the diagonal forced to zero; no 36-way select, no second store pattern)
          Row6 x = trsm_row(acc[h], Lk, invd);
          if (rr == k) {
#pragma unroll
            for (int c = 0; c < 6; ++c) x.v[c] = (c <= r) ? x.v[c] : 0.0;
          }
          store_row(&T[TRI(rr, k) + 6 * r], x);
        }
      }
      if (stamp && lane == 0) stamp[8 + 5 * k + 3] = __builtin_readcyclecounter();
      __syncthreads();
      if (stamp && lane == 0) stamp[8 + 5 * k + 4] = __builtin_readcyclecounter();
    }
  } else {
    const int nn = lane & 15, q4 = lane >> 4;
    const int ntile = nJ * (nJ + 1) / 2;                     // lower tiles incl. the diagonal ones, PAIR order (I, K), K <= I
    // EXCL (the 16-wave instantiation): the waves that share a SIMD with the pivot wave (4, 8, 12: waves are dealt round-robin
    // to the four SIMDs) take no tiles, so the pivot chain -- the critical path of the kernel -- has a SIMD's issue slots to
    // itself.  Measured with FGO_TRI_PROF (tools/tri_prof.py): a column of the chain costs ~3 400 cycles when the pivot wave
    // shares its SIMD with three worker waves.
    constexpr bool EXCL = NW >= 16;
    constexpr int NWORK = EXCL ? NW - NW / 4 : NW - 1;
    constexpr int NT = (NJMAX * (NJMAX + 1) / 2 + NWORK - 1) / NWORK;
    const bool idle = EXCL && (wave & 3) == 0;
    const int aw = EXCL ? wave - 1 - (wave >> 2) : wave - 1;
    // per owned tile: LDS offsets of the V rows feeding the A / B operands and of the four result rows, packed triangle:
    // element (scalar row i, block column k, in-block column c) sits at  base(i) + 36 k + c,  base(i) = TRI(i / 6, 0) + 6 (i % 6)
    d4_t C[NT];
    bool own[NT];
    int offA[NT], rrA[NT], offB[NT], rrB[NT], cj[NT], offE[NT][4], rrE[NT][4], tI[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int p = aw + NWORK * u;
      own[u] = !idle && p < ntile;
      const int I = PAIR_A[own[u] ? p : 0], K = PAIR_B[own[u] ? p : 0];
      tI[u] = I;
      const int iA = 16 * I + nn, iB = 16 * K + nn;
      rrA[u] = iA < n ? iA / 6 : -1; offA[u] = TRI(iA / 6, 0) + (iA % 6) * 6;
      rrB[u] = iB < n ? iB / 6 : -1; offB[u] = TRI(iB / 6, 0) + (iB % 6) * 6;
      cj[u] = iB % 6;
      C[u] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int i = 16 * I + q4 + 4 * r4;
        rrE[u][r4] = i < n ? i / 6 : -1; offE[u][r4] = TRI(i / 6, 0) + (i % 6) * 6;
        if (own[u] && rrE[u][r4] >= 0 && rrB[u] >= 0 && rrE[u][r4] >= rrB[u]) C[u][r4] = T[offE[u][r4] + 36 * rrB[u] + cj[u]];
      }
    }
    // phase 0 has nothing for the workers (columns 0 and 1 are staged by the initial load): LDS is not written before
    // the first barrier, so reading the initial values above needs no extra barrier
    for (int k = 0; k < m; ++k) {
      if (k > 0) {
#pragma unroll
        for (int u = 0; u < NT; ++u)
          if (own[u] && 16 * tI[u] + 15 >= 6 * k) {             // tile reaches into the part right of column k-1
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
              const int c = 4 * kc + q4;
              double a = 0.0, b = 0.0;
              if (c < 6) {
                if (rrA[u] > k - 1) a = -T[offA[u] + (k - 1) * 36 + c];
                if (rrB[u] > k - 1) b = T[offB[u] + (k - 1) * 36 + c];
              }
              C[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, C[u], 0, 0, 0);
            }
          }
#pragma unroll
        for (int u = 0; u < NT; ++u)
          if (own[u] && rrB[u] == k + 1) {                      // stage column k+1 for the phase after next
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4)
              if (rrE[u][r4] >= k + 1) T[offE[u][r4] + (k + 1) * 36 + cj[u]] = C[u][r4];
          }
      }
      __syncthreads();
    }
  }
  if (stamp && threadIdx.x == 0) stamp[2] = __builtin_readcyclecounter();
  // ---- Epilogue: the L blocks go to global memory, and the factored triangle once more as a dense scalar matrix cut into
  // 16x16 tiles in MFMA A-operand order (lane l <-> element [l & 15][4 kc + (l >> 4)] of the tile, i.e. column-major):
  // strictly-lower tiles NEGATED, diagonal tiles INVERTED.  Only the tiles of the nJ tile rows the panel really has are
  // written / read.  The inverses are the one dependent chain left after the last pivot.  In the 16-wave form (one or two
  // panels per level: the launch lasts as long as its chain) they come first and have waves 0 and 1 to themselves, while the
  // other waves copy the L blocks and the lower tiles out (stores nobody waits for).  The 8-wave throughput form copies
  // first with all waves, as its register budget (128, two workgroups per CU) has no room for the two roles side by side.
  auto Ls = [&](int i, int j) -> double {
    if (i >= n || j >= n) return (i == j) ? 1.0 : 0.0;          // identity padding up to the tile boundary
    const int rr = i / 6, kk = j / 6;
    if (rr < kk) return 0.0;
    return T[TRI(rr, kk) + (i - 6 * rr) * 6 + (j - 6 * kk)];
  };
  double *__restrict__ tp = P.pp.ptop + (int64_t)dsc.top * 256;
  __shared__ double Dt[NJMAX * 256];                            // the diagonal tiles, staged in LDS (51 KB with the triangle image)
  __shared__ double Dr[NW >= 16 ? NJMAX * 16 : 1];              // the reciprocals of their diagonals (16-wave form)
  // lane groups gq0, gq0 + gstep, ... copy the L blocks, threads e0, e0 + estep, ... the elements of the lower tiles
  auto copy_out = [&](int gq0, int gstep, int e0, int estep) {
    for (int gq = gq0; lane_on && gq < npair; gq += gstep) {
      const int rr = PAIR_A[gq], kk = PAIR_B[gq];
      const int t = tb[rr * PM + kk];
      if (t >= 0) store_row(Lv + 36 * (int64_t)t + 6 * r, load_row(&T[36 * gq + 6 * r]));
    }
    for (int e = e0; e < (nJ * (nJ - 1) / 2) * 256; e += estep) {   // tiles (J, I), I < J < nJ, are the first nJ (nJ-1) / 2
      const int tile = e >> 8, kc = (e >> 6) & 3, l = e & 63;
      const int J = PAIR_A[tile] + 1, I = PAIR_B[tile];
      tp[e] = -Ls(16 * J + (l & 15), 16 * I + 4 * kc + (l >> 4));
    }
  };
  auto invert = [&]() {
    if ((int)threadIdx.x < 16 * nJ) {                           // column c of the inverse of diagonal tile J, straight to memory
      const int J = threadIdx.x >> 4, c = threadIdx.x & 15;
      double xc[16];
      // column c of Dt^-1 by forward substitution, right-looking: the 16 reciprocals first (independent of the chain; the 16-wave
      // form computes one per lane of the tile's 16 and shares them through LDS: one division in front of the chain instead of 16
      // in a lane's instruction stream), then per step one multiply and the updates of the rows below (chain: 2 operations per
      // row instead of a dot product and a division)
      const double *__restrict__ D = &Dt[J * 256];
      if (NW >= 16) {
        Dr[threadIdx.x] = 1.0 / D[c * 17];
        __builtin_amdgcn_wave_barrier();                          // (the 16 lanes of a tile are lanes of one wave)
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) xc[i] = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        xc[i] *= NW >= 16 ? Dr[16 * J + i] : 1.0 / D[i * 17];     // (the same correctly rounded quotient either way)
#pragma unroll
        for (int i2 = 0; i2 < 16; ++i2) if (i2 > i) xc[i2] = fma(-D[i2 * 16 + i], xc[i], xc[i2]);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) tp[(NLT + J) * 256 + 16 * c + i] = xc[i];
    }
  };
  if (NW < 16) copy_out(gid, NW * 10, (int)threadIdx.x, NW * 64);
  for (int e = threadIdx.x; e < nJ * 256; e += NW * 64) Dt[e] = Ls(16 * (e >> 8) + ((e >> 4) & 15), 16 * (e >> 8) + (e & 15));
  __syncthreads();
  if (NW < 16 || wave < 2) invert();
  else copy_out(gid - 20, (NW - 2) * 10, (int)threadIdx.x - 128, (NW - 2) * 64);
  if (stamp && threadIdx.x == 0) { stamp[3] = __builtin_readcyclecounter(); stamp[4] = wall_clock64(); }
}

// ---- THROUGHPUT form of the triangle kernel for the WIDE levels (more panels than k_panel_tri<16> has CUs for): ONE WAVE per
// panel, no workgroup barrier anywhere.  k_panel_tri spends a panel's time in a pivot chain on one wave while the other waves
// of its workgroup wait at barriers -- right where one or two panels exist per level, wasteful where there are thousands
// (cfg 2 level 1: 2 047 panels, two 8-wave workgroups per CU, four rounds of ~40 us).  Here a wave keeps the whole trailing
// matrix of its panel as 21 f64 MFMA accumulator tiles (168 registers) and walks the block columns on its own:
//   column k:  the accumulated updates of its 6 scalar columns leave the tiles through a 4.6 KB LDS image (C layout ->
//              one scalar row per lane), are added to the column's own values (a 48-byte row of a block of L or H per lane,
//              requested one column ahead), 6x6 Cholesky + row TRSM as in k_panel_tri, the finished rows go to L, to the
//              operand tiles `ptop` (strictly-lower tiles negated, in A-operand order) and back to the LDS image, from
//              which every lane picks its MFMA operands:  C(I, K) -= V_I V_K^T, two v_mfma_f64_16x16x4 per live tile.
// Diagonal tiles are collected in LDS and inverted at the end (16 lanes per tile, right-looking substitution).  Same contract
// as k_panel_tri (L blocks + ptop), so k_panel_rows, the solves and the backward kernels do not know which one ran.
// A column is a chain of dependent steps with little to issue beside it, so the kernel is held to TWO waves per SIMD
// (amdgpu_waves_per_eu(2, 2): 256 registers, no scratch; 19 232 B of LDS, eight workgroups per CU), where one wave's chain
// fills the other's gaps: tests/test_tri1_resources.py holds the compiler's resource report to that budget.
constexpr int tri1_tile(int I, int K) { return I * (I + 1) / 2 + K; }
constexpr int TRI1_NR = 16 * NJMAX;                               // scalar rows incl. the padding of the last tile row
struct Tri1Ctx {                                                  // wave-uniform / per-lane constants of a panel
  const double *Hblk; double *Lv; double *tp; int64_t zero_blk;
  int m, n, nJ, lane, nn, q;
  double lambda;
  int rr[2], rho[2];
  bool rv[2], rpad[2];
};
__device__ __forceinline__ const double *tri1_src_row(const Tri1Ctx &X, const int *__restrict__ tsrc, int h, int k) {
  const int sc = tsrc[X.rr[h] * PM + k];
  const double *base = sc >= 0 ? X.Lv + 36 * (int64_t)sc : (sc <= -2 ? X.Hblk + 36 * (int64_t)(-2 - sc) : X.Lv + 36 * X.zero_blk);
  return base + 6 * X.rho[h];
}
// ---- the 6x6 factor of a column WITHOUT 54 registers of wave-uniform values in every lane (chol6_lds: Lk[21] + invd[6] next to
// 168 accumulator registers kept the kernel at one wave per SIMD).  Lane i < 6 holds ROW i of the block (the other lanes repeat
// row 5 and are never read); a pivot and the finished column below it travel to all lanes through v_readlane, i.e. as SCALAR
// operands of the v_mul / v_fma that use them, and stay in scalar registers for the row TRSM.  Every element sees the
// operations of chol6_lds on the same values in the same order (d * inv, L_ij * inv, fma(-L_ij, L_kj, L_ik) for ascending j):
// the same bits.  The chain per pivot grows by two v_readlane pairs.
__device__ __forceinline__ double tri1_bcast(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
constexpr int tri1_low(int i, int j) { return i * (i - 1) / 2 + j; }   // strictly lower, packed: i > j
__device__ __forceinline__ bool tri1_chol6(const double *__restrict__ sd, int lane, double (&Ls)[15], double (&invd)[6]) {
  Row6 row = load_row(&sd[6 * (lane < 5 ? lane : 5)]);
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double d = tri1_bcast(row.v[j], j);
    if (!(d > 0.0)) ok = false;
    const double inv = rsqrt_nr(d);
    invd[j] = inv;
    row.v[j] *= inv;
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (k > j) {
        const double lkj = tri1_bcast(row.v[j], k);
        Ls[tri1_low(k, j)] = lkj;
        row.v[k] = fma(-row.v[j], lkj, row.v[k]);                   // (rows i < k carry values nobody reads)
      }
  }
  return ok;
}
__device__ __forceinline__ Row6 tri1_trsm_row(const Row6 &u, const double (&Ls)[15], const double (&invd)[6]) {   // = trsm_row
  Row6 x, w = u;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    x.v[c] = w.v[c] * invd[c];
#pragma unroll
    for (int c2 = 0; c2 < 6; ++c2) if (c2 > c) w.v[c2] = fma(-x.v[c], Ls[tri1_low(c2, c)], w.v[c2]);
  }
  return x;
}
// block column K of a panel, K a compile-time constant: every tile index below is static, so the 21 accumulator tiles stay
// in registers (a run-time column index made the compiler address them through v_readlane / v_accvgpr chains: 75 us per panel)
template <int K>
__device__ __forceinline__ void tri1_step(const Tri1Ctx &X, d4_t (&C)[NJMAX * (NJMAX + 1) / 2], Row6 (&sN)[2], bool &ok_all,
                                          double *__restrict__ W, double *__restrict__ Dt, double *__restrict__ D6,
                                          const int *__restrict__ tsrc, const int *__restrict__ tblk) {
  constexpr int c0 = 6 * K, K0 = c0 >> 4, K1 = (c0 + 5) >> 4;       // tile columns the block column lies in
  const int lane = X.lane, nn = X.nn, q = X.q;
  Row6 s[2] = {sN[0], sN[1]};
  if (K + 1 < X.m) {                                               // request the next column's rows now: they arrive behind this column's chain
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (X.rv[h] && X.rr[h] >= K + 1) sN[h] = load_row(tri1_src_row(X, tsrc, h, K + 1));
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)                                      // setLambda on a diagonal block that comes straight from H
    if (X.rv[h] && X.rr[h] == K && tsrc[K * PM + K] <= -2) {
#pragma unroll
      for (int c = 0; c < 6; ++c) s[h].v[c] += (c == X.rho[h]) ? X.lambda : 0.0;
    }
  if constexpr (K > 0) {
    // ---- the updates of columns < K leave the accumulator tiles: element (row 16 I + q + 4 r4, column 16 Kt + nn)
#pragma unroll
    for (int I = 0; I < NJMAX; ++I)
#pragma unroll
      for (int Kt = 0; Kt < NJMAX; ++Kt)
        if ((Kt == K0 || Kt == K1) && Kt <= I && 16 * I + 15 >= c0 && I < X.nJ) {
          const int c = 16 * Kt + nn - c0;
          if (c >= 0 && c < 6) {
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) W[(16 * I + q + 4 * r4) * 6 + c] = C[tri1_tile(I, Kt)][r4];
          }
        }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (X.rv[h] && X.rr[h] >= K) {
        const Row6 e = load_row(&W[(lane + 64 * h) * 6]);
#pragma unroll
        for (int c = 0; c < 6; ++c) s[h].v[c] += e.v[c];
      }
  }
  // ---- 6x6 factor of the diagonal block, TRSM of the rows below
#pragma unroll
  for (int h = 0; h < 2; ++h)
    if (X.rv[h] && X.rr[h] == K) store_row(&D6[6 * X.rho[h]], s[h]);
  __builtin_amdgcn_wave_barrier();
  double Lk[15], invd[6];
  ok_all = tri1_chol6(D6, lane, Lk, invd) && ok_all;
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h == 1 && 16 * X.nJ <= 64) continue;                       // (wave-uniform: no rows 64 .. 95)
    const int i = lane + 64 * h;
    Row6 v = {{0, 0, 0, 0, 0, 0}};
    if (X.rv[h] && X.rr[h] >= K) {
      v = tri1_trsm_row(s[h], Lk, invd);
      if (X.rr[h] == K) {
#pragma unroll
        for (int c = 0; c < 6; ++c) v.v[c] = (c <= X.rho[h]) ? v.v[c] : 0.0;
      }
      const int t = tblk[X.rr[h] * PM + K];
      if (t >= 0) store_row(X.Lv + 36 * (int64_t)t + 6 * X.rho[h], v);
    }
    if (X.rpad[h] && i >= c0) {
      store_row(&W[i * 6], v);                                      // (rows of the padding carry zeros)
      const int J = i >> 4, a = i & 15;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        constexpr int dummy = 0; (void)dummy;
        const int col = c0 + c, I = col >> 4, b = col & 15;         // constants
        if (J > I) X.tp[(J * (J - 1) / 2 + I) * 256 + 16 * b + a] = -v.v[c];
        else if (J == I && X.rv[h]) Dt[J * 256 + 16 * a + b] = v.v[c];
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  // ---- rank-6 update of the trailing tiles: operands from the column image (rows at or above the diagonal block -> 0)
  if (K + 1 < X.m) {
    constexpr int I0 = (c0 + 6) >> 4;
    double av[NJMAX][2];
#pragma unroll
    for (int I = 0; I < NJMAX; ++I)
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        const int row = 16 * I + nn, c = 4 * kc + q;
        av[I][kc] = (I >= I0 && I < X.nJ && c < 6 && row >= c0 + 6 && row < X.n) ? W[row * 6 + c] : 0.0;
      }
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
      for (int I = 0; I < NJMAX; ++I)
#pragma unroll
        for (int Kt = 0; Kt < NJMAX; ++Kt)
          if (Kt <= I && Kt >= I0 && I < X.nJ)
            C[tri1_tile(I, Kt)] = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[I][kc], av[Kt][kc], C[tri1_tile(I, Kt)], 0, 0, 0);
    __builtin_amdgcn_wave_barrier();                                // (the operand reads are done before the next column's image is written)
  }
}
template <int K>
__device__ __forceinline__ void tri1_steps(const Tri1Ctx &X, d4_t (&C)[NJMAX * (NJMAX + 1) / 2], Row6 (&sN)[2], bool &ok_all,
                                           double *__restrict__ W, double *__restrict__ Dt, double *__restrict__ D6,
                                           const int *__restrict__ tsrc, const int *__restrict__ tblk) {
  if constexpr (K < PM) {
    if (K < X.m) {
      tri1_step<K>(X, C, sN, ok_all, W, Dt, D6, tsrc, tblk);
      tri1_steps<K + 1>(X, C, sN, ok_all, W, Dt, D6, tsrc, tblk);
    }
  }
}
__device__ __forceinline__ void tri1_body(const DevPlan &P, const double *__restrict__ Hblk, double *__restrict__ Lv, int pn0,
                                          const double *__restrict__ lambda_p, int *__restrict__ fail_flag) {
  __shared__ __attribute__((aligned(16))) double W[TRI1_NR * 6];   // column image: row i at W + 6 i
  __shared__ __attribute__((aligned(16))) double Dt[NJMAX * 256];  // diagonal tiles, row-major
  __shared__ __attribute__((aligned(16))) double D6[36];
  __shared__ int tsrc[PM * PM], tblk[PM * PM];
  const int pn = !P.task_dirty ? P.pp.tri_order[pn0 + blockIdx.x] : pn0 + (int)blockIdx.x;      // (full sweep: panels in width order)
  const PanelDesc dsc = P.pp.pdesc[pn];
  if (!task_runs(P, dsc.task)) return;
  Tri1Ctx X;
  X.Hblk = Hblk; X.Lv = Lv; X.zero_blk = P.zero_blk;
  X.m = dsc.m; X.n = 6 * dsc.m; X.nJ = (X.n + 15) >> 4;
  X.lane = threadIdx.x; X.nn = X.lane & 15; X.q = X.lane >> 4;
  X.lambda = *lambda_p;
  X.tp = P.pp.ptop + (int64_t)dsc.top * 256;
  const int lane = X.lane, n = X.n, nJ = X.nJ;
#pragma unroll
  for (int e = 0; e < PM * PM / 64; ++e) {
    tsrc[lane + 64 * e] = P.pp.ptri_src[(int64_t)pn * PM * PM + lane + 64 * e];
    tblk[lane + 64 * e] = P.pp.ptri_blk[(int64_t)pn * PM * PM + lane + 64 * e];
  }
  for (int e = lane; e < NJMAX * 256; e += 64) {                    // zero above the diagonal, identity on the padding
    const int i = (e >> 4) & 15, j = e & 15, J = e >> 8;
    Dt[e] = (i == j && 16 * J + i >= n) ? 1.0 : 0.0;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {                                     // the lane's scalar rows: i = lane and (lanes 0 .. 31) i = 64 + lane
    const int i = lane + 64 * h;
    X.rv[h] = i < n; X.rpad[h] = i < 16 * nJ && i < TRI1_NR;
    X.rr[h] = i / 6; X.rho[h] = i - 6 * X.rr[h];
  }
  __builtin_amdgcn_wave_barrier();
  d4_t C[NJMAX * (NJMAX + 1) / 2];
#pragma unroll
  for (int p = 0; p < NJMAX * (NJMAX + 1) / 2; ++p) C[p] = d4_t{0.0, 0.0, 0.0, 0.0};
  Row6 sN[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    sN[h] = Row6{{0, 0, 0, 0, 0, 0}};
    if (X.rv[h]) sN[h] = load_row(tri1_src_row(X, tsrc, h, 0));
  }
  bool ok_all = true;
  tri1_steps<0>(X, C, sN, ok_all, W, Dt, D6, tsrc, tblk);
  if (!ok_all && lane == 0) atomicOr(fail_flag, 1);
  __builtin_amdgcn_wave_barrier();
  // ---- inverses of the diagonal tiles: lane (J, c) computes column c of tile J's inverse (right-looking substitution)
#pragma unroll
  for (int pass = 0; pass < (NJMAX + 3) / 4; ++pass) {
    const int J = 4 * pass + X.q, c = X.nn;
    if (J < nJ) {
      const double *__restrict__ D = &Dt[J * 256];
      double xc[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) xc[i] = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        xc[i] *= 1.0 / D[i * 17];
#pragma unroll
        for (int i2 = 0; i2 < 16; ++i2) if (i2 > i) xc[i2] = fma(-D[i2 * 16 + i], xc[i], xc[i2]);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) X.tp[(NLT + J) * 256 + 16 * c + i] = xc[i];
    }
  }
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_panel_tri1(DevPlan P, const double *__restrict__ Hblk, double *__restrict__ Lv, int pn0,
                                                   const double *__restrict__ lambda_p, int *__restrict__ fail_flag) {
  tri1_body(P, Hblk, Lv, pn0, lambda_p, fail_flag);
}

// Rider role of a k_panel_rows launch of a narrow level (one wave per workgroup): the wave's 10 lane groups stride one item.
__device__ __forceinline__ void ride_item_wave(const DevPlan &P, const double *__restrict__ Hblk, double *__restrict__ Lv,
                                               const double *__restrict__ lambda_p, int item, double *__restrict__ tile) {
  const RideItem it = P.ride_items[item];
  if (P.task_dirty && !P.task_dirty[it.task]) return;
  const int lane = threadIdx.x;
  const int g = lane / 6, r = lane - 6 * g;
  if (lane < 60) {
    Row6 acc = {{0, 0, 0, 0, 0, 0}};
    if (g == 0) acc = it.first ? load_A_row(P, Hblk, it.t, r, *lambda_p) : load_row(Lv + 36 * (int64_t)it.t + 6 * r);
    apply_ops(P, Lv, acc, g, r, it.o0 + g, it.o0 + it.n, 10, tile);
#pragma unroll
    for (int c = 0; c < 6; ++c) tile[6 * lane + c] = acc.v[c];
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < 36) {
    double sum = 0;
#pragma unroll
    for (int q = 0; q < 10; ++q) sum += tile[q * 36 + lane];
    Lv[36 * (int64_t)it.t + lane] = sum;
  }
}

// Off-triangle rows of a panel: X <- U T^-T for all rows at once, done as the transposed problem
// Y = T^-1 U^T on 16-wide tiles with v_mfma_f64_16x16x4_f64: one wave owns ROW_SETS x 16 scalar rows (the N dimension),
// Y_J = Dinv_J (U^T_J - sum_{I<J} T_JI Y_I).  The f64 MFMA result layout (row = (lane >> 4) + 4 reg) makes the
// result tile Y_I directly usable as the B operand of the next products, so the 6 tiles never leave registers; the
// A operands stream from the panel's operand buffer (written by k_panel_tri), one coalesced 512-byte load each.
// With x != nullptr the right-hand side rides along as scalar row R6 of the panel (x holds b - external sums for
// the panel's columns, left there by fwd_ext_column): the in-panel forward substitution costs nothing extra.
template <bool BYC = false>
__device__ __forceinline__ void panel_rows_body(const DevPlan &P, const double *__restrict__ Hblk, double *__restrict__ Lv, int chunk0,
                                                double *__restrict__ x, int n_chunks, const double *__restrict__ lambda_p, int ride0) {
  if ((int)blockIdx.x >= n_chunks) {                               // riders (symbolic.cpp)
    __shared__ __attribute__((aligned(16))) double ride_tile[360];
    ride_item_wave(P, Hblk, Lv, lambda_p, ride0 + (int)blockIdx.x - n_chunks, ride_tile);
    return;
  }
  const int ci = chunk0 + xcd_contiguous(blockIdx.x, n_chunks);
  const RowChunk rc = P.pp.rchunks[ci];
  const int lane = threadIdx.x, nn = lane & 15, q = lane >> 4;
  // BYC (narrow levels, 16-column panels): the source codes of this lane's scalar row from the table laid out by chunk -- addressed without the
  // descriptor, so both requests travel together (structure_upload.cpp "rchunk_src")
  int scq[4 * NJMAX];
  if constexpr (BYC) {
    const int *__restrict__ rsq = P.pp.rchunk_src + ((int64_t)(ci - P.pp.rchunk_src0) * 16 + nn) * PANEL_MAX;
#pragma unroll
    for (int e = 0; e < 4 * NJMAX; ++e) scq[e] = rsq[(16 * (e >> 2) + q + 4 * (e & 3)) / 6];
  }
  if (!task_runs(P, rc.task)) return;
  const int m = rc.m;
  const int n = 6 * m, nJ = (n + 15) >> 4;
  const int R6 = rc.R6;
  const int *__restrict__ cols = P.task_cols + rc.cols0;
  const double *__restrict__ tp = P.pp.ptop + (int64_t)rc.top * 256;
  constexpr int RS = ROW_SETS;                                   // sets of 16 scalar rows handled by this wave
  constexpr int NE = 4 * NJMAX;                                  // elements of U^T per lane and set: NJMAX tiles x 4 registers
  // gather U^T in MFMA C layout: (lane, J, r) <-> scalar column c = 16 J + (lane >> 4) + 4 r of scalar row s.
  // Two memory round trips in all: the source codes, then the values (branch-free; absent -> the zero block).
  int sc[RS][NE], rho[RS];
  int64_t rowoff[RS];
  bool valid[RS], rhs[RS];
#pragma unroll
  for (int u = 0; u < RS; ++u) {
    const int s = rc.s0 + 16 * u + nn;                           // scalar row within the panel's off-triangle rows
    valid[u] = s < R6;
    rhs[u] = x != nullptr && s == R6;
    const int br = valid[u] ? s / 6 : 0;
    rho[u] = valid[u] ? s - 6 * br : 0;
    rowoff[u] = (int64_t)(rc.prow0 + br) * PM;
    const int *__restrict__ rs = P.pp.prow_src + rowoff[u];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int c = 16 * (e >> 2) + q + 4 * (e & 3);
      if constexpr (BYC) sc[u][e] = ((valid[u] || rhs[u]) && c < n) ? scq[e] : -1;
      else sc[u][e] = (valid[u] && c < n) ? rs[c / 6] : ((rhs[u] && c < n) ? cols[c / 6] : -1);
    }
  }
  d4_t Y[RS][NJMAX];
#pragma unroll
  for (int u = 0; u < RS; ++u)
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int c = 16 * (e >> 2) + q + 4 * (e & 3);
      const int k = c / 6;
      const int code = sc[u][e];
      const double *base = code >= 0 ? Lv + 36 * (int64_t)code : (code <= -2 ? Hblk + 36 * (int64_t)(-2 - code) : Lv + 36 * (int64_t)P.zero_blk);
      if (rhs[u] && c < n) base = x + 6 * (int64_t)code;      // rho == 0 on this lane
      Y[u][e >> 2][e & 3] = base[6 * rho[u] + (c - 6 * k)];
    }
  // operand tiles stream in one tile row ahead of the MFMAs that use them (tile row J: J negated lower tiles + its
  // inverted diagonal tile = 4 (J + 1) doubles per lane); every tile feeds the MFMAs of all RS row sets
  auto load_tile_row = [&](int J, double (&A)[4 * NJMAX]) {
#pragma unroll
    for (int I = 0; I < NJMAX; ++I)
      if (I < J) {
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) A[4 * I + kc] = tp[((J * (J - 1) / 2 + I) * 4 + kc) * 64 + lane];
      }
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) A[4 * (NJMAX - 1) + kc] = tp[((NLT + J) * 4 + kc) * 64 + lane];   // slot NJMAX-1 is never a lower tile of row J <= NJMAX-1
  };
  double Abuf[2][4 * NJMAX];
  load_tile_row(0, Abuf[0]);
#pragma unroll
  for (int J = 0; J < NJMAX; ++J)
    if (J < nJ) {
      double (&A)[4 * NJMAX] = Abuf[J & 1];
      if (J + 1 < nJ) load_tile_row(J + 1, Abuf[(J + 1) & 1]);
#pragma unroll
      for (int u = 0; u < RS; ++u) {
        d4_t acc = Y[u][J];
#pragma unroll
        for (int I = 0; I < J; ++I)
#pragma unroll
          for (int kc = 0; kc < 4; ++kc)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[4 * I + kc], Y[u][I][kc], acc, 0, 0, 0);
        d4_t z = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) z = __builtin_amdgcn_mfma_f64_16x16x4f64(A[4 * (NJMAX - 1) + kc], acc[kc], z, 0, 0, 0);
        Y[u][J] = z;
      }
    }
#pragma unroll
  for (int u = 0; u < RS; ++u) {
    const int *__restrict__ rb = P.pp.prow_blk + rowoff[u];
    int tt[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int c = 16 * (e >> 2) + q + 4 * (e & 3);
      tt[e] = (valid[u] && c < n) ? rb[c / 6] : -1;
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int c = 16 * (e >> 2) + q + 4 * (e & 3);
      if (tt[e] >= 0) Lv[36 * (int64_t)tt[e] + 6 * rho[u] + (c - 6 * (c / 6))] = Y[u][e >> 2][e & 3];
      if (rhs[u] && c < n) x[6 * (int64_t)sc[u][e] + (c - 6 * (c / 6))] = Y[u][e >> 2][e & 3];
    }
  }
}

__global__ __launch_bounds__(64) void k_panel_rows(DevPlan P, const double *__restrict__ Hblk, double *__restrict__ Lv, int chunk0,
                                                   double *__restrict__ x, int n_chunks, const double *__restrict__ lambda_p, int ride0) {
  panel_rows_body<false>(P, Hblk, Lv, chunk0, x, n_chunks, lambda_p, ride0);
}
__global__ __launch_bounds__(64) void k_panel_rows_byc(DevPlan P, const double *__restrict__ Hblk, double *__restrict__ Lv, int chunk0,
                                                       double *__restrict__ x, int n_chunks, const double *__restrict__ lambda_p, int ride0) {
  panel_rows_body<true>(P, Hblk, Lv, chunk0, x, n_chunks, lambda_p, ride0);
}

// ---- multi-GPU: a rank's contribution to the top of the factor.  One lane group per top block t (row per lane, 10
// blocks per wave):  L[t] = H_partial[t] (+ lambda on the designated rank's diagonal blocks) - sum over the updates whose
// source column lies in THIS rank's domain.  After the all-reduce over the ranks L[t] holds A[t] minus every
// domain-sourced update; the top-sourced updates follow in the ordinary kernels (k_chol_acc from top_ext0, the panels).
__global__ __launch_bounds__(64) void k_dist_acc(DevPlan P, const double *__restrict__ Hblk, double *__restrict__ Lv,
                                                 const double *__restrict__ lambda_p) {
  __shared__ __attribute__((aligned(16))) double tile[360];
  const int lane = threadIdx.x, g = lane / 6, r = lane - 6 * g;
  const int64_t q = (int64_t)blockIdx.x * 10 + g;
  const int64_t nq = (int64_t)P.zero_blk - P.top_blk0;                 // zero_blk == nnzL
  const bool on = lane < 60 && q < nq;
  Row6 acc = {{0, 0, 0, 0, 0, 0}};
  const int64_t t = P.top_blk0 + (on ? q : 0);
  if (on) {
    const int a = P.asrc[t];
    if (a >= 0) {
      acc = load_row(Hblk + 36 * (int64_t)a + 6 * r);
      if (a < P.nb && P.lambda_rank) {
        const double lambda = *lambda_p;
#pragma unroll
        for (int c = 0; c < 6; ++c) acc.v[c] += (c == r) ? lambda : 0.0;
      }
    }
  }
  apply_ops(P, Lv, acc, g, r, on ? P.own_op0[q] : 0, on ? P.own_op1[q] : 0, 1, tile);
  if (on) store_row(Lv + 36 * t + 6 * r, acc);
}
// ... and to the right-hand side of the top columns: x_k = b_partial_k - sum_{j in this rank's domain} L_kj y_j
// (one wave per top column)
// (bfull: landmark elimination in distributed mode -- bvec is this rank's REDUCED gradient b - sum over ITS landmarks, b the completed
//  gradient of the top; b itself is counted on one rank, the landmark terms (bvec - bfull) on every rank)
__global__ __launch_bounds__(64) void k_dist_rhs(DevPlan P, const double *__restrict__ Lv, const double *__restrict__ bvec, double *__restrict__ x,
                                                 const double *__restrict__ bfull) {
  __shared__ double sred[60];
  const int kq = blockIdx.x, k = P.top_col0 + kq;
  const int lane = threadIdx.x, g = lane / 6, r = lane - 6 * g;
  const int64_t e0 = P.own_row0[kq], e1 = P.own_row1[kq];
  double acc = 0;
  if (lane < 60) {
    for (int64_t e = e0 + g; e < e1; e += 40) {
      int bi[4], ci[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t ee = e + 10 * q;
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
    sred[lane] = acc;
  }
  __syncthreads();
  if (lane < 6) {
    double sv = P.lambda_rank ? bvec[6 * (int64_t)k + lane] : (bfull ? bvec[6 * (int64_t)k + lane] - bfull[6 * (int64_t)k + lane] : 0.0);    // b of the top was completed after the linearisation: counted once
    for (int q = 0; q < 10; ++q) sv -= sred[q * 6 + lane];
    x[6 * (int64_t)k + lane] = sv;
  }
}

// per-device kernel attributes (called from the structure build, with the context's device current): the leaf kernel
// keeps a sub-tree's blocks and op lists in up to ~78 KB of dynamic LDS, above the 64 KB that need no opt-in.  Once per
// device and under a lock: re-setting the attribute while another host thread launches the kernel made launches fail
// (two contexts driven from two threads: tests/test_gpu_shard.py).
void prepare_device_kernels() {
  static std::mutex mu;
  static std::vector<char> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return;
  std::lock_guard<std::mutex> lock(mu);
  if ((int)done.size() <= dev) done.resize(dev + 1, 0);
  if (done[dev]) return;
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_chol_leaf<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  done[dev] = 1;
}

// ---- the index ranges of level l that one sweep launches.  The lists of a level are in task order (PartialSweep, device_plan.hpp), so
// a partial sweep takes a sub-range of each; the kernels and their template choices are those of the full sweep either way.
struct LevelRange {
  bool nothing_dirty;          // partial sweep without a dirty task in the level: only the riders of its launches run
  int64_t sf, sn;              // short-list accumulate targets: first, count
  int64_t lf; int n_long;      // long-list targets: first, count
  int n_acc_wg;                // workgroups of the short targets, padded to a multiple of 8 when long targets follow (padding workgroups find idx >= count and idle)
  bool fw_table;               // forward-role work items come from the work-item table (a level with split rows) ...
  int col0, n_fwd_wg;          // ... col0 = -1 - first table entry; else first entry of task_cols; count (0: no fused forward solve here)
  int64_t g2f; int n_g2;       // column groups: first, count
  int t0, nt, pn0;             // tasks: first, count; first panel (the panels of a level are numbered in task order)
  int c0, nc;                  // row chunks of a panel level: first, count
};
static LevelRange level_range(const HostSchedule &H, const PartialSweep *ps, int l, bool fwd) {
  LevelRange R{};
  const int64_t a0 = H.acc_ptr[l], am = H.acc_mid[l], a1 = H.acc_ptr[l + 1];
  const int t0f = H.level_ptr[l], ntf = H.level_ptr[l + 1] - t0f;
  const bool panel = H.level_panel[l];
  const int n_g2_full = H.g2_lvl.empty() ? 0 : (int)(H.g2_lvl[l + 1] - H.g2_lvl[l]);
  const int64_t g2_first = H.g2_lvl.empty() ? 0 : H.g2_lvl[l];
  // forward-solve work items of the level: its panel columns, or (a level with long rows) the entries of the work-item table
  R.fw_table = H.fwg_ptr[l + 1] - H.fwg_ptr[l] != H.level_col_ptr[l + 1] - H.level_col_ptr[l];
  R.col0 = R.fw_table ? -1 - H.fwg_ptr[l] : H.level_col_ptr[l];
  const int n_fwd_full = (fwd && panel) ? (R.fw_table ? H.fwg_ptr[l + 1] - H.fwg_ptr[l] : H.level_col_ptr[l + 1] - H.level_col_ptr[l]) : 0;
  const int ta = ps ? ps->t_lo[l] : 0, tb = ps ? ps->t_hi[l] : -1;
  R.nothing_dirty = ps && tb < ta;
  if (!ps) {
    // full sweep: every list of the level, whole
    R.sf = a0; R.sn = am - a0;
    R.lf = am; R.n_long = (int)(a1 - am);
    R.n_fwd_wg = n_fwd_full;
    R.g2f = g2_first; R.n_g2 = n_g2_full;
    R.t0 = t0f; R.nt = ntf;
    if (panel) { R.c0 = H.rchunk_ptr[l]; R.nc = H.rchunk_ptr[l + 1] - H.rchunk_ptr[l]; }
  } else if (R.nothing_dirty) {
    // partial sweep, nothing dirty in the level: the full sweep's first indices, every count zero
    R.sf = a0; R.sn = 0;
    R.lf = am; R.n_long = 0;
    R.n_fwd_wg = 0;
    R.g2f = g2_first; R.n_g2 = 0;
    R.t0 = t0f; R.nt = 0;
    if (panel) { R.c0 = H.rchunk_ptr[l]; R.nc = 0; }
  } else {
    // partial sweep, the tasks [ta, tb] cover the level's dirty ones: from the first index of ta to the end of tb in every list
    R.sf = ps->s0[ta]; R.sn = ps->s1[tb] - ps->s0[ta];
    R.lf = ps->l0[ta]; R.n_long = (int)(ps->l1[tb] - ps->l0[ta]);
    R.n_fwd_wg = n_fwd_full;                                 // (the work-item table is launched whole: its workgroups look their task's flag up)
    if (n_fwd_full > 0 && !R.fw_table) { R.col0 = ps->task_ptr[ta]; R.n_fwd_wg = ps->task_ptr[tb + 1] - ps->task_ptr[ta]; }
    if (n_g2_full == 0) { R.g2f = g2_first; R.n_g2 = 0; }
    else { R.g2f = ps->g0[ta]; R.n_g2 = ps->g1[tb] - ps->g0[ta]; }
    R.t0 = ta; R.nt = tb - ta + 1;
    if (panel) { R.c0 = ps->c0[ta]; R.nc = ps->c1[tb] - ps->c0[ta]; }
  }
  R.n_acc_wg = R.n_long > 0 ? (cdiv(R.sn, 10) + 7) & ~7 : cdiv(R.sn, 10);
  R.pn0 = panel ? H.level_pn0[l] + (R.t0 - t0f) : 0;
  return R;
}

// With b / x given the forward solve L y = b is fused into the sweep (x <- y): a level's right-hand side is one
// more row of its columns, so its external sums ride in the accumulate launch and the in-panel substitution in the
// row kernel; non-panel levels run the generic forward kernel right after their factor kernel.
void launch_factor(const DevPlan &P, const HostSchedule &H, const double *Hblk, double *Lv, const double *lambda_p,
                   int *fail_flag, hipStream_t s, const double *b, double *x, int phase, const PartialSweep *ps, const double *b_full, LaunchCensus *cz) {
  // (partial sweep, P.task_dirty set: the caller has prepared x = b on the dirty columns and the saved y elsewhere)
  if (x && phase != PHASE_TOP && !P.task_dirty && !cz) launch_copy_vec(b, x, (int64_t)P.top_col0 * 6, s);   // (the top of x is written by k_dist_rhs when distributed)
  if (cz) { cz->level_riders.assign((size_t)H.n_levels, 0); cz->level_long.assign((size_t)H.n_levels, 0); cz->level_fwd.assign((size_t)H.n_levels, 0); cz->level_fwtab.assign((size_t)H.n_levels, 0); }
  for (int l = 0; l < H.n_levels; ++l) {
    if (!seg_runs(H, l, phase)) continue;
    const LevelRange R = level_range(H, ps, l, x != nullptr);
    const int grid = R.n_acc_wg + R.n_long + R.n_fwd_wg, grid2 = R.n_g2 + R.n_fwd_wg;
    if (cz) { cz->level_fwd[(size_t)l] = R.n_fwd_wg; cz->level_fwtab[(size_t)l] = (R.fw_table && R.n_fwd_wg > 0) ? 1 : 0; }
    const LaunchForm acc = select_acc(H, l);
    const bool acc_g2 = acc == LF_ACC2_8 || acc == LF_ACC2_4 || acc == LF_ACC2_1;
    if (cz && !acc_g2 && grid > 0) cz->level_long[(size_t)l] = R.n_long;
    if (acc_g2 ? grid2 > 0 : grid > 0)
      switch (acc) {
        case LF_ACC2_8: FGO_LAUNCH_N(cz, acc, grid2, R.n_g2, k_chol_acc2<8>, dim3(grid2), dim3(512), 0, s, P, Hblk, Lv, Lv, R.g2f, R.n_g2, lambda_p, x, R.col0); break;
        case LF_ACC2_4: FGO_LAUNCH_N(cz, acc, grid2, R.n_g2, k_chol_acc2<4>, dim3(grid2), dim3(256), 0, s, P, Hblk, Lv, Lv, R.g2f, R.n_g2, lambda_p, x, R.col0); break;
        case LF_ACC2_1: FGO_LAUNCH_N(cz, acc, grid2, R.n_g2, k_chol_acc2<1>, dim3(grid2), dim3(64), 0, s, P, Hblk, Lv, Lv, R.g2f, R.n_g2, lambda_p, x, R.col0); break;
        case LF_ACC8: FGO_LAUNCH_N(cz, acc, grid, R.sn + R.n_long, k_chol_acc<8>, dim3(grid), dim3(512), 0, s, P, Hblk, Lv, R.sf, R.sn, lambda_p, x, R.n_acc_wg, R.col0, R.n_long, R.lf); break;
        case LF_ACC4: FGO_LAUNCH_N(cz, acc, grid, R.sn + R.n_long, k_chol_acc<4>, dim3(grid), dim3(256), 0, s, P, Hblk, Lv, R.sf, R.sn, lambda_p, x, R.n_acc_wg, R.col0, R.n_long, R.lf); break;
        case LF_ACC2: FGO_LAUNCH_N(cz, acc, grid, R.sn + R.n_long, k_chol_acc<2>, dim3(grid), dim3(128), 0, s, P, Hblk, Lv, R.sf, R.sn, lambda_p, x, R.n_acc_wg, R.col0, R.n_long, R.lf); break;
        default: FGO_LAUNCH_N(cz, LF_ACC1, grid, R.sn + R.n_long, k_chol_acc<1>, dim3(grid), dim3(64), 0, s, P, Hblk, Lv, R.sf, R.sn, lambda_p, x, R.n_acc_wg, R.col0, R.n_long, R.lf); break;
      }
    if (x && H.level_panel[l] && !H.fsplit_ptr.empty() && H.fsplit_ptr[l + 1] > H.fsplit_ptr[l] && !R.nothing_dirty)
      FGO_LAUNCH(cz, LF_FWD_COMBINE, H.fsplit_ptr[l + 1] - H.fsplit_ptr[l], k_fwd_combine, dim3(H.fsplit_ptr[l + 1] - H.fsplit_ptr[l]), dim3(64), 0, s, P, x, H.fsplit_ptr[l]);
    const int t0 = R.t0, nt = R.nt;
    if (H.level_panel[l]) {
      switch (select_tri(H, l)) {
        case LF_TRI1:
          if (nt > 0) FGO_LAUNCH(cz, LF_TRI1, nt, k_panel_tri1, dim3(nt), dim3(64), 0, s, P, Hblk, Lv, R.pn0, lambda_p, fail_flag);
          break;
        case LF_TRI8:
          if (nt > 0) FGO_LAUNCH(cz, LF_TRI8, nt, (k_panel_tri<8>), dim3(nt), dim3(8 * 64), 0, s, P, Hblk, Lv, R.pn0, lambda_p, fail_flag, nt, 0, 0, nt);
          break;
        default: {
          constexpr int TRI_NW = 16;                                          // the latency form: 16 waves per panel, riders behind the panels
          const int r0 = H.ride_ptr.empty() ? 0 : H.ride_ptr[2 * l], nr = H.ride_ptr.empty() ? 0 : H.ride_ptr[2 * l + 1] - r0;
          const int ntp = (nr > 0 && P.ride_xcd) ? (nt + 7) & ~7 : nt;      // riders start at a multiple of 8: XCD = (blockIdx - ntp) & 7
          if (ntp + nr > 0) {
            if (cz) cz->level_riders[(size_t)l] += nr;
            FGO_LAUNCH(cz, LF_TRI16, ntp + (nr + RIDE_PER_WG - 1) / RIDE_PER_WG, (k_panel_tri<TRI_NW>), dim3(ntp + (nr + RIDE_PER_WG - 1) / RIDE_PER_WG), dim3(TRI_NW * 64), 0, s, P, Hblk, Lv, R.pn0, lambda_p, fail_flag, ntp, r0, nr, nt);
          }
        }
      }
      const int q0 = H.ride_ptr.empty() ? 0 : H.ride_ptr[2 * l + 1], nq = H.ride_ptr.empty() ? 0 : H.ride_ptr[2 * l + 2] - q0;   // riders of the row launch
      if (R.nc + nq > 0) {
        if (cz) cz->level_riders[(size_t)l] += nq;
        if (select_rows(H, l) == LF_ROWS_BYC) FGO_LAUNCH(cz, LF_ROWS_BYC, R.nc + nq, k_panel_rows_byc, dim3(R.nc + nq), dim3(64), 0, s, P, Hblk, Lv, R.c0, x, R.nc, lambda_p, q0);
        else FGO_LAUNCH(cz, LF_ROWS, R.nc + nq, k_panel_rows, dim3(R.nc + nq), dim3(64), 0, s, P, Hblk, Lv, R.c0, x, R.nc, lambda_p, q0);
      }
      continue;
    }
    if (nt <= 0) continue;                              // (partial sweep: nothing dirty in this level)
    const LaunchForm fact = select_fact(H, l);
    switch (fact) {
      case LF_LEAF4: {
        const int lb = H.level_leaf_maxblk[l], lc = H.level_maxtaskcols[l];
        const size_t lds = ((size_t)lb + 1) * 36 * sizeof(double) + (size_t)12 * lc * sizeof(double) + ((size_t)lb + 2 + lc + 2) * sizeof(int) +
                           ((size_t)lb + 2) * sizeof(unsigned short) + (size_t)H.level_leaf_maxops[l] * sizeof(unsigned);
        FGO_LAUNCH(cz, LF_LEAF4, nt, (k_chol_leaf<4>), dim3(nt), dim3(256), lds, s, P, Hblk, Lv, t0, lambda_p, fail_flag, lb, lc, x);
        break;                                          // (the forward solve of a leaf level is part of the kernel)
      }
      case LF_FACT_1_2: FGO_LAUNCH(cz, fact, nt, (k_chol_fact<1, 2>), dim3(nt), dim3(64), 0, s, P, Hblk, Lv, t0, lambda_p, fail_flag); break;
      case LF_FACT_1_3: FGO_LAUNCH(cz, fact, nt, (k_chol_fact<1, 3>), dim3(nt), dim3(64), 0, s, P, Hblk, Lv, t0, lambda_p, fail_flag); break;
      case LF_FACT_4_3: FGO_LAUNCH(cz, fact, nt, (k_chol_fact<4, 3>), dim3(nt), dim3(256), 0, s, P, Hblk, Lv, t0, lambda_p, fail_flag); break;
      case LF_FACT_8_3: FGO_LAUNCH(cz, fact, nt, (k_chol_fact<8, 3>), dim3(nt), dim3(512), 0, s, P, Hblk, Lv, t0, lambda_p, fail_flag); break;
      default: FGO_LAUNCH(cz, LF_FACT_16_2, nt, (k_chol_fact<16, 2>), dim3(nt), dim3(1024), 0, s, P, Hblk, Lv, t0, lambda_p, fail_flag); break;
    }
    if (x && fact != LF_LEAF4) launch_fwd_level(P, H, Lv, x, l, s, cz);
  }
  if (phase == PHASE_DOMAIN && !cz) {
    // this rank's contributions to the top: every block of the top columns, and (forward solve fused) their right-hand side
    if (H.n_top_blocks > 0) hipLaunchKernelGGL(k_dist_acc, dim3(cdiv(H.n_top_blocks, 10)), dim3(64), 0, s, P, Hblk, Lv, lambda_p);
    if (x && H.n_top_cols > 0) hipLaunchKernelGGL(k_dist_rhs, dim3(H.n_top_cols), dim3(64), 0, s, P, Lv, b, x, b_full);
  }
}

}  // namespace fgo
