// Cluster filtering and floor removal of a point cloud on the MI355X (gfx950, 64-bit integers, wave64): the program that ends the
// reference's run, mapping/pcd_filter.cpp -- clusterFilter(0.03, ...) = pcl::EuclideanClusterExtraction with setMinClusterSize(200),
// then remove_floor_pt -- in ONE call.  include/fgo.h states the semantics (this project's: integer distances on the 2^-20 m quantum,
// clusters numbered by their smallest member), tests/map_clean_reference.py restates them in numpy.
//
//   quantise  one lane per point: Q = llrint(x 2^20), the cell c = floor(Q / T) and its key, or the out-of-range mark.  Contraction
//             is switched off for these lines; from there on everything is integer.
//   index     map_cell_index.hip, shared with kernels_map_normals.hip: the stable sort of the (cell key, input index) pairs and the
//             gather of the quantised coordinates into sorted order, which counts the run heads.  A cell's run is found by binary
//             search of the sorted keys (map_cells_device.hpp, as are the quantisation, the floor division and the key).  An
//             open-addressing table cell key -> start of the run (64-bit atomicCAS on the key, two slots per point) was built and
//             measured as well: 5 % faster on a map of 44 000 points, 11 % slower on a sheet of 2 000 000, 24 to 48 more bytes per
//             point; it is not kept (the figures of both: profiles/NOTES.md).
//   link      one lane per point in sorted order: it walks back over the points of its own cell that precede it and over the 13
//             neighbour cells that precede its cell in key order -- every pair of points within reach is visited once -- applies
//             dQ.dQ <= T^2 and unites the two points' sets in a lock-free union-find over the input indices.
//             INVARIANT: parent[i] <= i.  A root is only ever hooked under a SMALLER root, by atomicCAS(&parent[r], r, s) with
//             s < r, and path halving only replaces a parent by an ancestor (atomicMin), so every chain decreases strictly: there
//             is no cycle, find() ends, and the root of a set is its smallest member.  EVERY read of parent[] in this kernel is a
//             relaxed agent-scope atomic load or what a CAS returned: a plain load may be served from a stale L1 line or another
//             XCD's L2, and the retry loop would spin on it.  A CAS that fails means that another lane hooked that root: the loop
//             finds the roots again and retries.  No lane ever waits for another one.
//   flatten   every point walks to its root; the root's size is an integer atomicAdd, one per distinct root of a wave.
//   number    rocPRIM's exclusive scan over "is a root" in input order: the clusters in ascending order of their smallest member.
//   floor     h = up_sign Q_up: its minimum by a reduction over the workgroup and one integer atomicMin, the histogram in LDS and
//             flushed by integer atomicAdd, the most populated bin (the lowest on a tie) by one workgroup.
//   compact   rocPRIM's exclusive scan of the keep flags, then index and xyz in input order.
// No floating-point atomics anywhere; the only floating-point arithmetic is the quantisation and the one subtraction on output.
// Every barrier is outside every branch that is not uniform over the workgroup: the loops that hold one run over block-uniform
// bounds.  The grids are capped and the kernels stride beyond that.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>
#include <climits>
#include <cmath>
#include <cstring>
#include "../../include/fgo.h"
#include "batch_call.hpp"
#include "map_cell_index.hpp"
#include "map_cells_device.hpp"
#include "small_dense_device.hpp"

namespace fgo {
namespace {

using dev::map_cell_key, dev::MAP_QUANTA_PER_M, dev::MAP_CELL_BIAS, dev::MAP_CELL_EMPTY;      // |c_k| < 2^20; the key of an out-of-range point

constexpr int MC_T = 256;                        // threads of a workgroup
constexpr uint32_t MC_NONE = ~0u;                // no such cell
constexpr int MC_MAX_BINS = 8192;                // floor_span / floor_res <= 4096 gives at most 6145 bins (R = 1, S = 6144)
constexpr unsigned MC_HIST_GRID = 1024;          // workgroups of the histogram: each flushes its bins once

enum { MC_C_OOR, MC_C_CELLS, MC_C_CLUSTERS, MC_C_CLUSTERS_KEPT, MC_C_AFTER, MC_C_HMIN, MC_C_FLOOR_BIN, MC_C_FLOOR_CNT, MC_C_F, MC_C_KEPT,
       MC_C_COUNT };

struct McArgs : dev::MapCellIndex {              // n, Q, sQ, key, skey, idx, sidx
  long long T, T2, R, S, C;
  int min_size, max_size, floor, axis, sign, nbins;
  const double *xyz;
  int32_t *parent;
  uint32_t *size, *flag, *num, *pos, *bins;      // flag: is a root, then: is kept
  long long *cnt;
  int32_t *label, *csize;                        // label holds the root until the clusters are numbered
  uint8_t *reason;
  int64_t *index;
  double *xyz_out;
};

// (lanes are counted by dev::wave_count; the counts that a scan ends on anyway -- clusters, kept points -- are read off the scan)
__global__ __launch_bounds__(MC_T) void k_mc_quantise(McArgs A) {
#pragma clang fp contract(off)
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < A.n; p += stride) {
    bool ok = true;
    long long c[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      long long Q;
      if (dev::map_quantise(A.xyz[3 * p + k], 0x1p62, Q)) {               // 2^62: beyond any cell, and llrint is safe
        const long long q = dev::map_floor_div(Q, A.T);
        if (q <= -MAP_CELL_BIAS || q >= MAP_CELL_BIAS) ok = false;
        c[k] = q;
      } else ok = false;
      A.Q[3 * p + k] = Q;
    }
    A.key[p] = ok ? map_cell_key(c[0] + MAP_CELL_BIAS, c[1] + MAP_CELL_BIAS, c[2] + MAP_CELL_BIAS) : MAP_CELL_EMPTY;
    A.idx[p] = (uint32_t)p;
    A.parent[p] = (int32_t)p;
    A.size[p] = 0;
    if (!ok) dev::wave_count(A.cnt + MC_C_OOR);
  }
}

// the start of the run of `key` in sorted order, or MC_NONE
__device__ inline uint32_t mc_lookup(const McArgs &A, unsigned long long key) {
  const int64_t lo = dev::map_key_lower_bound(A.skey, A.n, key);                        // the first s with skey[s] >= key
  return lo < A.n && A.skey[lo] == key ? (uint32_t)lo : MC_NONE;
}

__device__ inline int32_t mc_parent(const int32_t *parent, int32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x, halving the path on the way: parent[x] becomes its grandparent, an ancestor still, and never grows
__device__ inline int32_t mc_find(int32_t *parent, int32_t x) {
  int32_t p = mc_parent(parent, x);
  while (p != x) {
    const int32_t g = mc_parent(parent, p);
    if (g != p) atomicMin(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

__device__ inline void mc_unite(int32_t *parent, int32_t a, int32_t b) {
  for (;;) {
    a = mc_find(parent, a);
    b = mc_find(parent, b);
    if (a == b) return;
    if (a < b) { const int32_t t = a; a = b; b = t; }
    if (atomicCAS(parent + a, a, b) == a) return;                 // the larger root under the smaller; else another lane hooked a
  }
}

__global__ __launch_bounds__(MC_T) void k_mc_link(McArgs A) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t s = (int64_t)blockIdx.x * MC_T + threadIdx.x; s < A.n; s += stride) {
    const unsigned long long key = A.skey[s];
    if (key == MAP_CELL_EMPTY) continue;
    const long long q0 = A.sQ[3 * s], q1 = A.sQ[3 * s + 1], q2 = A.sQ[3 * s + 2];
    const int32_t p = (int32_t)A.sidx[s];
    auto visit = [&](int64_t j) {
      const long long d0 = A.sQ[3 * j] - q0, d1 = A.sQ[3 * j + 1] - q1, d2 = A.sQ[3 * j + 2] - q2;
      if (d0 * d0 + d1 * d1 + d2 * d2 <= A.T2) mc_unite(A.parent, p, (int32_t)A.sidx[j]);
    };
    for (int64_t j = s - 1; j >= 0 && A.skey[j] == key; --j) visit(j);         // its own cell: the points before it
    const long long c[3] = {dev::map_cell_coord(key, 0), dev::map_cell_coord(key, 1), dev::map_cell_coord(key, 2)};      // c_k + 2^20
    for (int t = 0; t < 13; ++t) {                                             // the neighbour cells before its own in key order
      const long long e[3] = {c[0] + t % 3 - 1, c[1] + (t / 3) % 3 - 1, c[2] + t / 9 - 1};
      if (e[0] < 1 || e[1] < 1 || e[2] < 1 || e[0] >= 2 * MAP_CELL_BIAS || e[1] >= 2 * MAP_CELL_BIAS || e[2] >= 2 * MAP_CELL_BIAS) continue;   // no such cell
      const unsigned long long nkey = map_cell_key(e[0], e[1], e[2]);
      const uint32_t j0 = mc_lookup(A, nkey);
      if (j0 == MC_NONE) continue;
      for (int64_t j = j0; j < A.n && A.skey[j] == nkey; ++j) visit(j);
    }
  }
}

// root of every point; one atomicAdd on the root's size per distinct root of a wave
__global__ __launch_bounds__(MC_T) void k_mc_flatten(McArgs A) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * MC_T; base < A.n; base += (int64_t)gridDim.x * MC_T) {       // uniform over the workgroup
    const int64_t p = base + threadIdx.x;
    bool todo = p < A.n && A.key[p] != MAP_CELL_EMPTY;
    int32_t r = -1;
    if (todo) {
      r = mc_find(A.parent, (int32_t)p);
      A.label[p] = r;
    }
    for (unsigned long long m = __ballot(todo); m; m = __ballot(todo)) {
      const int leader = __ffsll((long long)m) - 1;
      const int32_t r0 = __shfl(r, leader);
      const bool mine = todo && r == r0;
      const unsigned long long mm = __ballot(mine);
      if (lane == leader) atomicAdd(&A.size[r0], (uint32_t)__popcll(mm));
      if (mine) todo = false;
    }
  }
}

__device__ inline bool mc_size_ok(const McArgs &A, uint32_t sz) {
  return sz >= (uint32_t)A.min_size && (A.max_size == 0 || sz <= (uint32_t)A.max_size);
}

// "is a root" for the scan; the kept clusters and the points in them, summed over the wave first
__global__ __launch_bounds__(MC_T) void k_mc_roots(McArgs A) {
  for (int64_t base = (int64_t)blockIdx.x * MC_T; base < A.n; base += (int64_t)gridDim.x * MC_T) {       // uniform over the workgroup
    const int64_t p = base + threadIdx.x;
    const bool root = p < A.n && A.key[p] != MAP_CELL_EMPTY && A.label[p] == (int32_t)p;
    if (p < A.n) A.flag[p] = root;
    unsigned long long kept = root && mc_size_ok(A, A.size[p]) ? A.size[p] : 0;
    if (kept) dev::wave_count(A.cnt + MC_C_CLUSTERS_KEPT);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(reinterpret_cast<unsigned long long *>(A.cnt + MC_C_AFTER), kept);
  }
}

// label, cluster size, the mask of the cluster stage (into flag, whose scan num now holds), and the smallest height of what is left;
// the number of clusters is where the scan ended
__global__ __launch_bounds__(MC_T) void k_mc_label(McArgs A) {
  __shared__ long long s_h[MC_T / 64];
  for (int64_t base = (int64_t)blockIdx.x * MC_T; base < A.n; base += (int64_t)gridDim.x * MC_T) {       // uniform over the workgroup
    const int64_t p = base + threadIdx.x;
    long long h = LLONG_MAX;
    if (p < A.n) {
      bool keep = false;
      if (p == A.n - 1) A.cnt[MC_C_CLUSTERS] = (long long)A.num[p] + (A.key[p] != MAP_CELL_EMPTY && A.label[p] == (int32_t)p);
      if (A.key[p] == MAP_CELL_EMPTY) {
        A.label[p] = -1;
        A.reason[p] = 1;
      } else {
        const int32_t r = A.label[p];                              // its root; only p itself reads and writes label[p]
        const uint32_t sz = A.size[r], c = A.num[r];
        A.label[p] = (int32_t)c;
        if (r == (int32_t)p) A.csize[c] = (int32_t)sz;
        keep = mc_size_ok(A, sz);
        A.reason[p] = keep ? 0 : 2;
        if (keep) h = A.sign * A.Q[3 * p + A.axis];
      }
      A.flag[p] = keep;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long other = __shfl_xor(h, o);
      h = other < h ? other : h;
    }
    if ((threadIdx.x & 63) == 0) s_h[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < MC_T / 64; ++w) h = s_h[w] < h ? s_h[w] : h;
      if (h != LLONG_MAX) atomicMin(A.cnt + MC_C_HMIN, h);
    }
    __syncthreads();                                               // the next round writes s_h
  }
}

__global__ __launch_bounds__(MC_T) void k_mc_hist(McArgs A) {
  __shared__ uint32_t s_bin[MC_MAX_BINS];
  for (int b = threadIdx.x; b < A.nbins; b += MC_T) s_bin[b] = 0;
  __syncthreads();
  const long long hmin = A.cnt[MC_C_HMIN];
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < A.n; p += stride) {
    if (!A.flag[p]) continue;
    const long long d = A.sign * A.Q[3 * p + A.axis] - hmin;
    if (d <= A.S) atomicAdd(&s_bin[(d + A.R / 2) / A.R], 1u);       // d >= 0; the bin is below nbins = (S + R div 2) div R + 1
  }
  __syncthreads();
  for (int b = threadIdx.x; b < A.nbins; b += MC_T)
    if (s_bin[b]) atomicAdd(&A.bins[b], s_bin[b]);
}

// one workgroup: the most populated bin, the lowest of them on a tie
__global__ __launch_bounds__(MC_T) void k_mc_floor(McArgs A) {
  __shared__ unsigned long long s_best;
  if (A.cnt[MC_C_AFTER] == 0) return;                              // uniform: nothing is left, floor_bin stays -1
  if (threadIdx.x == 0) s_best = 0;
  __syncthreads();
  unsigned long long best = 0;
  for (int b = threadIdx.x; b < A.nbins; b += MC_T) {
    const unsigned long long v = ((unsigned long long)A.bins[b] << 32) | (unsigned long long)(0xffffffffu - (uint32_t)b);
    best = v > best ? v : best;
  }
  atomicMax(&s_best, best);
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long b = (long long)(0xffffffffu - (uint32_t)(s_best & 0xffffffffu));
    A.cnt[MC_C_FLOOR_BIN] = b;
    A.cnt[MC_C_FLOOR_CNT] = (long long)(s_best >> 32);
    A.cnt[MC_C_F] = A.cnt[MC_C_HMIN] + b * A.R;
  }
}

__global__ __launch_bounds__(MC_T) void k_mc_mask(McArgs A) {
  const bool floor = A.floor && A.cnt[MC_C_FLOOR_BIN] >= 0;
  const long long lim = A.cnt[MC_C_F] + A.C;
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < A.n; p += stride) {
    if (!A.flag[p]) continue;
    if (floor && !(A.sign * A.Q[3 * p + A.axis] > lim)) {
      A.flag[p] = 0;
      A.reason[p] = 3;
    }
  }
}

__global__ __launch_bounds__(MC_T) void k_mc_compact(McArgs A) {
#pragma clang fp contract(off)
  const bool floor = A.floor && A.cnt[MC_C_FLOOR_BIN] >= 0;
  const double lift = (double)A.sign * ((double)A.cnt[MC_C_F] * (1.0 / MAP_QUANTA_PER_M));      // up_sign floor_height: exact
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < A.n; p += stride) {
    if (p == A.n - 1) A.cnt[MC_C_KEPT] = (long long)A.pos[p] + A.flag[p];      // where the scan ended
    if (!A.flag[p]) continue;
    const int64_t o = A.pos[p];
    A.index[o] = p;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double x = A.xyz[3 * p + k];
      A.xyz_out[3 * o + k] = floor && k == A.axis ? x - lift : x;
    }
  }
}

double g_mc_kernel_ms = 0.0;

}  // namespace
}  // namespace fgo

extern "C" double fgo_debug_map_clean_kernel_ms(void) { return fgo::g_mc_kernel_ms; }

extern "C" void fgo_map_clean_params_default(fgo_map_clean_params *p) {
  if (!p) return;
  p->tolerance = 0.03;
  p->min_cluster_size = 200;
  p->max_cluster_size = 0;
  p->remove_floor = 1;
  p->up_axis = 2; p->up_sign = 1;
  p->floor_res = 0.1;
  p->floor_span = 2.0;
  p->floor_clearance = 0.1;
}

extern "C" int fgo_map_clean(int device, int64_t n_points, const double *xyz, const fgo_map_clean_params *params, fgo_map_clean_result *result,
                             int32_t *label_out, uint8_t *reason_out, int32_t *cluster_size_out, int64_t *index_out, double *xyz_out) {
  using namespace fgo;
  fgo_map_clean_params P;
  fgo_map_clean_params_default(&P);
  if (params) P = *params;
  if (!result || n_points < 0 || n_points >= (1ll << 30) || (n_points > 0 && !xyz)) return FGO_EINVAL;
  if (!in_closed(P.tolerance, 1.0 / MAP_QUANTA_PER_M, 256.0)) return FGO_EINVAL;
  if (P.min_cluster_size < 1 || P.max_cluster_size < 0 || (P.max_cluster_size >= 1 && P.max_cluster_size < P.min_cluster_size)) return FGO_EINVAL;
  if (P.up_axis < 0 || P.up_axis > 2 || (P.up_sign != 1 && P.up_sign != -1) || (P.remove_floor != 0 && P.remove_floor != 1)) return FGO_EINVAL;
  McArgs A;
  std::memset(&A, 0, sizeof A);
  A.nbins = 1;
  if (P.remove_floor) {
    if (!in_closed(P.floor_res, 1.0 / MAP_QUANTA_PER_M, 1024.0) || !in_closed(P.floor_span, 0.0, HUGE_VAL) || !(P.floor_span / P.floor_res <= 4096.0))
      return FGO_EINVAL;
    if (!in_closed(P.floor_clearance, 0.0, HUGE_VAL) || P.floor_clearance == HUGE_VAL) return FGO_EINVAL;
    A.R = llrint(P.floor_res * MAP_QUANTA_PER_M);
    A.S = llrint(P.floor_span * MAP_QUANTA_PER_M);
    const double c = P.floor_clearance * MAP_QUANTA_PER_M;
    A.C = c < 0x1p62 ? llrint(c) : (1ll << 62);                                // no height reaches 2^49: beyond that every C acts alike
    const long long nb = (A.S + A.R / 2) / A.R + 1;
    if (nb > MC_MAX_BINS) return FGO_EINVAL;                                    // the bounds above give at most 6145
    A.nbins = (int)nb;
  }
  std::memset(result, 0, sizeof *result);
  result->floor_bin = -1;
  if (n_points == 0) return FGO_OK;
  if (int rc = select_device(device)) return rc;

  const size_t n = (size_t)n_points;
  A.n = n_points;
  A.T = llrint(P.tolerance * MAP_QUANTA_PER_M);
  A.T2 = A.T * A.T;
  A.min_size = P.min_cluster_size; A.max_size = P.max_cluster_size;
  A.floor = P.remove_floor; A.axis = P.up_axis; A.sign = P.up_sign;

  size_t scan_bytes = 0;
  uint32_t *no_val = nullptr;
  if (rocprim::exclusive_scan(nullptr, scan_bytes, no_val, no_val, 0u, n, rocprim::plus<uint32_t>(), 0) != hipSuccess) return FGO_ENUM;
  long long cnt[MC_C_COUNT] = {0};
  cnt[MC_C_HMIN] = LLONG_MAX;
  cnt[MC_C_FLOOR_BIN] = -1;
  Staged S;
  const int h_xyz = S.in(xyz, 3 * n * sizeof(double)), h_cnt = S.in(cnt, sizeof cnt);
  const int h_label = S.out(label_out, n * sizeof(int32_t), true), h_reason = S.out(reason_out, n, true);
  const int h_csize = S.out(nullptr, n * sizeof(int32_t), true), h_index = S.out(nullptr, n * sizeof(int64_t), true);
  const int h_out = S.out(nullptr, 3 * n * sizeof(double), true);
  MapCellStage index;                                              // the scans work in its scratch
  if (int rc = index.reserve(S, n, scan_bytes)) return rc;
  const int h_parent = S.out(nullptr, n * sizeof(int32_t), true), h_size = S.out(nullptr, n * sizeof(uint32_t), true);
  const int h_flag = S.out(nullptr, n * sizeof(uint32_t), true), h_num = S.out(nullptr, n * sizeof(uint32_t), true);
  const int h_pos = S.out(nullptr, n * sizeof(uint32_t), true), h_bins = S.out(nullptr, MC_MAX_BINS * sizeof(uint32_t), true);
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  A.xyz = S.ptr<double>(h_xyz); A.cnt = S.ptr<long long>(h_cnt);
  A.label = S.ptr<int32_t>(h_label); A.reason = S.ptr<uint8_t>(h_reason); A.csize = S.ptr<int32_t>(h_csize);
  A.index = S.ptr<int64_t>(h_index); A.xyz_out = S.ptr<double>(h_out);
  index.bind(S, A);
  A.parent = S.ptr<int32_t>(h_parent); A.size = S.ptr<uint32_t>(h_size);
  A.flag = S.ptr<uint32_t>(h_flag); A.num = S.ptr<uint32_t>(h_num); A.pos = S.ptr<uint32_t>(h_pos); A.bins = S.ptr<uint32_t>(h_bins);

  KernelTimer timer;
  const dim3 grid(grid_for(n, MC_T)), block(MC_T);
  if (!timer.start()) return FGO_ENUM;
  if (hipMemsetAsync(A.bins, 0, MC_MAX_BINS * sizeof(uint32_t), 0) != hipSuccess) return FGO_ENUM;
  hipLaunchKernelGGL(k_mc_quantise, grid, block, 0, 0, A);
  if (int rc = index.build(A, A.cnt + MC_C_CELLS)) return rc;
  hipLaunchKernelGGL(k_mc_link, grid, block, 0, 0, A);
  hipLaunchKernelGGL(k_mc_flatten, grid, block, 0, 0, A);
  hipLaunchKernelGGL(k_mc_roots, grid, block, 0, 0, A);
  if (rocprim::exclusive_scan(index.scratch, scan_bytes, A.flag, A.num, 0u, n, rocprim::plus<uint32_t>(), 0) != hipSuccess) return FGO_ENUM;
  hipLaunchKernelGGL(k_mc_label, grid, block, 0, 0, A);
  if (P.remove_floor) {
    hipLaunchKernelGGL(k_mc_hist, dim3(grid.x < MC_HIST_GRID ? grid.x : MC_HIST_GRID), block, 0, 0, A);
    hipLaunchKernelGGL(k_mc_floor, dim3(1), block, 0, 0, A);
  }
  hipLaunchKernelGGL(k_mc_mask, grid, block, 0, 0, A);
  if (rocprim::exclusive_scan(index.scratch, scan_bytes, A.flag, A.pos, 0u, n, rocprim::plus<uint32_t>(), 0) != hipSuccess) return FGO_ENUM;
  hipLaunchKernelGGL(k_mc_compact, grid, block, 0, 0, A);
  timer.stop();
  if (hipMemcpy(cnt, A.cnt, sizeof cnt, hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  g_mc_kernel_ms = timer.ms();

  result->n_points = n_points;
  result->n_out_of_range = cnt[MC_C_OOR];
  result->n_cells = cnt[MC_C_CELLS];
  result->n_clusters = cnt[MC_C_CLUSTERS];
  result->n_clusters_kept = cnt[MC_C_CLUSTERS_KEPT];
  result->n_after_clusters = cnt[MC_C_AFTER];
  result->n_floor_removed = cnt[MC_C_AFTER] - cnt[MC_C_KEPT];     // only the floor stage takes a point that the cluster stage left
  result->n_kept = cnt[MC_C_KEPT];
  result->floor_bin = cnt[MC_C_FLOOR_BIN];
  result->floor_bin_points = cnt[MC_C_FLOOR_CNT];
  result->floor_height = (double)cnt[MC_C_F] * (1.0 / MAP_QUANTA_PER_M);
  if (int rc = S.download()) return rc;                            // label and reason: n rows each
  // only the n_clusters sizes and the n_kept rows go back
  const size_t nc = (size_t)cnt[MC_C_CLUSTERS], nk = (size_t)cnt[MC_C_KEPT];
  void *const host[3] = {cluster_size_out, index_out, xyz_out};
  const void *const dev[3] = {A.csize, A.index, A.xyz_out};
  const size_t bytes[3] = {nc * sizeof(int32_t), nk * sizeof(int64_t), 3 * nk * sizeof(double)};
  for (int k = 0; k < 3; ++k)
    if (host[k] && bytes[k] && hipMemcpy(host[k], dev[k], bytes[k], hipMemcpyDeviceToHost) != hipSuccess) return FGO_ENUM;
  return FGO_OK;
}
