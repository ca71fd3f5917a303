// Cluster filtering and floor removal of a point cloud on the MI355X (gfx950, 64-bit integers, wave64): the program that ends the
// reference's run, mapping/pcd_filter.cpp -- clusterFilter(0.03, ...) = pcl::EuclideanClusterExtraction with setMinClusterSize(200),
// then remove_floor_pt -- in ONE call.  include/fgo.h states the semantics (this project's: integer distances on the 2^-20 m quantum,
// clusters numbered by their smallest member), tests/map_clean_reference.py restates them in numpy.
//
//   quantise  one lane per point: Q = llrint(x 2^20), the cell c = floor(Q / T) and its key, or the out-of-range mark.  Contraction
//             is switched off for these lines; from there on everything is integer.
//   sort      rocPRIM's radix sort of the (cell key, input index) pairs.  It is stable, so a cell's run is in ascending input index;
//             the out-of-range mark is the largest key and sorts behind every cell.
//   cells     the quantised coordinates are gathered into sorted order and the run heads are counted.  A cell's run is found by
//             binary search of the sorted keys (map_cells_device.hpp, shared with kernels_map_normals.hip, as are the floor
//             division and the key): neighbouring lanes look for neighbouring cells, so the upper levels of the search stay in cache.  An open-addressing table cell key -> start of the run (64-bit atomicCAS on the key, two slots per
//             point) was built and measured as well: 5 % faster on a map of 44 000 points, 11 % slower on a sheet of 2 000 000,
//             24 to 48 more bytes per point; it is not kept (the figures of both: profiles/NOTES.md).
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
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>
#include <climits>
#include <cmath>
#include <cstring>
#include "../../include/fgo.h"
#include "batch_call.hpp"
#include "map_cells_device.hpp"

namespace fgo {
namespace {

using dev::map_cell_key;

constexpr int MC_T = 256;                        // threads of a workgroup
constexpr long long MC_IMAX = dev::MAP_CELL_BIAS; // |c_k| < 2^20
constexpr unsigned long long MC_EMPTY = dev::MAP_CELL_EMPTY;      // the key of an out-of-range point: behind every cell in sorted order
constexpr uint32_t MC_NONE = ~0u;                // no such cell
constexpr unsigned MC_MAX_GRID = 1u << 20;       // workgroups of a launch; the kernels stride beyond that
constexpr int MC_MAX_BINS = 8192;                // floor_span / floor_res <= 4096 gives at most 6145 bins (R = 1, S = 6144)
constexpr unsigned MC_HIST_GRID = 1024;          // workgroups of the histogram: each flushes its bins once

enum { MC_C_OOR, MC_C_CELLS, MC_C_CLUSTERS, MC_C_CLUSTERS_KEPT, MC_C_AFTER, MC_C_HMIN, MC_C_FLOOR_BIN, MC_C_FLOOR_CNT, MC_C_F, MC_C_KEPT,
       MC_C_COUNT };

struct McArgs {
  int64_t n;
  long long T, T2, R, S, C;
  int min_size, max_size, floor, axis, sign, nbins;
  const double *xyz;
  long long *Q, *sQ;                             // n x 3: in input order, in sorted order
  unsigned long long *key, *skey;                // in input order (what says "in range" from the sort on), sorted
  uint32_t *idx, *sidx;
  int32_t *parent;
  uint32_t *size, *flag, *num, *pos, *bins;      // flag: is a root, then: is kept
  long long *cnt;
  int32_t *label, *csize;                        // label holds the root until the clusters are numbered
  uint8_t *reason;
  int64_t *index;
  double *xyz_out;
};

// counts the lanes that get here: the first of them adds their number, one atomic per wave and call.  (One atomicAdd of 1 per lane,
// all on one address, measured 12 ns per POINT in a kernel that counted the kept points: nine tenths of the call.  The counts that
// a scan ends on anyway -- clusters, kept points -- are read off the scan instead.)
__device__ inline void mc_count(long long *cnt, int which) {
  const unsigned long long m = __ballot(1);
  if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1)
    atomicAdd(reinterpret_cast<unsigned long long *>(cnt + which), (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(MC_T) void k_mc_quantise(McArgs A) {
#pragma clang fp contract(off)
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < A.n; p += stride) {
    bool ok = true;
    long long c[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double y = A.xyz[3 * p + k] * 1048576.0;
      long long Q = 0;
      if (fabs(y) < 4611686018427387904.0) {                       // finite and below 2^62
        Q = llrint(y);                                             // ties to even
        const long long q = dev::map_floor_div(Q, A.T);
        if (q <= -MC_IMAX || q >= MC_IMAX) ok = false;
        c[k] = q;
      } else ok = false;
      A.Q[3 * p + k] = Q;
    }
    A.key[p] = ok ? map_cell_key(c[0] + MC_IMAX, c[1] + MC_IMAX, c[2] + MC_IMAX) : MC_EMPTY;
    A.idx[p] = (uint32_t)p;
    A.parent[p] = (int32_t)p;
    A.size[p] = 0;
    if (!ok) mc_count(A.cnt, MC_C_OOR);
  }
}

// Q in sorted order; the occupied cells are the run heads
__global__ __launch_bounds__(MC_T) void k_mc_cells(McArgs A) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t s = (int64_t)blockIdx.x * MC_T + threadIdx.x; s < A.n; s += stride) {
    const unsigned long long key = A.skey[s];
    if (key == MC_EMPTY) continue;
    const int64_t p = A.sidx[s];
#pragma unroll
    for (int k = 0; k < 3; ++k) A.sQ[3 * s + k] = A.Q[3 * p + k];
    if (s == 0 || A.skey[s - 1] != key) mc_count(A.cnt, MC_C_CELLS);
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
    if (key == MC_EMPTY) continue;
    const long long q0 = A.sQ[3 * s], q1 = A.sQ[3 * s + 1], q2 = A.sQ[3 * s + 2];
    const int32_t p = (int32_t)A.sidx[s];
    auto visit = [&](int64_t j) {
      const long long d0 = A.sQ[3 * j] - q0, d1 = A.sQ[3 * j + 1] - q1, d2 = A.sQ[3 * j + 2] - q2;
      if (d0 * d0 + d1 * d1 + d2 * d2 <= A.T2) mc_unite(A.parent, p, (int32_t)A.sidx[j]);
    };
    for (int64_t j = s - 1; j >= 0 && A.skey[j] == key; --j) visit(j);         // its own cell: the points before it
    const long long c[3] = {(long long)(key & 0x1fffff), (long long)((key >> 21) & 0x1fffff), (long long)(key >> 42)};      // c_k + 2^20
    for (int t = 0; t < 13; ++t) {                                             // the neighbour cells before its own in key order
      const long long e[3] = {c[0] + t % 3 - 1, c[1] + (t / 3) % 3 - 1, c[2] + t / 9 - 1};
      if (e[0] < 1 || e[1] < 1 || e[2] < 1 || e[0] >= 2 * MC_IMAX || e[1] >= 2 * MC_IMAX || e[2] >= 2 * MC_IMAX) continue;   // no such cell
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
    bool todo = p < A.n && A.key[p] != MC_EMPTY;
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
    const bool root = p < A.n && A.key[p] != MC_EMPTY && A.label[p] == (int32_t)p;
    if (p < A.n) A.flag[p] = root;
    unsigned long long kept = root && mc_size_ok(A, A.size[p]) ? A.size[p] : 0;
    if (kept) mc_count(A.cnt, MC_C_CLUSTERS_KEPT);
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
      if (p == A.n - 1) A.cnt[MC_C_CLUSTERS] = (long long)A.num[p] + (A.key[p] != MC_EMPTY && A.label[p] == (int32_t)p);
      if (A.key[p] == MC_EMPTY) {
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
  const double lift = (double)A.sign * ((double)A.cnt[MC_C_F] * (1.0 / 1048576.0));      // up_sign floor_height: exact
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

unsigned grid_for(unsigned long long items, unsigned per_group) {
  const unsigned long long g = (items + per_group - 1) / per_group;
  return (unsigned)(g < 1 ? 1 : g > MC_MAX_GRID ? MC_MAX_GRID : g);
}

bool in_closed(double v, double lo, double hi) { return v >= lo && v <= hi; }      // false for a NaN

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
  if (!in_closed(P.tolerance, 1.0 / 1048576.0, 256.0)) return FGO_EINVAL;
  if (P.min_cluster_size < 1 || P.max_cluster_size < 0 || (P.max_cluster_size >= 1 && P.max_cluster_size < P.min_cluster_size)) return FGO_EINVAL;
  if (P.up_axis < 0 || P.up_axis > 2 || (P.up_sign != 1 && P.up_sign != -1) || (P.remove_floor != 0 && P.remove_floor != 1)) return FGO_EINVAL;
  McArgs A;
  std::memset(&A, 0, sizeof A);
  A.nbins = 1;
  if (P.remove_floor) {
    if (!in_closed(P.floor_res, 1.0 / 1048576.0, 1024.0) || !in_closed(P.floor_span, 0.0, HUGE_VAL) || !(P.floor_span / P.floor_res <= 4096.0))
      return FGO_EINVAL;
    if (!in_closed(P.floor_clearance, 0.0, HUGE_VAL) || P.floor_clearance == HUGE_VAL) return FGO_EINVAL;
    A.R = llrint(P.floor_res * 1048576.0);
    A.S = llrint(P.floor_span * 1048576.0);
    const double c = P.floor_clearance * 1048576.0;
    A.C = c < 4611686018427387904.0 ? llrint(c) : (1ll << 62);                  // no height reaches 2^49: beyond that every C acts alike
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
  A.T = llrint(P.tolerance * 1048576.0);
  A.T2 = A.T * A.T;
  A.min_size = P.min_cluster_size; A.max_size = P.max_cluster_size;
  A.floor = P.remove_floor; A.axis = P.up_axis; A.sign = P.up_sign;

  size_t sort_bytes = 0, scan_bytes = 0;
  {
    unsigned long long *no_key = nullptr;
    uint32_t *no_val = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, sort_bytes, no_key, no_key, no_val, no_val, n, 0, 64, 0) != hipSuccess) return FGO_ENUM;
    if (rocprim::exclusive_scan(nullptr, scan_bytes, no_val, no_val, 0u, n, rocprim::plus<uint32_t>(), 0) != hipSuccess) return FGO_ENUM;
  }
  long long cnt[MC_C_COUNT] = {0};
  cnt[MC_C_HMIN] = LLONG_MAX;
  cnt[MC_C_FLOOR_BIN] = -1;
  Staged S;
  const int h_xyz = S.in(xyz, 3 * n * sizeof(double)), h_cnt = S.in(cnt, sizeof cnt);
  const int h_label = S.out(label_out, n * sizeof(int32_t), true), h_reason = S.out(reason_out, n, true);
  const int h_csize = S.out(nullptr, n * sizeof(int32_t), true), h_index = S.out(nullptr, n * sizeof(int64_t), true);
  const int h_out = S.out(nullptr, 3 * n * sizeof(double), true);
  const int h_Q = S.out(nullptr, 3 * n * sizeof(long long), true), h_sQ = S.out(nullptr, 3 * n * sizeof(long long), true);
  const int h_key = S.out(nullptr, n * sizeof(unsigned long long), true), h_skey = S.out(nullptr, n * sizeof(unsigned long long), true);
  const int h_idx = S.out(nullptr, n * sizeof(uint32_t), true), h_sidx = S.out(nullptr, n * sizeof(uint32_t), true);
  const int h_parent = S.out(nullptr, n * sizeof(int32_t), true), h_size = S.out(nullptr, n * sizeof(uint32_t), true);
  const int h_flag = S.out(nullptr, n * sizeof(uint32_t), true), h_num = S.out(nullptr, n * sizeof(uint32_t), true);
  const int h_pos = S.out(nullptr, n * sizeof(uint32_t), true), h_bins = S.out(nullptr, MC_MAX_BINS * sizeof(uint32_t), true);
  const int h_tmp = S.out(nullptr, sort_bytes > scan_bytes ? sort_bytes : scan_bytes, true);
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  A.xyz = S.ptr<double>(h_xyz); A.cnt = S.ptr<long long>(h_cnt);
  A.label = S.ptr<int32_t>(h_label); A.reason = S.ptr<uint8_t>(h_reason); A.csize = S.ptr<int32_t>(h_csize);
  A.index = S.ptr<int64_t>(h_index); A.xyz_out = S.ptr<double>(h_out);
  A.Q = S.ptr<long long>(h_Q); A.sQ = S.ptr<long long>(h_sQ);
  A.key = S.ptr<unsigned long long>(h_key); A.skey = S.ptr<unsigned long long>(h_skey);
  A.idx = S.ptr<uint32_t>(h_idx); A.sidx = S.ptr<uint32_t>(h_sidx);
  A.parent = S.ptr<int32_t>(h_parent); A.size = S.ptr<uint32_t>(h_size);
  A.flag = S.ptr<uint32_t>(h_flag); A.num = S.ptr<uint32_t>(h_num); A.pos = S.ptr<uint32_t>(h_pos); A.bins = S.ptr<uint32_t>(h_bins);
  void *tmp = S.ptr<void>(h_tmp);

  Events ev;
  if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) return FGO_ENUM;
  const dim3 grid(grid_for(n, MC_T)), block(MC_T);
  (void)hipEventRecord(ev.a, 0);
  if (hipMemsetAsync(A.bins, 0, MC_MAX_BINS * sizeof(uint32_t), 0) != hipSuccess) return FGO_ENUM;
  hipLaunchKernelGGL(k_mc_quantise, grid, block, 0, 0, A);
  if (rocprim::radix_sort_pairs(tmp, sort_bytes, A.key, A.skey, A.idx, A.sidx, n, 0, 64, 0) != hipSuccess) return FGO_ENUM;
  hipLaunchKernelGGL(k_mc_cells, grid, block, 0, 0, A);
  hipLaunchKernelGGL(k_mc_link, grid, block, 0, 0, A);
  hipLaunchKernelGGL(k_mc_flatten, grid, block, 0, 0, A);
  hipLaunchKernelGGL(k_mc_roots, grid, block, 0, 0, A);
  if (rocprim::exclusive_scan(tmp, scan_bytes, A.flag, A.num, 0u, n, rocprim::plus<uint32_t>(), 0) != hipSuccess) return FGO_ENUM;
  hipLaunchKernelGGL(k_mc_label, grid, block, 0, 0, A);
  if (P.remove_floor) {
    const unsigned g = grid_for(n, MC_T);
    hipLaunchKernelGGL(k_mc_hist, dim3(g < MC_HIST_GRID ? g : MC_HIST_GRID), block, 0, 0, A);
    hipLaunchKernelGGL(k_mc_floor, dim3(1), block, 0, 0, A);
  }
  hipLaunchKernelGGL(k_mc_mask, grid, block, 0, 0, A);
  if (rocprim::exclusive_scan(tmp, scan_bytes, A.flag, A.pos, 0u, n, rocprim::plus<uint32_t>(), 0) != hipSuccess) return FGO_ENUM;
  hipLaunchKernelGGL(k_mc_compact, grid, block, 0, 0, A);
  (void)hipEventRecord(ev.b, 0);
  if (hipMemcpy(cnt, A.cnt, sizeof cnt, hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  float ms = 0;
  if (hipEventElapsedTime(&ms, ev.a, ev.b) != hipSuccess) ms = 0;
  g_mc_kernel_ms = (double)ms;

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
  result->floor_height = (double)cnt[MC_C_F] * (1.0 / 1048576.0);
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
