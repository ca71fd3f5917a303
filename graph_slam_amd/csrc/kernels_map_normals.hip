// k-nearest-neighbour surface normals of a point cloud on the MI355X (gfx950, 64-bit integers and f64, wave64): the first half of
// the reference's mapping/pcd2mesh.cpp:52-67 -- pcl::NormalEstimation with a kd-tree and setKSearch(20), a normal and a curvature
// for every point of the map -- in ONE call.  include/fgo.h states the semantics (this project's: integer distances on the 2^-20 m
// quantum, the neighbours in ascending (d2, input index), an exact integer scatter matrix), tests/map_normals_reference.py restates
// them in numpy.  The search is exact and its outputs do not depend on the side of the search cells.
//
//   quantise  one lane per point: Q = llrint(x 2^20), the range test |Q_k| < 2^34, the cell c = floor(Q / T_cell) and its key, or the
//             out-of-range mark and that point's outputs (status 1, NaN, no neighbours).
//   index     map_cell_index.hip, shared with kernels_map_clean.hip: the stable sort of the (cell key, input index) pairs, so a
//             cell's run is in ascending input index, and the gather of Q into sorted order; the run heads are the occupied cells.
//   search    one lane per point in SORTED order, so that the lanes of a wave read the same runs.  The cells are visited in rings
//             (Chebyshev shells) around the point's own cell.  The x coordinate is the low field of the key, so the cells of one
//             (y, z) row of a shell are one stretch of the sorted keys: one binary search per row, two for a row of which only the
//             two end cells belong to the shell.  The best k pairs (d2, input index) are kept SORTED, by insertion from the end, in
//             LDS laid out [entry][lane]: 12 bytes per entry, the workgroup is sized from k so that the list fits 64 KiB (256 lanes
//             up to k = 21, 128 up to 42, 64 beyond).  The worst pair kept is mirrored in registers, so a candidate that does not
//             make the list costs no LDS access.
//             STOPPING RULE: after ring r every point not yet seen lies outside the cube of (2 r + 1)^3 cells, so along some axis
//             it is at least g = r T_cell + min_k min(off_k + 1, T_cell - off_k) quanta away (off_k = Q_k - c_k T_cell, the point's
//             offset in its own cell).  The search ends when g > Rq (nothing outside is within the radius), or when the list is full
//             and g^2 > the k-th d2 (STRICTLY: at equality a point outside with a smaller index would still displace it).
//             g >= r T_cell + 1, so there are at most Rq / T_cell <= 17 rings.
//   fit       in the same launch, by the same lane: the list is written out, dQ is summed into S1 and S2 in 64-bit integers,
//             M = m S2 - S1 S1^T, A = (double)M / (m^2 2^40), 8 sweeps of the shared 3x3 cyclic Jacobi, the orientation.
// No floating-point atomics, and no barrier at all: a lane owns its column of the list.  The whole file is compiled with
// contraction off, the shared Jacobi rotation included: the double arithmetic is the one include/fgo.h states.  The grids are
// capped and the kernels stride beyond that.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
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

using dev::MAP_QUANTA_PER_M;

constexpr int MN_T = 256;                        // threads of a workgroup; the search runs with 256, 128 or 64
constexpr int MN_K_MAX = 64;
constexpr size_t MN_LDS = 65536;                 // what the candidate lists of a workgroup may take
constexpr long long MN_QMAX = 1ll << 34;         // |Q_k| < 2^34
constexpr int MN_SWEEPS = 8;                     // cyclic Jacobi sweeps (quadratic convergence: 4 - 5 reach rounding)

enum { MN_C_OOR, MN_C_CELLS, MN_C_VALID, MN_C_FEW, MN_C_DEGENERATE, MN_C_COUNT };

struct MnArgs : dev::MapCellIndex {              // n, Q, sQ, key, skey, idx, sidx
  int k;
  long long T, R, R2;                            // the cell, the radius and its square, in quanta
  double view[3];
  const double *xyz;
  long long *cnt;
  double *normal, *curvature, *eig;              // eig may be NULL
  int32_t *nn;
  uint8_t *status;
  int32_t *neighbour;                            // n x k, may be NULL
  int64_t *dist2, *scatter;                      // n x k, n x 6, may be NULL
};

// what a point without a fit gets: NaN for every floating output
__device__ inline void mn_no_fit(const MnArgs &A, int64_t p, int status) {
  const double nan = __builtin_nan("");
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    A.normal[3 * p + c] = nan;
    if (A.eig) A.eig[3 * p + c] = nan;
  }
  A.curvature[p] = nan;
  A.status[p] = (uint8_t)status;
}

__global__ __launch_bounds__(MN_T) void k_mn_quantise(MnArgs A) {
  const int64_t stride = (int64_t)gridDim.x * MN_T;
  for (int64_t p = (int64_t)blockIdx.x * MN_T + threadIdx.x; p < A.n; p += stride) {
    bool ok = true;
    long long e[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      long long Q;
      if (dev::map_quantise(A.xyz[3 * p + c], 0x1p35, Q)) {               // 2^35: beyond the range, and llrint is safe
        if (Q <= -MN_QMAX || Q >= MN_QMAX) ok = false;
        e[c] = dev::map_floor_div(Q, A.T) + dev::MAP_CELL_BIAS;    // in [0, 2^21) when in range: T >= 2^14
      } else ok = false;
      A.Q[3 * p + c] = Q;
    }
    A.key[p] = ok ? dev::map_cell_key(e[0], e[1], e[2]) : dev::MAP_CELL_EMPTY;
    A.idx[p] = (uint32_t)p;
    if (!ok) {
      mn_no_fit(A, p, 1);
      A.nn[p] = 0;
      for (int e2 = 0; e2 < A.k; ++e2) {
        if (A.neighbour) A.neighbour[p * A.k + e2] = -1;
        if (A.dist2) A.dist2[p * A.k + e2] = -1;
      }
      if (A.scatter)
        for (int c = 0; c < 6; ++c) A.scatter[6 * p + c] = 0;
      dev::wave_count(A.cnt + MN_C_OOR);
    }
  }
}

// the eigen-decomposition of the scatter matrix, the normal, its orientation and the curvature of one valid point
__device__ inline void mn_fit(const MnArgs &A, int64_t p, int m, const long long M[6], const long long q[3]) {
  const double den = (double)((long long)m * m) * (MAP_QUANTA_PER_M * MAP_QUANTA_PER_M);      // m^2 2^40, quanta^2 to m^2: exact
  const double xx = (double)M[0] / den, xy = (double)M[1] / den, xz = (double)M[2] / den;
  const double yy = (double)M[3] / den, yz = (double)M[4] / den, zz = (double)M[5] / den;
  double a[9] = {xx, xy, xz, xy, yy, yz, xz, yz, zz};
  double v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll 1
  for (int sweep = 0; sweep < MN_SWEEPS; ++sweep) {
    dev::jacobi_rot<3, 0, 1>(a, v); dev::jacobi_rot<3, 0, 2>(a, v); dev::jacobi_rot<3, 1, 2>(a, v);
  }
  // ascending eigenvalues with their columns: three compare-and-swaps, the earlier column first on a tie
  double l[3] = {a[0], a[4], a[8]};
  double e[3][3] = {{v[0], v[3], v[6]}, {v[1], v[4], v[7]}, {v[2], v[5], v[8]}};
  auto order = [&](int i, int j) {
    if (l[j] < l[i]) {
      const double t = l[i]; l[i] = l[j]; l[j] = t;
#pragma unroll
      for (int c = 0; c < 3; ++c) { const double u = e[i][c]; e[i][c] = e[j][c]; e[j][c] = u; }
    }
  };
  order(0, 1); order(1, 2); order(0, 1);
  const double len = sqrt((e[0][0] * e[0][0] + e[0][1] * e[0][1]) + e[0][2] * e[0][2]);
  double nx = e[0][0] / len, ny = e[0][1] / len, nz = e[0][2] / len;
  const double d0 = A.view[0] - (double)q[0] * (1.0 / MAP_QUANTA_PER_M), d1 = A.view[1] - (double)q[1] * (1.0 / MAP_QUANTA_PER_M),
               d2 = A.view[2] - (double)q[2] * (1.0 / MAP_QUANTA_PER_M);
  const double dot = (nx * d0 + ny * d1) + nz * d2;
  bool flip = dot < 0;
  if (dot == 0) flip = nx != 0 ? nx < 0 : ny != 0 ? ny < 0 : nz < 0;         // the first non-zero component positive
  if (flip) { nx = -nx; ny = -ny; nz = -nz; }
  A.normal[3 * p] = nx; A.normal[3 * p + 1] = ny; A.normal[3 * p + 2] = nz;
  A.curvature[p] = l[0] / ((l[0] + l[1]) + l[2]);
  if (A.eig) { A.eig[3 * p] = l[0]; A.eig[3 * p + 1] = l[1]; A.eig[3 * p + 2] = l[2]; }
  A.status[p] = 0;
}

// The list of lane t: entry e is D[e * W + t] (d2) and I[e * W + t] (input index), W = blockDim.x: the lanes of a wave hit
// different banks.  D takes the first 8 k W bytes of the dynamic LDS, I the 4 k W behind them.
__global__ __launch_bounds__(MN_T) void k_mn_search(MnArgs A) {
  extern __shared__ unsigned long long mn_lds[];
  const int W = (int)blockDim.x, k = A.k;
  long long *const D = reinterpret_cast<long long *>(mn_lds) + threadIdx.x;
  uint32_t *const I = reinterpret_cast<uint32_t *>(mn_lds + (size_t)k * W) + threadIdx.x;
  const long long EMAX = 2 * dev::MAP_CELL_BIAS - 1;                          // the largest biased cell coordinate
  const int64_t stride = (int64_t)gridDim.x * W;
  for (int64_t s = (int64_t)blockIdx.x * W + threadIdx.x; s < A.n; s += stride) {
    const unsigned long long key = A.skey[s];
    if (key == dev::MAP_CELL_EMPTY) continue;
    const long long q[3] = {A.sQ[3 * s], A.sQ[3 * s + 1], A.sQ[3 * s + 2]};
    const int64_t p = A.sidx[s];
    const long long c[3] = {dev::map_cell_coord(key, 0), dev::map_cell_coord(key, 1), dev::map_cell_coord(key, 2)};      // biased
    long long gmin = LLONG_MAX;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const long long off = q[a] - (c[a] - dev::MAP_CELL_BIAS) * A.T;         // in [0, T)
      const long long near = off + 1 < A.T - off ? off + 1 : A.T - off;
      gmin = near < gmin ? near : gmin;
    }
    int cnt = 0;
    long long wd = LLONG_MAX;                                                 // the worst pair kept, once the list is full
    uint32_t wi = ~0u;
    // the points of the cells [x0, x1] of the row (ey, ez): one stretch of the sorted keys
    auto row = [&](long long x0, long long x1, long long ey, long long ez) {
      if (x0 < 0) x0 = 0;
      if (x1 > EMAX) x1 = EMAX;
      if (x0 > x1) return;
      const unsigned long long k1 = dev::map_cell_key(x1, ey, ez);
      for (int64_t j = dev::map_key_lower_bound(A.skey, A.n, dev::map_cell_key(x0, ey, ez)); j < A.n && A.skey[j] <= k1; ++j) {
        const long long t0 = A.sQ[3 * j] - q[0], t1 = A.sQ[3 * j + 1] - q[1], t2 = A.sQ[3 * j + 2] - q[2];
        const long long d2 = t0 * t0 + t1 * t1 + t2 * t2;                     // |t| <= 18 T <= 2^29
        if (d2 > A.R2 || d2 > wd) continue;
        const uint32_t i = A.sidx[j];
        if (d2 == wd && i > wi) continue;
        int e = cnt < k ? cnt : k - 1;                                        // the slot that opens: behind the list, or its last
        while (e > 0) {
          const long long pd = D[(e - 1) * W];
          const uint32_t pi = I[(e - 1) * W];
          if (pd < d2 || (pd == d2 && pi < i)) break;
          D[e * W] = pd; I[e * W] = pi;
          --e;
        }
        D[e * W] = d2; I[e * W] = i;
        if (cnt < k) ++cnt;
        if (cnt == k) { wd = D[(k - 1) * W]; wi = I[(k - 1) * W]; }
      }
    };
    for (long long r = 0;; ++r) {
      for (long long dz = -r; dz <= r; ++dz) {
        const long long ez = c[2] + dz;
        if (ez < 0 || ez > EMAX) continue;
        for (long long dy = -r; dy <= r; ++dy) {
          const long long ey = c[1] + dy;
          if (ey < 0 || ey > EMAX) continue;
          if (dz == -r || dz == r || dy == -r || dy == r) row(c[0] - r, c[0] + r, ey, ez);
          else { row(c[0] - r, c[0] - r, ey, ez); row(c[0] + r, c[0] + r, ey, ez); }
        }
      }
      const long long g = r * A.T + gmin;                                     // every point not seen yet is at least g away
      if (g > A.R || (cnt == k && g * g > wd)) break;
    }
    // the list is in ascending (d2, index): out it goes, and into the integer sums
    long long S1[3] = {0, 0, 0}, S2[6] = {0, 0, 0, 0, 0, 0};
    for (int e = 0; e < cnt; ++e) {
      const int64_t i = I[e * W];
      if (A.neighbour) A.neighbour[p * k + e] = (int32_t)i;
      if (A.dist2) A.dist2[p * k + e] = D[e * W];
      const long long t0 = A.Q[3 * i] - q[0], t1 = A.Q[3 * i + 1] - q[1], t2 = A.Q[3 * i + 2] - q[2];
      S1[0] += t0; S1[1] += t1; S1[2] += t2;
      S2[0] += t0 * t0; S2[1] += t0 * t1; S2[2] += t0 * t2; S2[3] += t1 * t1; S2[4] += t1 * t2; S2[5] += t2 * t2;
    }
    for (int e = cnt; e < k; ++e) {
      if (A.neighbour) A.neighbour[p * k + e] = -1;
      if (A.dist2) A.dist2[p * k + e] = -1;
    }
    A.nn[p] = cnt;
    const long long m = cnt;
    const long long M[6] = {m * S2[0] - S1[0] * S1[0], m * S2[1] - S1[0] * S1[1], m * S2[2] - S1[0] * S1[2],
                            m * S2[3] - S1[1] * S1[1], m * S2[4] - S1[1] * S1[2], m * S2[5] - S1[2] * S1[2]};
    if (A.scatter)
#pragma unroll
      for (int a = 0; a < 6; ++a) A.scatter[6 * p + a] = M[a];
    if (cnt < 3) {
      mn_no_fit(A, p, 2);
      dev::wave_count(A.cnt + MN_C_FEW);
    } else if ((M[0] | M[1] | M[2] | M[3] | M[4] | M[5]) == 0) {
      mn_no_fit(A, p, 3);
      dev::wave_count(A.cnt + MN_C_DEGENERATE);
    } else {
      mn_fit(A, p, cnt, M, q);
      dev::wave_count(A.cnt + MN_C_VALID);
    }
  }
}

double g_mn_kernel_ms = 0.0;

}  // namespace
}  // namespace fgo

extern "C" double fgo_debug_map_normals_kernel_ms(void) { return fgo::g_mn_kernel_ms; }

extern "C" void fgo_map_normals_params_default(fgo_map_normals_params *p) {
  if (!p) return;
  p->k = 20;
  p->max_radius = 0.16;
  p->cell = 0.04;
  p->viewpoint[0] = p->viewpoint[1] = p->viewpoint[2] = 0.0;
}

extern "C" int fgo_map_normals(int device, int64_t n_points, const double *xyz, const fgo_map_normals_params *params,
                               fgo_map_normals_result *result, double *normal_out, double *curvature_out, double *eigenvalues_out,
                               int32_t *n_neighbours_out, uint8_t *status_out, int32_t *neighbour_out, int64_t *dist2_out,
                               int64_t *scatter_out) {
  using namespace fgo;
  fgo_map_normals_params P;
  fgo_map_normals_params_default(&P);
  if (params) P = *params;
  if (!result || n_points < 0 || n_points >= (1ll << 30) || (n_points > 0 && !xyz)) return FGO_EINVAL;
  if (n_points > 0 && (!normal_out || !curvature_out || !n_neighbours_out || !status_out)) return FGO_EINVAL;
  if (P.k < 3 || P.k > MN_K_MAX) return FGO_EINVAL;
  if (!in_closed(P.max_radius, 1.0 / MAP_QUANTA_PER_M, 16.0) || !in_closed(P.cell, 1.0 / 64.0, 16.0)) return FGO_EINVAL;
  if (!(P.max_radius / P.cell <= 16.0)) return FGO_EINVAL;
  for (int c = 0; c < 3; ++c)
    if (!std::isfinite(P.viewpoint[c])) return FGO_EINVAL;
  std::memset(result, 0, sizeof *result);
  if (n_points == 0) return FGO_OK;
  if (int rc = select_device(device)) return rc;

  const size_t n = (size_t)n_points, k = (size_t)P.k;
  MnArgs A;
  std::memset(&A, 0, sizeof A);
  A.n = n_points;
  A.k = P.k;
  A.T = llrint(P.cell * MAP_QUANTA_PER_M);
  A.R = llrint(P.max_radius * MAP_QUANTA_PER_M);
  A.R2 = A.R * A.R;
  for (int c = 0; c < 3; ++c) A.view[c] = P.viewpoint[c];
  unsigned W = MN_T;                                                          // the search's workgroup: its lists fit MN_LDS
  while (W > 64 && k * W * 12 > MN_LDS) W /= 2;

  long long cnt[MN_C_COUNT] = {0};
  Staged S;
  const int h_xyz = S.in(xyz, 3 * n * sizeof(double)), h_cnt = S.in(cnt, sizeof cnt);
  const int h_normal = S.out(normal_out, 3 * n * sizeof(double)), h_curv = S.out(curvature_out, n * sizeof(double));
  const int h_eig = S.out(eigenvalues_out, 3 * n * sizeof(double));
  const int h_nn = S.out(n_neighbours_out, n * sizeof(int32_t)), h_status = S.out(status_out, n);
  const int h_nb = S.out(neighbour_out, n * k * sizeof(int32_t)), h_d2 = S.out(dist2_out, n * k * sizeof(int64_t));
  const int h_sc = S.out(scatter_out, 6 * n * sizeof(int64_t));
  MapCellStage index;
  if (int rc = index.reserve(S, n)) return rc;
  if (int rc = S.alloc()) return rc;
  if (int rc = S.upload()) return rc;
  A.xyz = S.ptr<double>(h_xyz); A.cnt = S.ptr<long long>(h_cnt);
  A.normal = S.ptr<double>(h_normal); A.curvature = S.ptr<double>(h_curv); A.eig = S.ptr<double>(h_eig);
  A.nn = S.ptr<int32_t>(h_nn); A.status = S.ptr<uint8_t>(h_status);
  A.neighbour = S.ptr<int32_t>(h_nb); A.dist2 = S.ptr<int64_t>(h_d2); A.scatter = S.ptr<int64_t>(h_sc);
  index.bind(S, A);

  KernelTimer timer;
  if (!timer.start()) return FGO_ENUM;
  hipLaunchKernelGGL(k_mn_quantise, dim3(grid_for(n, MN_T)), dim3(MN_T), 0, 0, A);
  if (int rc = index.build(A, A.cnt + MN_C_CELLS)) return rc;
  hipLaunchKernelGGL(k_mn_search, dim3(grid_for(n, W)), dim3(W), k * W * 12, 0, A);
  timer.stop();
  if (hipMemcpy(cnt, A.cnt, sizeof cnt, hipMemcpyDeviceToHost) != hipSuccess || hipGetLastError() != hipSuccess) return FGO_ENUM;
  g_mn_kernel_ms = timer.ms();

  result->n_points = n_points;
  result->n_out_of_range = cnt[MN_C_OOR];
  result->n_cells = cnt[MN_C_CELLS];
  result->n_valid = cnt[MN_C_VALID];
  result->n_few = cnt[MN_C_FEW];
  result->n_degenerate = cnt[MN_C_DEGENERATE];
  return S.download();
}
