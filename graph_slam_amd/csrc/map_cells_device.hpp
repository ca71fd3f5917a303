// What the kernels that work on a cloud cut into cells share (kernels_map_fuse.hip, kernels_map_clean.hip, kernels_map_normals.hip
// and the index build of map_cell_index.hip; gfx950, 64-bit integers): the quantum and the quantisation of a coordinate, floor
// division of a quantised coordinate, the 3 x 21 bit cell key and its decoding, the lookup of a key in the sorted keys and the
// device view of a cell index.  Which points are in range is each caller's rule; the key of a point that is not is MAP_CELL_EMPTY,
// the largest key there is, so that it sorts behind every cell.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fgo {
namespace dev {

constexpr long long MAP_CELL_BIAS = 1ll << 20;                // a cell coordinate c is stored as c + 2^20 in 21 bits
constexpr unsigned long long MAP_CELL_EMPTY = ~0ull;
constexpr double MAP_QUANTA_PER_M = 1048576.0;                // 2^20: the quantum is 2^-20 m

// One coordinate in quanta: Q = llrint(x 2^20), ties to even.  False and Q = 0 unless |x 2^20| < bound, which a NaN fails too: the
// caller's bound (at most 2^63) keeps llrint defined and says how far its own range test has to look.  Contraction is off.
__device__ __forceinline__ bool map_quantise(double x, double bound, long long &Q) {
#pragma clang fp contract(off)
  const double y = x * MAP_QUANTA_PER_M;
  const bool ok = fabs(y) < bound;
  Q = ok ? llrint(y) : 0;
  return ok;
}
// floor(Q / T) for T > 0: Q = -1 is in cell -1
__device__ __forceinline__ long long map_floor_div(long long Q, long long T) {
  long long q = Q / T;
  if (Q - q * T < 0) --q;
  return q;
}
// the key of the cell with the BIASED coordinates e_k = c_k + 2^20 in [0, 2^21)
__device__ __forceinline__ unsigned long long map_cell_key(long long e0, long long e1, long long e2) {
  return ((unsigned long long)e2 << 42) | ((unsigned long long)e1 << 21) | (unsigned long long)e0;
}
// the biased coordinate e_a, a = 0, 1, 2, of a key that is not MAP_CELL_EMPTY
__device__ __forceinline__ long long map_cell_coord(unsigned long long key, int a) {
  return (long long)(a == 2 ? key >> 42 : (key >> (21 * a)) & 0x1fffff);
}
// the first s in [0, n] with skey[s] >= key, by binary search of the sorted keys: neighbouring lanes look for neighbouring cells,
// so the upper levels of the search stay in cache
__device__ __forceinline__ int64_t map_key_lower_bound(const unsigned long long *__restrict__ skey, int64_t n, unsigned long long key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (skey[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the cell index of a cloud of n points as a kernel sees it; map_cell_index.hpp builds it
struct MapCellIndex {
  int64_t n;
  long long *Q, *sQ;                             // n x 3: in input order, in sorted order
  unsigned long long *key, *skey;                // in input order (what says "in range" from the sort on), sorted
  uint32_t *idx, *sidx;
};

}  // namespace dev
}  // namespace fgo
