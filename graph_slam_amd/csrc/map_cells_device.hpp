// What the kernels that work on a cloud cut into cells share (kernels_map_clean.hip, kernels_map_normals.hip; gfx950, 64-bit
// integers): the quantum, floor division of a quantised coordinate, the 3 x 21 bit cell key and the lookup of a key in the sorted
// keys.  Which points are in range is each caller's rule; the key of a point that is not is MAP_CELL_EMPTY, the largest key there
// is, so that it sorts behind every cell.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fgo {
namespace dev {

constexpr long long MAP_CELL_BIAS = 1ll << 20;                // a cell coordinate c is stored as c + 2^20 in 21 bits
constexpr unsigned long long MAP_CELL_EMPTY = ~0ull;
constexpr double MAP_QUANTA_PER_M = 1048576.0;                // 2^20: the quantum is 2^-20 m

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

}  // namespace dev
}  // namespace fgo
