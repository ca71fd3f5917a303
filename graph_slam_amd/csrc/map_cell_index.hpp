// Host side of the cell index of a cloud (map_cell_index.hip): what happens between "keys written" and "index ready", and the one
// radix sort of (64-bit key, 32-bit value) pairs that the map calls use.  Host-only: the kernels see dev::MapCellIndex.
#pragma once
#include "batch_call.hpp"
#include "map_cells_device.hpp"

namespace fgo {

// Stable radix sort of n pairs over the key bits [0, end_bit) on the null stream; `bytes` is what the size query gave.  The size
// query is the same call with scratch == NULL: nothing is sorted and `bytes` becomes the scratch the sort asks for.
int map_sort_pairs(void *scratch, size_t &bytes, unsigned long long *key, unsigned long long *skey, uint32_t *val, uint32_t *sval, size_t n,
                   int end_bit);
inline int map_sort_pairs_bytes(size_t n, int end_bit, size_t &bytes) { return map_sort_pairs(nullptr, bytes, nullptr, nullptr, nullptr, nullptr, n, end_bit); }

// The index of a call in its Staged: seven entries, the six arrays and the scratch.
struct MapCellStage {
  int h[7];
  size_t sort_bytes;
  void *scratch;                                                   // after bind(): max(sort_bytes, min_scratch) bytes, the caller's between builds
  int reserve(Staged &S, size_t n, size_t min_scratch = 0);        // before S.alloc()
  void bind(const Staged &S, dev::MapCellIndex &X);                // after S.alloc(): the device view
  // after the caller's kernel wrote X.Q, X.key and X.idx = 0 .. n - 1: the sort, then the gather of Q into sorted order, which adds
  // the number of run heads -- the occupied cells -- to *run_heads (device); both on the null stream
  int build(const dev::MapCellIndex &X, long long *run_heads);
};

}  // namespace fgo
