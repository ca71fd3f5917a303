// The cell index of a point cloud on the MI355X (gfx950, 64-bit integers, wave64), shared by map cleaning and map normals, and the
// radix sort that map fusion orders its voxels with: rocPRIM's radix_sort_pairs is instantiated here and nowhere else.
// The sort of the (cell key, input index) pairs runs over all 64 key bits and is stable, so a cell's run is in ascending input index;
// the out-of-range mark is the largest key and sorts behind every cell.  The gather is integer work; it strides beyond its capped grid.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "map_cell_index.hpp"
#include "small_dense_device.hpp"

namespace fgo {
namespace {

constexpr int MI_T = 256;                        // threads of a workgroup

__global__ __launch_bounds__(MI_T) void k_map_cells_gather(dev::MapCellIndex X, long long *run_heads) {
  const int64_t stride = (int64_t)gridDim.x * MI_T;
  for (int64_t s = (int64_t)blockIdx.x * MI_T + threadIdx.x; s < X.n; s += stride) {
    const unsigned long long key = X.skey[s];
    if (key == dev::MAP_CELL_EMPTY) continue;
    const int64_t p = X.sidx[s];
#pragma unroll
    for (int k = 0; k < 3; ++k) X.sQ[3 * s + k] = X.Q[3 * p + k];
    if (s == 0 || X.skey[s - 1] != key) dev::wave_count(run_heads);
  }
}

}  // namespace

int map_sort_pairs(void *scratch, size_t &bytes, unsigned long long *key, unsigned long long *skey, uint32_t *val, uint32_t *sval, size_t n,
                   int end_bit) {
  return rocprim::radix_sort_pairs(scratch, bytes, key, skey, val, sval, n, 0, end_bit, 0) == hipSuccess ? FGO_OK : FGO_ENUM;
}

int MapCellStage::reserve(Staged &S, size_t n, size_t min_scratch) {
  if (int rc = map_sort_pairs_bytes(n, 64, sort_bytes)) return rc;
  const size_t q = 3 * n * sizeof(long long), k = n * sizeof(unsigned long long), i = n * sizeof(uint32_t);
  const size_t bytes[7] = {q, q, k, k, i, i, sort_bytes > min_scratch ? sort_bytes : min_scratch};      // Q sQ key skey idx sidx scratch
  for (int k = 0; k < 7; ++k) h[k] = S.out(nullptr, bytes[k], true);
  return FGO_OK;
}

void MapCellStage::bind(const Staged &S, dev::MapCellIndex &X) {
  X.Q = S.ptr<long long>(h[0]); X.sQ = S.ptr<long long>(h[1]); X.key = S.ptr<unsigned long long>(h[2]); X.skey = S.ptr<unsigned long long>(h[3]);
  X.idx = S.ptr<uint32_t>(h[4]); X.sidx = S.ptr<uint32_t>(h[5]); scratch = S.ptr<void>(h[6]);
}

int MapCellStage::build(const dev::MapCellIndex &X, long long *run_heads) {
  if (int rc = map_sort_pairs(scratch, sort_bytes, X.key, X.skey, X.idx, X.sidx, (size_t)X.n, 64)) return rc;
  hipLaunchKernelGGL(k_map_cells_gather, dim3(grid_for((unsigned long long)X.n, MI_T)), dim3(MI_T), 0, 0, X, run_heads);
  return FGO_OK;
}

}  // namespace fgo
