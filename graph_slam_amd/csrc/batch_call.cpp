// The one setting of the plumbing in batch_call.hpp: the largest grid grid_for() hands out.  The default never changes; the
// development hook lowers it so that a test of a few seconds runs the capped-grid kernels past their grid.
#include "batch_call.hpp"

namespace fgo {
namespace {
unsigned g_grid_cap = GRID_CAP_DEFAULT;
}  // namespace
unsigned grid_cap() { return g_grid_cap; }
}  // namespace fgo

extern "C" int fgo_debug_grid_cap(int cap) {
  if (cap == 0) fgo::g_grid_cap = fgo::GRID_CAP_DEFAULT;
  else if (cap >= 1 && (unsigned)cap <= fgo::GRID_CAP_DEFAULT) fgo::g_grid_cap = (unsigned)cap;
  return (int)fgo::g_grid_cap;
}
