// What the translation units of the optimiser's device path share (gfx950, f64, wave64) -- kernels.hip (graph side: linearisation, chi2,
// update, utility kernels), kernels_factor.hip (factor sweep, launch_factor), kernels_solve.hip (triangular solves, launch_solve) -- and
// nothing that only one of them uses.  The cross-phase CONSTANTS are in device_plan.hpp (operand-tile layout of ptop) and fgo_internal.hpp
// (RIDE_PER_WG, beside PANEL_MAX / PANEL_ROWS / ROW_SETS), the launch thresholds in launch_select.cpp.
//
//   who uses what                            kernels.hip   kernels_factor.hip   kernels_solve.hip
//   WAVE                                          x                                    x
//   PM                                                             x                   x
//   Row6, load_row                                                 x                   x
//   store_row (load_row's other half)                              x
//   task_runs                                                      x                   x
//   cdiv                                          x                x
//   FGO_LAUNCH                                                     x                   x
//   FGO_LAUNCH_N (its form with an item count)                     x
//   seg_runs                                                       x                   x
//   launch_fwd_level (kernels_solve.hip)                           x                   x
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "device_plan.hpp"
#include "fgo_internal.hpp"

namespace fgo {

#define WAVE 64
constexpr int PM = PANEL_MAX;

// ------------------------------------------------------------------------------------------------
// Block Cholesky.  L blocks are 6x6 row-major (row = later-eliminated pose).
// Lane mapping ("row per lane"): lane = 6 g + r owns ROW r of the target block handled by lane group g
// (10 groups per wave, lanes 60..63 idle).  One update L_t -= L_a L_b^T costs a lane 3 + 18 16-byte loads
// (its row of L_a, all of L_b; the 6 lanes of a group read the same L_b lines) for 36 FMAs, needs no
// cross-lane traffic, and the row stays in registers through the diagonal Cholesky and the TRSM.
struct Row6 { double v[6]; };

__device__ __forceinline__ Row6 load_row(const double *__restrict__ p) {
  const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2),
                c = *reinterpret_cast<const double2 *>(p + 4);
  return {{a.x, a.y, b.x, b.y, c.x, c.y}};
}
__device__ __forceinline__ void store_row(double *__restrict__ p, const Row6 &x) {
  *reinterpret_cast<double2 *>(p) = make_double2(x.v[0], x.v[1]);
  *reinterpret_cast<double2 *>(p + 2) = make_double2(x.v[2], x.v[3]);
  *reinterpret_cast<double2 *>(p + 4) = make_double2(x.v[4], x.v[5]);
}

// partial re-factorisation: is this task part of the sweep?  (task_dirty == NULL: everything is)
__device__ __forceinline__ bool task_runs(const DevPlan &P, int task) { return !P.task_dirty || P.task_dirty[task]; }

// ------------------------------------------------------------------------------------------------
// host side of the launchers (no synchronisation, capturable)
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// a launch, or (census) its record: launch_factor / launch_fwd_level / launch_solve are walked unchanged by fgo_debug_launch_census
#define FGO_LAUNCH(cz, form, grid, ...) do { if (cz) (cz)->add((form), (int64_t)(grid)); else hipLaunchKernelGGL(__VA_ARGS__); } while (0)
#define FGO_LAUNCH_N(cz, form, grid, items, ...) do { if (cz) (cz)->add((form), (int64_t)(grid), (int64_t)(items)); else hipLaunchKernelGGL(__VA_ARGS__); } while (0)

// does segment l belong to this pass of the sweep?  (phase: device_plan.hpp PHASE_*)
static inline bool seg_runs(const HostSchedule &H, int l, int phase) {
  if (H.level_ptr[l + 1] == H.level_ptr[l]) return false;            // empty segment
  if (phase == PHASE_ALL) return true;
  const int gq = H.seg_group[l];
  return phase == PHASE_DOMAIN ? gq == H.rank : gq == H.world;
}

// generic forward kernel of a non-panel level (kernels_solve.hip): launch_factor runs it behind the level's factor kernel when the
// forward solve is fused into the sweep, launch_solve in the stand-alone forward solve
void launch_fwd_level(const DevPlan &P, const HostSchedule &H, const double *Lv, double *x, int l, hipStream_t s, LaunchCensus *cz);

}  // namespace fgo
