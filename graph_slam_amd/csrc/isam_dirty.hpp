// The host side of a partial ISAM2 update (fgo_isam2.cpp): the pinned flag arrays and the walk from the affected variables up
// the elimination tree.  Host-only (no HIP, std types): tools/isam_dirty_check.cpp drives it stand-alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fgo {

// The flag arrays of an ISAM2 context, one pinned allocation.  isam_flags() is the only place that lays it out.
struct IsamFlags {
  unsigned char *moved = nullptr;       // [NX] variables this update's relinearisation moved (copied from the device)
  unsigned char *task_dirty = nullptr;  // [ntask] tasks this update re-runs
  unsigned char *col_dirty = nullptr;   // [nb] their columns
  unsigned char *moved_next = nullptr;  // [NX] look-ahead: variables the NEXT update's relinearisation will move
  unsigned char *affected = nullptr;    // [NX] variables whose factors are linearised again
  size_t bytes = 0;                     // of the whole allocation
};
inline IsamFlags isam_flags(unsigned char *base, int64_t NX, int ntask, int nb) {   // base == nullptr: the byte count only
  IsamFlags f;
  auto take = [&](size_t n) { unsigned char *p = base ? base + f.bytes : nullptr; f.bytes += n; return p; };
  f.moved = take((size_t)NX); f.task_dirty = take((size_t)ntask); f.col_dirty = take((size_t)nb);
  f.moved_next = take((size_t)NX); f.affected = take((size_t)NX);
  return f;
}

// task_dirty, col_dirty and affected are all-zero between updates: an update remembers the entries it sets and the next one
// clears exactly those, so the host side of an update is O(affected), not O(graph), apart from one pass over `moved`
struct IsamSets {
  std::vector<int> tasks, cols;
  std::vector<int64_t> aff;
  void clear() { tasks.clear(); cols.clear(); aff.clear(); }
};

struct IsamGraph {                      // what the walk reads of the graph and its structure
  int64_t N;                            // variables (slots beyond N are phantom: never flagged)
  const std::vector<int> &ei, &ej;      // binary factors
  const std::vector<int> &imu_ids;      // 6 variables per IMU factor
  const std::vector<int> &prior_v;
  const std::vector<int64_t> &he_ptr;   // incidence CSRs per variable: he[p] >> 1 = binary factor, imu_inc[p] >> 3 = IMU factor
  const std::vector<int> &he;
  const std::vector<int64_t> &imu_inc_ptr;
  const std::vector<int> &imu_inc;
  const std::vector<int> &pose_col;     // column of a variable, -1: fixed
  const std::vector<int> &parent;       // elimination tree over the columns, -1: root
  const std::vector<int> &col_task, &task_ptr, &task_cols;
};
struct IsamAdded { int64_t v0, e0, f0, p0; };   // variables / binary / IMU / prior factors the previous update already knew

// Clears what the previous update set, then marks the added variables and the variables of the added factors.  Does not read `moved`.
void isam_mark_added(const IsamFlags &F, const IsamGraph &G, const IsamAdded &A, IsamSets &set);
// Then, once moved[0 .. N) is on the host: affected += moved + everything that shares a factor with a moved variable; dirty columns =
// the ancestors of the affected; dirty tasks = their tasks; dirty columns closed over whole tasks.  Returns the number of dirty
// tasks, or -2 (flags set all the same) when they are more than full_frac of all: the full sweep is the faster one then.
int64_t isam_dirty_tasks(const IsamFlags &F, const unsigned char *moved, const IsamGraph &G, IsamSets &set, double full_frac);

}  // namespace fgo
