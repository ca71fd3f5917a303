// ISAM2 re-eliminates only the cliques on the paths from the affected variables to the root of the Bayes tree; here: only the
// TASKS of the elimination tree on those paths are run again.  Affected = variables that were relinearised + everything that
// shares a factor with them (those factors are re-linearised) + the variables of factors and variables added since the previous
// step.  (isam_dirty.hpp)
#include "isam_dirty.hpp"
#include <cstring>

namespace fgo {

namespace {
struct Marker {
  unsigned char *aff;
  std::vector<int64_t> &set_aff;
  void operator()(int64_t v) const { if (!aff[v]) { aff[v] = 1; set_aff.push_back(v); } }
};
}  // namespace

void isam_mark_added(const IsamFlags &F, const IsamGraph &G, const IsamAdded &A, IsamSets &set) {
  for (int t : set.tasks) F.task_dirty[t] = 0;
  for (int k : set.cols) F.col_dirty[k] = 0;
  for (int64_t v : set.aff) F.affected[v] = 0;
  set.clear();
  const Marker mark{F.affected, set.aff};
  for (int64_t v = A.v0; v < G.N; ++v) mark(v);
  for (int64_t e = A.e0; e < (int64_t)G.ei.size(); ++e) { mark(G.ei[e]); mark(G.ej[e]); }
  for (int64_t f = A.f0; 6 * f < (int64_t)G.imu_ids.size(); ++f) for (int u = 0; u < 6; ++u) mark(G.imu_ids[6 * f + u]);
  for (int64_t q = A.p0; q < (int64_t)G.prior_v.size(); ++q) mark(G.prior_v[q]);
}

int64_t isam_dirty_tasks(const IsamFlags &F, const unsigned char *moved, const IsamGraph &G, IsamSets &set, double full_frac) {
  const Marker mark{F.affected, set.aff};
  auto moved_var = [&](int64_t v) {
    mark(v);
    for (int64_t p = G.he_ptr[v]; p < G.he_ptr[v + 1]; ++p) { const int64_t e = G.he[p] >> 1; mark(G.ei[e]); mark(G.ej[e]); }
    for (int64_t p = G.imu_inc_ptr[v]; p < G.imu_inc_ptr[v + 1]; ++p) { const int64_t f = G.imu_inc[p] >> 3; for (int u = 0; u < 6; ++u) mark(G.imu_ids[6 * f + u]); }
  };
  int64_t v = 0;
  for (; v + 8 <= G.N; v += 8) {                          // (eight flags per load: a settled graph has none set)
    uint64_t wd; std::memcpy(&wd, moved + v, 8);
    if (!wd) continue;
    for (int u = 0; u < 8; ++u) if (moved[v + u]) moved_var(v + u);
  }
  for (; v < G.N; ++v) if (moved[v]) moved_var(v);
  for (size_t q = 0; q < set.aff.size(); ++q)
    for (int k = G.pose_col[set.aff[q]]; k >= 0 && !F.col_dirty[k]; k = G.parent[k]) { F.col_dirty[k] = 1; set.cols.push_back(k); }   // up the elimination tree
  for (size_t q = 0, n0 = set.cols.size(); q < n0; ++q) {
    const int t = G.col_task[set.cols[q]];
    if (!F.task_dirty[t]) { F.task_dirty[t] = 1; set.tasks.push_back(t); }
  }
  const int64_t n_dirty_tasks = (int64_t)set.tasks.size();
  // a task is re-run as a whole: all of its columns take part in the forward solve again
  for (int t : set.tasks)
    for (int q = G.task_ptr[t]; q < G.task_ptr[t + 1]; ++q) { const int k = G.task_cols[q]; if (!F.col_dirty[k]) { F.col_dirty[k] = 1; set.cols.push_back(k); } }
  // when most of the tree is affected (a relinearisation wave after a loop closure) the full sweep is the faster one:
  // the flag look-ups cost every workgroup two extra dependent loads
  const int ntask = (int)G.task_ptr.size() - 1;
  return n_dirty_tasks > (int64_t)(full_frac * ntask) ? -2 : n_dirty_tasks;
}

}  // namespace fgo
