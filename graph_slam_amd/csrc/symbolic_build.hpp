// Phases of build_symbolic (symbolic.cpp is the driver and reads as their list): what each one takes and leaves behind, the little state
// that several of them need, and the helpers they share.  Host only; also built without the HIP headers (tools/symstats.cpp).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "fgo_internal.hpp"

namespace fgo {
namespace symbolic {

// FGO_SYM_PROFILE: the time since the previous lap, on stderr
struct Laps {
  bool on = false;
  double tprev = 0;
  static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  void operator()(const char *what) { if (on) { const double t = now(); std::fprintf(stderr, "[fgo symbolic] %-28s %.1f ms\n", what, 1e3 * (t - tprev)); tprev = t; } }
};

// What more than one phase needs and Symbolic does not hold.  Everything else is local to its phase.
struct BuildState {
  // symbolic_schedule.cpp column_work(): work(k) ~ block operations needed to finish column k; sub = work summed over the sub-tree of k; subblk = blocks of L in
  // the sub-tree of k; height of the sub-tree
  std::vector<int64_t> work, sub, subblk;
  std::vector<int> height;
  // assign_tasks() numbers the tasks as it meets them; bucket_tasks() renumbers task_of and tlevel ONCE to the final ids, those of
  // S.task_ptr / S.level_ptr.  Every phase after "tasks and levels" sees the final ids only.
  std::vector<int> task_of;          // nb: task of a column
  std::vector<int> tlevel;           // per task: its schedule level (distributed: its segment, dependency level x (world + 1) + group)
  // first column of the distributed top (nb when world == 1), = S.dom_col0[world]: set by build_symbolic after decompose_domains(), for ext_ops()
  int top_col0 = 0;
};

inline int n_tasks(const Symbolic &S) { return (int)S.task_ptr.size() - 1; }
inline int n_levels(const Symbolic &S) { return (int)S.level_ptr.size() - 1; }

// ---- helpers
// group of column k -- 0 .. world-1: a rank's domain, world: the top
inline int group_of(const Symbolic &S, int k) {
  if (S.world == 1) return 0;
  return (int)(std::upper_bound(S.dom_col0.begin(), S.dom_col0.begin() + S.world + 1, k) - S.dom_col0.begin()) - 1;
}
// Update lists are generated per TARGET column k (no shared cursors, so the columns are spread over host threads
// and the result does not depend on the thread count): for every source column j of row k (ascending j) walk
// pattern(j) from row k downwards -- it is a subset of {k} U pattern(k) -- and merge it against column k.
//   fn(u, t, s): target block u (in column k)  -=  L[t] * L[s]^T,  t and s in column j, s = block (k, j)
// (a template over its callable: the inner loop of two parallel passes)
template <class F>
inline void for_each_op_of_column(const Symbolic &S, int k, F &&fn) {
  const int64_t k0 = S.colptr[k];
  for (int64_t e = S.rowptr[k]; e < S.rowptr[k + 1]; ++e) {
    const int64_t s = S.row_blk[e], c1 = S.colptr[S.row_col[e] + 1];
    int64_t u = k0;
    for (int64_t t = s; t < c1; ++t) {
      const int i = S.rowidx[t];
      while (S.rowidx[u] != i) ++u;
      fn(u, t, s);
    }
  }
}
// external updates of block b that its level's accumulate applies, the LAST ext_ops(b) entries of [op_ptr[b], op_mid[b])
// (multi-GPU: a top block's domain-sourced updates arrive through the collective; only its top-sourced external
//  updates -- the tail of the ascending list -- are left to the accumulate kernel)
inline int64_t ext_ops(const Symbolic &S, const BuildState &st, int64_t b) {
  if (S.blkcol[b] < st.top_col0) return S.op_mid[b] - S.op_ptr[b];
  int64_t o = S.op_mid[b];
  while (o > S.op_ptr[b] && S.blkcol[S.op_a[o - 1]] >= st.top_col0) --o;
  return S.op_mid[b] - o;
}
// block id of (row, col), row > col, or -1
inline int find_blk(const Symbolic &S, int row, int col) {
  const int *b = S.rowidx.data() + S.colptr[col] + 1, *e = S.rowidx.data() + S.colptr[col + 1];
  const int *p = std::lower_bound(b, e, row);
  return (p != e && *p == row) ? (int)(p - S.rowidx.data()) : -1;
}
// blocks of L a light sub-tree may have: it must fit the leaf kernel's LDS (LEAF_BLOCKS blocks of L per workgroup)
inline int64_t leaf_blocks_limit() {
  static const int64_t leaf_blocks = (int64_t)tune("leaf_blocks", LEAF_BLOCKS);
  return leaf_blocks;
}

// ---- phases, in the order build_symbolic calls them
// symbolic_pattern.cpp
// in: graph, order.  out: pm = the order post-ordered along its elimination tree, par = that tree under pm
void etree_postorder(const BlockGraph &g, const std::vector<int> &perm, std::vector<int> &pm, std::vector<int> &par);
// in: graph, order pm, its elimination tree if known (nullptr: not known, serial pass).  out: pat[k] = pattern of column k below the diagonal;
// S.perm, iperm, parent, colptr, max_col_blocks
void pattern_pass(const BlockGraph &g, const std::vector<int> &pm, const std::vector<int> *par, std::vector<std::vector<int>> &pat, Symbolic &S, bool prof);
// in: S.world, the pattern pass of the post-order.  out: S.dom_col0; world > 1: the columns re-ordered [domains | top] and the pattern pass redone
void decompose_domains(const BlockGraph &g, std::vector<std::vector<int>> &pat, Symbolic &S, bool prof);
// in: pat (emptied), S.colptr, rowidx / blkcol sized to nnzL.  out: S.rowidx, blkcol
void fill_columns(std::vector<std::vector<int>> &pat, Symbolic &S);
// in: columns.  out: S.rowptr, row_blk, row_col
void build_row_lists(Symbolic &S);
// in: columns, row lists.  out: S.op_ptr, nops
void count_update_ops(Symbolic &S);

// symbolic_schedule.cpp
// in: columns, op counts, the two work limits.  out: S.etree_height, seg_group, level_ptr, task_ptr, task_cols; st.work .. st.tlevel (final ids)
void build_schedule(Symbolic &S, int64_t task_work_limit, int64_t chain_work_limit, BuildState &st);

// symbolic_lists.cpp
// in: op counts, st.task_of.  out: S.op_a, op_b, op_mid
void fill_update_lists(Symbolic &S, const BuildState &st);
// in: update lists, schedule.  out: S.acc_ptr, acc_targets, acc_mid; FGO_TUNE=acc_stats=1: the per-level statistics on stderr
void accumulate_targets(Symbolic &S, const BuildState &st);
// in: accumulate targets.  out: S.g2_lvl, g2_tgt, g2_ptr, g2_b, g2_a
void column_group_lists(Symbolic &S, const BuildState &st);

// symbolic_panels.cpp
// in: schedule, columns, row lists.  out: S.task_panel .. prow_blk, level_panel, the p/r/f chunk tables, row_mid; row_blk / row_col of panel
// columns re-ordered [external | in-panel]
void build_panels(Symbolic &S, const BuildState &st);
// in: level_panel, update lists.  out: S.level_leaf, level_leaf_maxblk, level_leaf_maxops
void leaf_levels(Symbolic &S);

// symbolic_riders.cpp
// in: everything above.  out: S.ride_items, ride_ptr, n_scratch, acc_start; op_a / op_b of the candidate targets re-ordered by source level
// (hub targets: their ridden part copied behind the lists), acc_targets / acc_mid of the candidate levels re-split
void build_riders(Symbolic &S, const BuildState &st, Laps &lap);

}  // namespace symbolic
}  // namespace fgo
