// Symbolic phase, part 2: the schedule -- columns into tasks, tasks into dependency levels (distributed: segments), and the final
// numbering of the tasks by level (symbolic_build.hpp; symbolic.cpp is the driver).
#include <algorithm>
#include <cstdint>
#include <vector>
#include "symbolic_build.hpp"

namespace fgo {
namespace symbolic {

// work(k) ~ block operations needed to finish column k.
static void column_work(Symbolic &S, BuildState &st) {
  const int nb = S.nb;
  st.work.resize(nb); st.sub.resize(nb);
  for (int k = 0; k < nb; ++k) {
    const int64_t c0 = S.colptr[k], c1 = S.colptr[k + 1];
    st.work[k] = (S.op_ptr[c1] - S.op_ptr[c0]) + 2 * (c1 - c0);
    st.sub[k] = st.work[k];
  }
  st.height.assign(nb, 0);
  st.subblk.resize(nb);                 // blocks of L in the sub-tree of k
  for (int k = 0; k < nb; ++k) st.subblk[k] = S.colptr[k + 1] - S.colptr[k];
  for (int k = 0; k < nb; ++k) {
    const int p = S.parent[k];
    if (p >= 0) { st.sub[p] += st.sub[k]; st.subblk[p] += st.subblk[k]; st.height[p] = std::max(st.height[p], st.height[k] + 1); }
    S.etree_height = std::max(S.etree_height, st.height[k] + 1);
  }
}

// task id per column: maximal subtrees with sub <= limit become one task; above that, chains of
// columns with a single "heavy" child continue the child's task when the work is small.
// -> st.task_of (ids in the order the tasks are met); returns the number of tasks
static int assign_tasks(const Symbolic &S, int64_t task_work_limit, int64_t chain_work_limit, BuildState &st) {
  const int nb = S.nb, world = S.world;
  const std::vector<int64_t> &work = st.work, &sub = st.sub, &subblk = st.subblk;
  const std::vector<int> &height = st.height;
  std::vector<int> &task_of = st.task_of;
  task_of.assign(nb, -1);
  int ntask = 0;
  // subtree tasks: a column k is "light" if sub[k] <= limit.  Root of a light subtree = light column
  // whose parent is heavy (or none).
  std::vector<char> light(nb);
  // ... and fits the leaf kernel's LDS (LEAF_BLOCKS blocks of L per workgroup)
  const int64_t leaf_blocks = leaf_blocks_limit();
  for (int k = 0; k < nb; ++k)
    light[k] = sub[k] <= task_work_limit && subblk[k] <= leaf_blocks && sub[k] - 2 * subblk[k] <= LEAF_OPS && (world == 1 || k < S.dom_col0[world]);
  // children are numbered below parents, so a reverse sweep propagates the task id downwards
  for (int k = nb - 1; k >= 0; --k) {
    if (!light[k]) continue;
    const int p = S.parent[k];
    if (p >= 0 && light[p]) task_of[k] = task_of[p];
    else task_of[k] = ntask++;
  }
  // heavy columns: extend the task of a heavy only-child chain while the accumulated work is small
  std::vector<int64_t> task_work;
  std::vector<int> task_heavy_cols, heavy_children, last_heavy_child, tl, ch_m1, ch_m2, ch_arg;
  task_work.assign(ntask, 0);
  task_heavy_cols.assign(ntask, 0);
  // A column with several heavy children (the first column of a separator) continues the panel of its TALLEST heavy child
  // when that panel has room: a separator's last, partly filled panel and the head of the parent separator then share a
  // level instead of taking one each (the other children's updates arrive through the accumulate like any external
  // source).  FGO_MERGE_MULTI=0 restores the only-child rule.
  static const bool merge_multi = tune("merge_multi", 1) != 0;
  // WHICH child: the one whose task sits on the highest LEVEL so far (ties: the tallest sub-tree) -- continuing the panel on
  // the critical path saves a level, continuing a taller but lower-levelled one does not (by_level = 0: the tallest, as before).
  static const bool by_level = tune("merge_by_level", 1) != 0;
  heavy_children.assign(nb, 0); last_heavy_child.assign(nb, -1);
  tl.assign((size_t)ntask, 0);                                 // task levels as the sweep sees them (light sub-trees: 0)
  ch_m1.assign(nb, -1); ch_m2.assign(nb, -1); ch_arg.assign(nb, -1);   // per column: highest / second highest level among its children's tasks, a child at the highest
  auto note_child = [&](int p, int k, int lv) {                 // child k (task level lv) of p
    if (lv > ch_m1[p]) { ch_m2[p] = ch_m1[p]; ch_m1[p] = lv; ch_arg[p] = k; }
    else if (lv > ch_m2[p]) ch_m2[p] = lv;
  };
  for (int k = 0; k < nb; ++k) {
    const int p = S.parent[k];
    if (light[k]) { if (p >= 0 && !light[p]) note_child(p, k, 0); continue; }
    int t = -1, lv_new = ch_m1[k] + 1;
    if (heavy_children[k] == 1 || (merge_multi && heavy_children[k] > 1)) {
      const int c = last_heavy_child[k];
      const int tc = task_of[c];
      if (task_work[tc] + work[k] <= chain_work_limit && task_heavy_cols[tc] < PANEL_MAX && group_of(S, c) == group_of(S, k)) {
        t = tc;
        const int others = ch_arg[k] == c ? ch_m2[k] : ch_m1[k];      // (several children at the top level: m2 == m1 is noted as m2)
        lv_new = std::max(tl[tc], others + 1);
      }
    }
    if (t < 0) { t = ntask++; task_work.push_back(0); task_heavy_cols.push_back(0); tl.push_back(0); }
    task_of[k] = t;
    task_work[t] += work[k];
    task_heavy_cols[t]++;
    tl[t] = std::max(tl[t], lv_new);
    if (p >= 0) {
      heavy_children[p]++;
      const int q = last_heavy_child[p];
      const bool better = q < 0 || (by_level ? (tl[t] > tl[task_of[q]] || (tl[t] == tl[task_of[q]] && height[k] >= height[q])) : height[k] >= height[q]);
      if (better) last_heavy_child[p] = k;
      note_child(p, k, tl[t]);
    }
  }
  return ntask;
}

// levels: level(T) = 1 + max level of tasks owning children of T's columns
// -> st.tlevel, S.seg_group; returns the number of levels (distributed: of segments)
static int level_tasks(Symbolic &S, int ntask, BuildState &st) {
  const int nb = S.nb, world = S.world;
  const std::vector<int> &task_of = st.task_of;
  std::vector<int> &tlevel = st.tlevel;
  tlevel.assign(ntask, 0);
  for (int k = 0; k < nb; ++k) {          // ascending: children first
    const int p = S.parent[k];
    if (p < 0) continue;
    const int tk = task_of[k], tp = task_of[p];
    if (tk != tp) tlevel[tp] = std::max(tlevel[tp], tlevel[tk] + 1);
    else tlevel[tp] = std::max(tlevel[tp], tlevel[tk]);
  }
  // NOTE: a task's level can be raised after one of its earlier columns was visited; since the level is a
  // property of the task (max over all its columns' children) and parents are visited after children,
  // a second sweep makes it consistent.
  for (int pass = 0; pass < 2; ++pass)
    for (int k = 0; k < nb; ++k) {
      const int p = S.parent[k];
      if (p < 0) continue;
      const int tk = task_of[k], tp = task_of[p];
      if (tk != tp) tlevel[tp] = std::max(tlevel[tp], tlevel[tk] + 1);
    }
  int nlevels = 0;
  for (int t = 0; t < ntask; ++t) nlevels = std::max(nlevels, tlevel[t] + 1);
  // multi-GPU: a schedule "level" below is a SEGMENT = (dependency level, group); a rank runs the segments of its own
  // group, then -- after the collective -- those of the top, both in ascending level order
  if (world > 1) {
    std::vector<int> tgroup(ntask, 0);
    for (int k = 0; k < nb; ++k) tgroup[task_of[k]] = group_of(S, k);
    const int G = world + 1;
    for (int t = 0; t < ntask; ++t) tlevel[t] = tlevel[t] * G + tgroup[t];
    nlevels *= G;
    S.seg_group.resize(nlevels);
    for (int l = 0; l < nlevels; ++l) S.seg_group[l] = l % G;
  } else {
    S.seg_group.assign(nlevels, 0);
  }
  return nlevels;
}

// bucket tasks by level, columns by task (ascending column order inside a task).  The tasks take their FINAL ids here -- the position in
// the level buckets -- and st.task_of / st.tlevel are renumbered to them: nothing later sees the ids of assign_tasks().
static void bucket_tasks(Symbolic &S, int ntask, int nlevels, BuildState &st) {
  const int nb = S.nb;
  std::vector<int> tcount(ntask, 0);
  for (int k = 0; k < nb; ++k) tcount[st.task_of[k]]++;
  std::vector<int> order(ntask), lcount(nlevels + 1, 0);
  for (int t = 0; t < ntask; ++t) lcount[st.tlevel[t] + 1]++;
  for (int l = 0; l < nlevels; ++l) lcount[l + 1] += lcount[l];
  S.level_ptr = lcount;
  {
    std::vector<int> fill(lcount.begin(), lcount.end() - 1);
    for (int t = 0; t < ntask; ++t) order[t] = fill[st.tlevel[t]]++;   // new index of task t
  }
  S.task_ptr.assign(ntask + 1, 0);
  for (int t = 0; t < ntask; ++t) S.task_ptr[order[t] + 1] = tcount[t];
  for (int t = 0; t < ntask; ++t) S.task_ptr[t + 1] += S.task_ptr[t];
  for (int k = 0; k < nb; ++k) st.task_of[k] = order[st.task_of[k]];
  for (int l = 0; l < nlevels; ++l) for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t) st.tlevel[t] = l;
  S.task_cols.resize(nb);
  {
    std::vector<int> fill(S.task_ptr.begin(), S.task_ptr.end() - 1);
    for (int k = 0; k < nb; ++k) S.task_cols[fill[st.task_of[k]]++] = k;
  }
}

void build_schedule(Symbolic &S, int64_t task_work_limit, int64_t chain_work_limit, BuildState &st) {
  column_work(S, st);
  const int ntask = assign_tasks(S, task_work_limit, chain_work_limit, st);
  const int nlevels = level_tasks(S, ntask, st);
  bucket_tasks(S, ntask, nlevels, st);
}

}  // namespace symbolic
}  // namespace fgo
