// Symbolic phase of the block Cholesky (host, once per graph structure): block elimination tree,
// block column patterns of L, left-looking update lists, row lists for the triangular solves and
// the task/level schedule the device kernels follow.  Replaces what g2o does in
// BlockSolver::buildStructure + LinearSolverCSparse's symbolic decomposition ([UPSTREAM], reached
// from the reference at g2o/g2o_graph.cpp:246-249 on iteration 0 of every optimize() call).
//
// This file is the driver: the list of phases.  What each phase takes and leaves behind is stated in symbolic_build.hpp, the phases
// themselves are in symbolic_pattern.cpp, _schedule.cpp, _lists.cpp, _panels.cpp and _riders.cpp.
#include <cstdlib>
#include <vector>
#include "symbolic_build.hpp"

namespace fgo {

void build_symbolic(const BlockGraph &g, const std::vector<int> &perm, int64_t task_work_limit, int64_t chain_work_limit, Symbolic &S, int world, bool analyse_only) {
  using namespace symbolic;
  const int nb = g.n;
  Laps lap{std::getenv("FGO_SYM_PROFILE") != nullptr, Laps::now()};
  S = Symbolic();
  S.nb = nb;
  if (world < 1) world = 1;
  S.world = world;
  BuildState st;
  std::vector<std::vector<int>> pat(nb);                    // pattern of every column below the diagonal, until fill_columns() has stored it
  {
    std::vector<int> pm, par;
    etree_postorder(g, perm, pm, par);
    lap("  etree + post-order");
    pattern_pass(g, pm, &par, pat, S, lap.on);
  }
  decompose_domains(g, pat, S, lap.on);
  st.top_col0 = S.dom_col0[world];
  S.nnzL = S.colptr[nb];
  S.rowidx.resize(S.nnzL);
  S.blkcol.resize(S.nnzL);
  lap("  patterns");
  fill_columns(pat, S);
  lap("column patterns");
  build_row_lists(S);
  lap("row lists");
  count_update_ops(S);
  lap("update lists: count");
  build_schedule(S, task_work_limit, chain_work_limit, st);
  lap("tasks and levels");
  if (analyse_only) return;                 // S.nops, S.nnzL and the levels are known: what an ordering candidate is ranked by
  fill_update_lists(S, st);
  lap("update lists: fill");
  accumulate_targets(S, st);
  lap("accumulate targets");
  column_group_lists(S, st);
  lap("column-group lists (acc2)");
  build_panels(S, st);
  lap("panels, chunks");
  leaf_levels(S);
  lap("leaf levels");
  build_riders(S, st, lap);
  lap("riders");
}

}  // namespace fgo
