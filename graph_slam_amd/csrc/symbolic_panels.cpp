// Symbolic phase, part 4: panels (tasks that are a path of the elimination tree) with their triangle and row tables, the chunk tables of
// the panel levels, the forward-solve row lists of panel columns, and the leaf levels (symbolic_build.hpp; symbolic.cpp is the driver).
#include <algorithm>
#include <cstdint>
#include <vector>
#include "symbolic_build.hpp"

namespace fgo {
namespace symbolic {

// candidate levels: every task a chain of <= PM columns.  (A level of thousands of one- or two-column tasks -- the
// landmarks of a bundle adjustment: 400k single columns -- is cheaper in the generic one-workgroup-per-task kernel
// than in 1024-thread panel workgroups.)  Only tasks of candidate levels get panel tables.
// -> cand per level; S.task_panel, n_panels, panel_task, prow_ptr
static std::vector<char> number_panels(Symbolic &S) {
  const int nlevels = n_levels(S);
  std::vector<char> cand(nlevels, 0);
  for (int l = 0; l < nlevels; ++l) {
    bool all = S.level_ptr[l + 1] > S.level_ptr[l];
    int maxm = 0;
    for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1] && all; ++t) {
      const int c0 = S.task_ptr[t], m = S.task_ptr[t + 1] - c0;
      maxm = std::max(maxm, m);
      all = m <= PANEL_MAX;
      for (int q = 0; q + 1 < m && all; ++q) all = S.parent[S.task_cols[c0 + q]] == S.task_cols[c0 + q + 1];
    }
    if (all && maxm <= 2 && S.level_ptr[l + 1] - S.level_ptr[l] > 2048) all = false;
    cand[l] = all;
  }
  S.task_panel.assign(n_tasks(S), -1);
  S.prow_ptr.assign(1, 0);
  for (int l = 0; l < nlevels; ++l)
    if (cand[l])
      for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t) {
        const int last = S.task_cols[S.task_ptr[t + 1] - 1];
        S.task_panel[t] = S.n_panels++;
        S.panel_task.push_back(t);
        S.prow_ptr.push_back(S.prow_ptr.back() + (int)(S.colptr[last + 1] - S.colptr[last] - 1));
      }
  return cand;
}

// triangle and row tables of every panel -> S.ptri_blk, prow_idx, prow_blk; panel_ok per panel: it is a proper supernode-like path
static std::vector<char> panel_tables(Symbolic &S) {
  S.ptri_blk.assign(S.tri_off(S.n_panels), -1);
  S.prow_idx.resize((size_t)S.prow_ptr.back());
  S.prow_blk.assign(S.row_off(S.prow_ptr.back()), -1);
  std::vector<char> panel_ok((size_t)S.n_panels, 1);
  parallel_ranges(S.n_panels, 64, [&](int p0, int p1) {
    for (int pn = p0; pn < p1; ++pn) {
      const int t = S.panel_task[pn];
      const int c0 = S.task_ptr[t], m = S.task_ptr[t + 1] - c0;
      const int *cols = S.task_cols.data() + c0;
      const int last = cols[m - 1];
      constexpr int PM = PANEL_MAX;
      int *tri = S.ptri_blk.data() + S.tri_off(pn);
      int64_t covered = 0, total = 0;
      for (int k = 0; k < m; ++k) {
        tri[k * PM + k] = (int)S.colptr[cols[k]];
        ++covered;
        for (int r = k + 1; r < m; ++r) covered += (tri[r * PM + k] = find_blk(S, cols[r], cols[k])) >= 0;
        total += S.colptr[cols[k] + 1] - S.colptr[cols[k]];
      }
      bool nested = true;
      int q = S.prow_ptr[pn];
      for (int64_t p = S.colptr[last] + 1; p < S.colptr[last + 1]; ++p, ++q) {
        const int i = S.rowidx[p];
        S.prow_idx[q] = i;
        int *rb = S.prow_blk.data() + S.row_off(q);
        bool seen = false;
        for (int k = 0; k < m; ++k) {
          const int b = (k == m - 1) ? (int)p : find_blk(S, i, cols[k]);
          if (b >= 0) { seen = true; ++covered; } else if (seen) nested = false;   // must be a suffix k >= start
          rb[k] = b;
        }
      }
      // every block of the panel's columns must be covered by the triangle or the rows; otherwise it is not a
      // proper supernode-like path and its level is left to the generic kernels
      panel_ok[pn] = nested && covered == total;
    }
  });
  return panel_ok;
}

// forward-solve row lists of the panels' columns: [external | in-panel] (disjoint ranges of row_blk / row_col: in parallel)
static void split_panel_row_lists(Symbolic &S, const BuildState &st) {
  parallel_ranges(n_tasks(S), 16, [&](int tb, int te) {
    std::vector<std::pair<int, int>> ext, in;
    for (int t = tb; t < te; ++t) {
      if (S.task_panel[t] < 0 || !S.level_panel[st.tlevel[t]]) continue;
      const int c0 = S.task_ptr[t], m = S.task_ptr[t + 1] - c0;
      for (int q = 0; q < m; ++q) {
        const int k = S.task_cols[c0 + q];
        const int64_t r0 = S.rowptr[k], r1 = S.rowptr[k + 1];
        ext.clear(); in.clear();
        for (int64_t e = r0; e < r1; ++e) {
          const bool inside = S.row_col[e] >= S.task_cols[c0] && std::binary_search(S.task_cols.begin() + c0, S.task_cols.begin() + c0 + m, S.row_col[e]);
          (inside ? in : ext).push_back({S.row_blk[e], S.row_col[e]});
        }
        int64_t w = r0;
        for (auto &x : ext) { S.row_blk[w] = x.first; S.row_col[w] = x.second; ++w; }
        S.row_mid[k] = w;
        for (auto &x : in) { S.row_blk[w] = x.first; S.row_col[w] = x.second; ++w; }
      }
    }
  });
}

// per panel level: row chunks (k_panel_rows / the MFMA row tiles) and forward-solve chunks of its panels
static void panel_chunks(Symbolic &S) {
  const int nlevels = n_levels(S);
  for (int l = 0; l < nlevels; ++l) {
    const bool all = S.level_panel[l];
    if (all)
      for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t) {
        const int pn = S.task_panel[t];
        // panels of one level are numbered consecutively only if earlier levels hold no panel of a mixed level;
        // chunk ranges are stored per panel, so no such assumption is needed
        S.panel_chunk0[pn] = (int)S.pchunk_panel.size();
        for (int r0 = S.prow_ptr[pn]; r0 < S.prow_ptr[pn + 1]; r0 += PANEL_ROWS) {
          S.pchunk_panel.push_back(pn); S.pchunk_row0.push_back(r0);
          S.pchunk_nrows.push_back(std::min(PANEL_ROWS, S.prow_ptr[pn + 1] - r0));
        }
        for (int s0 = 0; s0 < 6 * (S.prow_ptr[pn + 1] - S.prow_ptr[pn]) + 1; s0 += 16 * ROW_SETS) {   // + 1: the right-hand side row
          S.rchunk_panel.push_back(pn); S.rchunk_s0.push_back(s0);
        }
        // forward-solve row lists of the panel's columns: [external | in-panel], external part chunked
        const int c0 = S.task_ptr[t], m = S.task_ptr[t + 1] - c0;
        for (int q = 0; q < m; ++q) {
          const int k = S.task_cols[c0 + q];
          const int64_t r0 = S.rowptr[k];
          S.pcol_fchunk0[S.col_off(pn) + q] = (int)S.fchunk_col.size();
          for (int64_t e = r0; e < S.row_mid[k]; e += FWD_CHUNK) { S.fchunk_col.push_back(k); S.fchunk_e0.push_back(e); }
          S.pcol_fchunkn[S.col_off(pn) + q] = (int)S.fchunk_col.size() - S.pcol_fchunk0[S.col_off(pn) + q];
        }
      }
    S.pchunk_ptr[l + 1] = (int)S.pchunk_panel.size();
    S.fchunk_ptr[l + 1] = (int)S.fchunk_col.size();
    S.rchunk_ptr[l + 1] = (int)S.rchunk_panel.size();
  }
}

// ---- panels
void build_panels(Symbolic &S, const BuildState &st) {
  const int nb = S.nb, nlevels = n_levels(S);
  const std::vector<char> cand = number_panels(S);
  const std::vector<char> panel_ok = panel_tables(S);
  S.level_panel.assign(nlevels, 0);
  S.pchunk_ptr.assign(nlevels + 1, 0);
  S.fchunk_ptr.assign(nlevels + 1, 0);
  S.rchunk_ptr.assign(nlevels + 1, 0);
  S.panel_chunk0.assign(S.n_panels + 1, 0);
  S.pcol_fchunk0.assign(S.col_off(S.n_panels), 0);
  S.pcol_fchunkn.assign(S.col_off(S.n_panels), 0);
  S.row_mid.resize(nb);
  for (int k = 0; k < nb; ++k) S.row_mid[k] = S.rowptr[k + 1];
  for (int l = 0; l < nlevels; ++l) {
    bool all = cand[l];
    for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1] && all; ++t) all = panel_ok[S.task_panel[t]];
    S.level_panel[l] = all;
  }
  split_panel_row_lists(S, st);
  panel_chunks(S);
}

// ---- leaf levels: every task a self-contained light sub-tree (contiguous columns, no external updates, at most
// leaf_blocks blocks) -> k_chol_leaf factors it inside LDS.  Levels of one- or two-column tasks stay on the one-wave
// generic kernel.
void leaf_levels(Symbolic &S) {
  const int nlevels = n_levels(S);
  const int64_t leaf_blocks = leaf_blocks_limit();
  S.level_leaf.assign(nlevels, 0);
  S.level_leaf_maxblk.assign(nlevels, 0);
  S.level_leaf_maxops.assign(nlevels, 0);
  for (int l = 0; l < nlevels; ++l) {
    if (S.level_panel[l] || S.level_ptr[l + 1] == S.level_ptr[l]) continue;
    bool ok = true;
    int maxm = 0;
    int64_t maxblk = 0, maxops = 0;
    for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1] && ok; ++t) {
      const int c0 = S.task_ptr[t], m = S.task_ptr[t + 1] - c0;
      maxm = std::max(maxm, m);
      const int k0 = S.task_cols[c0], k1 = S.task_cols[c0 + m - 1];
      ok = k1 - k0 == m - 1;
      const int64_t b0 = S.colptr[k0], b1 = S.colptr[k1 + 1];
      maxblk = std::max(maxblk, b1 - b0);
      maxops = std::max(maxops, S.op_ptr[b1] - S.op_ptr[b0]);
      ok = ok && b1 - b0 <= leaf_blocks && b1 - b0 < 65536 && S.op_ptr[b1] - S.op_ptr[b0] <= LEAF_OPS;
      for (int64_t u = b0; u < b1 && ok; ++u) ok = S.op_mid[u] == S.op_ptr[u];
    }
    if (ok && maxm > 2) { S.level_leaf[l] = 1; S.level_leaf_maxblk[l] = (int)maxblk; S.level_leaf_maxops[l] = (int)maxops; }
  }
}

}  // namespace symbolic
}  // namespace fgo
