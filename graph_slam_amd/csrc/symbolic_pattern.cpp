// Symbolic phase, part 1: elimination tree and post-order, column patterns of L, multi-GPU domain decomposition, the columns and row lists
// of L and the number of updates per block (symbolic_build.hpp; symbolic.cpp is the driver).
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "symbolic_build.hpp"

namespace fgo {
namespace symbolic {

// Post-order the elimination tree (same fill, same tree): every sub-tree becomes a contiguous column range, so a
// light sub-tree's blocks are one contiguous range of L and the leaf kernel can keep them in LDS under local
// indices.  Children keep their relative order; the nested-dissection order is nearly post-ordered already.
// The tree comes from the graph alone (Liu's algorithm: ancestors with path compression) -- no column patterns
// needed -- so the (serial) pattern pass runs once, on the final order.
void etree_postorder(const BlockGraph &g, const std::vector<int> &perm, std::vector<int> &pm, std::vector<int> &par2) {
  const int nb = g.n;
  std::vector<int> ip(nb), par(nb, -1), anc(nb, -1);
  for (int k = 0; k < nb; ++k) ip[perm[k]] = k;
  for (int k = 0; k < nb; ++k) {
    const int v = perm[k];
    for (int p = g.xadj[v]; p < g.xadj[v + 1]; ++p) {
      int r = ip[g.adj[p]];
      if (r >= k) continue;
      while (anc[r] != -1 && anc[r] != k) { const int nx = anc[r]; anc[r] = k; r = nx; }
      if (anc[r] == -1) { anc[r] = k; par[r] = k; }
    }
  }
  std::vector<int> head(nb, -1), nxt(nb, -1), post;
  for (int k = nb - 1; k >= 0; --k) if (par[k] >= 0) { nxt[k] = head[par[k]]; head[par[k]] = k; }
  post.reserve(nb);
  std::vector<int> stack;
  for (int r = 0; r < nb; ++r) {
    if (par[r] >= 0) continue;
    stack.push_back(r);
    while (!stack.empty()) {
      const int k = stack.back();
      if (head[k] >= 0) { const int c = head[k]; head[k] = nxt[c]; stack.push_back(c); }   // next unvisited child
      else { post.push_back(k); stack.pop_back(); }
    }
  }
  std::vector<int> ipost(nb);
  pm.assign(nb, 0);
  par2.assign(nb, -1);
  for (int k = 0; k < nb; ++k) { pm[k] = perm[post[k]]; ipost[post[k]] = k; }
  for (int k = 0; k < nb; ++k) if (par[k] >= 0) par2[ipost[k]] = ipost[par[k]];      // the same tree under the post-order
}

// ---- column patterns: pattern(k) = A(k+1:, k)  U  union over children c of pattern(c) \ {k}
// `par` = the elimination tree of the order `pm` when the caller knows it (Liu's algorithm above) and the order is a
// post-order: disjoint sub-trees are then contiguous column ranges whose patterns depend on nothing outside, so they are
// computed concurrently (one mark array per worker), the columns above them serially afterwards.
void pattern_pass(const BlockGraph &g, const std::vector<int> &pm, const std::vector<int> *par, std::vector<std::vector<int>> &pat, Symbolic &S, bool prof) {
  const int nb = g.n;
  S.perm = pm;
  S.iperm.assign(nb, -1);
  for (int k = 0; k < nb; ++k) S.iperm[pm[k]] = k;
  S.parent.assign(nb, -1);
  S.colptr.assign(nb + 1, 0);
  S.max_col_blocks = 0;
  std::vector<int> first_child(nb, -1), next_sib(nb, -1);
  std::vector<char> done(nb, 0);
  auto column = [&](int k, std::vector<int> &mark, std::vector<int> &tmp) {
    tmp.clear();
    mark[k] = k;
    const int v = pm[k];
    for (int p = g.xadj[v]; p < g.xadj[v + 1]; ++p) {
      const int i = S.iperm[g.adj[p]];
      if (i > k && mark[i] != k) { mark[i] = k; tmp.push_back(i); }
    }
    for (int c = first_child[k]; c >= 0; c = next_sib[c])
      for (int i : pat[c])
        if (i > k && mark[i] != k) { mark[i] = k; tmp.push_back(i); }
    std::sort(tmp.begin(), tmp.end());
    pat[k] = tmp;
    S.parent[k] = tmp.empty() ? -1 : tmp[0];
  };
  if (par && host_threads() > 1) {
    // children lists from the known tree (ascending), sub-tree sizes, and the maximal sub-trees below a size bound
    for (int k = nb - 1; k >= 0; --k) if ((*par)[k] >= 0) { next_sib[k] = first_child[(*par)[k]]; first_child[(*par)[k]] = k; }
    std::vector<int> size(nb, 1);
    for (int k = 0; k < nb; ++k) if ((*par)[k] >= 0) size[(*par)[k]] += size[k];
    const int bound = std::max(256, nb / (8 * host_threads()));
    std::vector<int> roots;
    for (int k = 0; k < nb; ++k) if (size[k] <= bound && ((*par)[k] < 0 || size[(*par)[k]] > bound)) roots.push_back(k);
    static std::atomic<uint64_t> calls{0};
    const uint64_t token = ++calls;                                  // (a pool thread's mark array is re-initialised once per call)
    parallel_ranges((int)roots.size(), 1, [&](int r0, int r1) {
      static thread_local std::vector<int> mark;
      static thread_local uint64_t mark_token = 0;
      std::vector<int> tmp;
      if (mark_token != token || (int)mark.size() != nb) { mark.assign(nb, -1); mark_token = token; }
      for (int r = r0; r < r1; ++r) {
        const int top = roots[r];
        for (int k = top - size[top] + 1; k <= top; ++k) { column(k, mark, tmp); done[k] = 1; }
        // (marks left on ancestors are column ids of THIS sub-tree: never equal to a later k of this call)
      }
    });
    std::vector<int> mark(nb, -1), tmp;
    int64_t nser = 0, wser = 0;
    for (int k = 0; k < nb; ++k) if (!done[k]) { column(k, mark, tmp); ++nser; wser += (int64_t)tmp.size(); }
    if (prof) std::fprintf(stderr, "[fgo symbolic]   pattern pass: %zu sub-trees in parallel (<= %d columns), %lld columns / %lld pattern entries serially\n", roots.size(), bound, (long long)nser, (long long)wser);
  } else {
    std::vector<int> mark(nb, -1), tmp;
    for (int k = 0; k < nb; ++k) {
      column(k, mark, tmp);
      if (!tmp.empty()) { const int p = tmp[0]; next_sib[k] = first_child[p]; first_child[p] = k; }
    }
  }
  for (int k = 0; k < nb; ++k) {
    S.colptr[k + 1] = S.colptr[k] + 1 + (int64_t)pat[k].size();
    S.max_col_blocks = std::max(S.max_col_blocks, 1 + (int)pat[k].size());
  }
}

// ---- multi-GPU: domain decomposition of the (post-ordered) elimination tree.  The tree is cut into disjoint
// sub-trees ("domains", dealt to the ranks by weight) and the set of their common ancestors (the "top": the upper
// nested-dissection separators).  Columns are re-ordered [domain of rank 0 | rank 1 | ... | top] -- still a
// topological order of the same tree, so the fill is unchanged; inside a group the post-order is kept, so a sub-tree
// stays a contiguous column range.  A rank factors only its own columns; every update that crosses from a domain into
// the top is summed over the ranks by one collective on the (contiguous) tail of L (fgo_api.cpp).
void decompose_domains(const BlockGraph &g, std::vector<std::vector<int>> &pat, Symbolic &S, bool prof) {
  const int nb = g.n, world = S.world;
  S.dom_col0.assign((size_t)world + 2, nb);
  S.dom_col0[0] = 0;
  if (world == 1) return;
  std::vector<double> subw(nb);
  for (int k = 0; k < nb; ++k) { const double c = (double)(S.colptr[k + 1] - S.colptr[k]); subw[k] = 0.5 * c * (c + 1); }   // updates generated by column k
  std::vector<int> head(nb, -1), nxt(nb, -1);
  double total = 0;
  for (int k = 0; k < nb; ++k) { const int p = S.parent[k]; if (p >= 0) subw[p] += subw[k]; }
  for (int k = nb - 1; k >= 0; --k) { const int p = S.parent[k]; if (p >= 0) { nxt[k] = head[p]; head[p] = k; } else total += subw[k]; }
  // open the heaviest sub-tree until there are enough of them to balance and none is too heavy.  Round 3 (tools/dist_sweep.sh,
  // profiles/r03_e_dist_decomposition.txt): a SMALLER top wins -- every column moved from the replicated, latency-bound top into
  // a domain is work divided by the ranks and bytes taken out of the collective: 2 sub-trees per rank and a cap of one fair
  // share (was 4 and a quarter) give 2.33 instead of 2.85 ms per trial at 8 ranks on cfg 2 with 4.2 instead of 20.2 MB in the
  // all-reduce, 6.9 instead of 8.3 ms on cfg 5 (8.4-23 instead of 20-35 MB)
  std::vector<std::pair<double, int>> heap;                           // (weight, root)
  for (int k = 0; k < nb; ++k) if (S.parent[k] < 0) heap.push_back({subw[k], k});
  std::make_heap(heap.begin(), heap.end());
  std::vector<char> is_top(nb, 0);
  static const double max_share = tune("dist_max_share", 1.0);   // of one rank's fair share
  while (!heap.empty()) {
    const std::pair<double, int> h = heap.front();
    static const int min_trees = (int)tune("dist_min_trees", 2);   // sub-trees per rank at least
    const bool enough = (int)heap.size() >= min_trees * world && h.first <= max_share * total / world;
    if (enough || head[h.second] < 0) break;                          // (a childless column cannot be opened)
    std::pop_heap(heap.begin(), heap.end()); heap.pop_back();
    is_top[h.second] = 1;
    for (int c = head[h.second]; c >= 0; c = nxt[c]) { heap.push_back({subw[c], c}); std::push_heap(heap.begin(), heap.end()); }
  }
  // largest first onto the least loaded rank (ties: lowest rank) -- deterministic, identical on every rank
  std::sort(heap.begin(), heap.end(), [](const std::pair<double, int> &a, const std::pair<double, int> &b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
  std::vector<double> load(world, 0.0);
  std::vector<int> group(nb, -1);
  for (const auto &h : heap) {
    int r = 0;
    for (int q = 1; q < world; ++q) if (load[q] < load[r]) r = q;
    load[r] += h.first;
    group[h.second] = r;
  }
  for (int k = nb - 1; k >= 0; --k) {                                 // parents before children: push the group down
    if (is_top[k]) { group[k] = world; continue; }
    if (group[k] < 0) group[k] = group[S.parent[k]];
  }
  std::vector<int> cnt((size_t)world + 2, 0);
  for (int k = 0; k < nb; ++k) cnt[group[k] + 1]++;
  for (int q = 0; q <= world; ++q) cnt[q + 1] += cnt[q];
  for (int q = 0; q <= world + 1; ++q) S.dom_col0[q] = cnt[q];
  std::vector<int> pm(nb);
  {
    std::vector<int> fill(cnt.begin(), cnt.end() - 1);
    for (int k = 0; k < nb; ++k) pm[fill[group[k]]++] = S.perm[k];
  }
  for (auto &v : pat) v.clear();
  pattern_pass(g, pm, nullptr, pat, S, prof);
  if (prof) {
    std::fprintf(stderr, "[fgo symbolic] domains: %zu sub-trees, top %d columns;", heap.size(), nb - S.dom_col0[world]);
    for (int q = 0; q < world; ++q) std::fprintf(stderr, " %.1f%%", 100.0 * load[q] / total);
    std::fprintf(stderr, " of the update work per rank\n");
  }
}

void fill_columns(std::vector<std::vector<int>> &pat, Symbolic &S) {
  parallel_ranges(S.nb, 2048, [&](int kb, int ke) {
    for (int k = kb; k < ke; ++k) {
      int64_t p = S.colptr[k];
      S.rowidx[p] = k; S.blkcol[p] = k; ++p;
      for (int i : pat[k]) { S.rowidx[p] = i; S.blkcol[p] = k; ++p; }
      std::vector<int>().swap(pat[k]);
    }
  });
}

// ---- row lists: row k = { L_kj : j < k }, ascending j
void build_row_lists(Symbolic &S) {
  const int nb = S.nb;
  S.rowptr.assign(nb + 1, 0);
  for (int j = 0; j < nb; ++j)
    for (int64_t p = S.colptr[j] + 1; p < S.colptr[j + 1]; ++p) S.rowptr[S.rowidx[p] + 1]++;
  for (int k = 0; k < nb; ++k) S.rowptr[k + 1] += S.rowptr[k];
  S.row_blk.resize(S.rowptr[nb]);
  S.row_col.resize(S.rowptr[nb]);
  std::vector<int64_t> fill(S.rowptr.begin(), S.rowptr.end() - 1);
  for (int j = 0; j < nb; ++j)
    for (int64_t p = S.colptr[j] + 1; p < S.colptr[j + 1]; ++p) {
      const int64_t o = fill[S.rowidx[p]]++;
      S.row_blk[o] = (int)p; S.row_col[o] = j;
    }
}

// ---- update lists, first pass: the number of updates per target block (for_each_op_of_column, symbolic_build.hpp)
void count_update_ops(Symbolic &S) {
  S.op_ptr.assign(S.nnzL + 1, 0);
  parallel_ranges(S.nb, 512, [&](int kb, int ke) {
    for (int k = kb; k < ke; ++k) for_each_op_of_column(S, k, [&](int64_t u, int64_t, int64_t) { S.op_ptr[u + 1]++; });
  });
  for (int64_t t = 0; t < S.nnzL; ++t) S.op_ptr[t + 1] += S.op_ptr[t];
  S.nops = S.op_ptr[S.nnzL];
}

}  // namespace symbolic
}  // namespace fgo
