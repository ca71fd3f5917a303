// Nested dissection, the tree: a region is bisected until its parts are leaves; the top of the tree is expanded breadth-first so that
// the regions below it can be ordered concurrently (ordering_build.hpp).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "ordering_build.hpp"

namespace fgo::ordering {

// A region that split() found DISCONNECTED (the component of S[0] in sc.bfs_order, levels set, label r on all of S): label
// ALL components in one linear pass (bundle adjustment leaves hundreds of thousands of isolated points once the cameras
// are taken out).  Small components are binned into leaf-sized groups (is_sep: ordered as they are); appended to `items` in
// the order the serial dissection pushes them on its stack -- they are processed in the REVERSE order.
void Dissection::components(const std::vector<int> &S, Scratch &sc, int r, std::vector<Item> &items) {
  std::vector<int> &region = sc.region;
  std::vector<std::vector<int>> big;
  std::vector<int> bin;
  auto flush = [&]() { if (!bin.empty()) { items.push_back({std::move(bin), true}); bin.clear(); } };
  std::vector<int> &comp = sc.comp;
  comp = sc.bfs_order;
  size_t next_seed = 0;
  while (true) {
    clear_lvl(comp, sc);
    const int rc = next_region++;
    for (int v : comp) region[v] = rc;
    if ((int)comp.size() > leaf) big.push_back(comp);
    else {
      if ((int)(bin.size() + comp.size()) > leaf) flush();
      bin.insert(bin.end(), comp.begin(), comp.end());
    }
    while (next_seed < S.size() && region[S[next_seed]] != r) ++next_seed;
    if (next_seed >= S.size()) break;
    bfs(S[next_seed], r, comp, sc);
  }
  flush();
  for (auto &b : big) items.push_back({std::move(b), false});
}

// serial dissection of one region (explicit stack); appends to sc.out
void Dissection::order_region(std::vector<int> vs, Scratch &sc) {
  std::vector<Item> stack;
  stack.push_back({std::move(vs), false});
  // Separators must be ordered AFTER both halves: emulate post-order with a second marker.
  // We push [sep(is_sep=true), B, A] so that A is popped first, then B, then the separator.
  prepare(sc);
  std::vector<int> A, B, sep;
  while (!stack.empty()) {
    Item it = std::move(stack.back());
    stack.pop_back();
    std::vector<int> &S = it.vs;
    if (S.empty()) continue;
    if (it.is_sep || (int)S.size() <= leaf) { leaf_md(S, sc); continue; }
    int r = 0;
    const SplitResult res = split(S, sc, r, A, B, sep);
    // (counted here and not in split(): the top tree tries such a region once more before it hands it over)
    if (res == NO_CUT) { sc.stats.n[ND_NO_CUT]++; leaf_md(S, sc); continue; }
    if (res == DISCONNECTED) { components(S, sc, r, stack); continue; }
    stack.push_back({std::move(sep), true});
    stack.push_back({std::move(B), false});
    stack.push_back({std::move(A), false});
    A = std::vector<int>(); B = std::vector<int>(); sep = std::vector<int>();
  }
}

// an expanded node of the top tree: its children in the order they are eliminated (two for a bisection, the components for a disconnected
// region -- the small ones together in ONE child that orders its sets as they are), then its separator
struct Node { std::vector<int> vs, sep, kids; std::vector<std::vector<int>> sets; bool expanded = false, leaf_only = false; Scratch sc; };
static double tnow() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void add_stats(OrderingStats &to, const OrderingStats &from) { for (int i = 0; i < ND_PATHS; ++i) to.n[i] += from.n[i]; }
static int add_node(std::vector<Node> &nodes, int parent, std::vector<int> &&vs) {       // (invalidates references, not indices)
  nodes.emplace_back(); nodes.back().vs = std::move(vs);
  nodes[(size_t)parent].kids.push_back((int)nodes.size() - 1);
  return (int)nodes.size() - 1;
}

// The regions of one depth are bisected concurrently until there are `want` regions AND none of them is much larger than its share:
// bisections are not balanced, and a region that stays big is ordered by ONE worker (cfg 5: a region of 274 k of the 1 M poses, 0.40 s of
// the 0.78 s).  in: nodes = the root.  out: the top tree
static void expand_top(Dissection &d, std::vector<Node> &nodes) {
  const int want = 2 * host_threads(), leaf = d.leaf;
  std::vector<int> frontier{0};                      // unexpanded regions that may still be bisected
  int settled = 0;                                   // unexpanded regions that will not be (small, or no cut found)
  const size_t big = std::max<size_t>((size_t)8 * leaf, nodes[0].vs.size() / (size_t)want);
  while (!frontier.empty()) {
    const bool more = (int)frontier.size() + settled < want;
    std::vector<int> cand;
    for (int id : frontier) {
      const size_t sz = nodes[id].vs.size();
      if ((int)sz > 8 * leaf && (more || sz > big)) cand.push_back(id); else ++settled;
    }
    if (cand.empty()) break;
    std::vector<std::vector<int>> A(cand.size()), B(cand.size());
    std::vector<std::vector<Item>> comps(cand.size());
    std::vector<char> ok(cand.size(), 0);                // 1: bisected, 2: disconnected (components)
    parallel_ranges((int)cand.size(), 1, [&](int q0, int q1) {
      for (int q = q0; q < q1; ++q) {
        Node &nd = nodes[cand[q]];
        int r = 0;
        const SplitResult res = d.split(nd.vs, nd.sc, r, A[q], B[q], nd.sep);
        if (res == DISCONNECTED) { d.components(nd.vs, nd.sc, r, comps[q]); ok[q] = 2; }
        else ok[q] = res == SPLIT;
      }
    });
    frontier.clear();
    for (size_t q = 0; q < cand.size(); ++q) {
      const int id = cand[q];
      if (!ok[q]) { ++settled; nodes[id].sep.clear(); continue; }
      nodes[id].expanded = true;
      std::vector<int>().swap(nodes[id].vs);
      { const OrderingStats keep = nodes[id].sc.stats; nodes[id].sc = Scratch(); nodes[id].sc.stats = keep; }   // its label arrays are no longer needed
      if (ok[q] == 1) {
        frontier.push_back(add_node(nodes, id, std::move(A[q])));
        frontier.push_back(add_node(nodes, id, std::move(B[q])));
        continue;
      }
      nodes[id].sep.clear();
      std::vector<std::vector<int>> sets;
      for (size_t x = comps[q].size(); x-- > 0;) {      // the order in which the serial dissection pops them
        Item &it = comps[q][x];
        if (it.is_sep) sets.push_back(std::move(it.vs)); else frontier.push_back(add_node(nodes, id, std::move(it.vs)));
      }
      if (!sets.empty()) {                               // (pushed first, hence popped last: behind the large components)
        Node &kid = nodes[(size_t)add_node(nodes, id, std::vector<int>())];
        kid.leaf_only = true; kid.sets = std::move(sets);
        ++settled;
      }
    }
  }
}
// the unexpanded regions, concurrently, one worker each; their orders are left in their own sc.out
static void order_regions(Dissection &d, std::vector<Node> &nodes, bool prof, double t1) {
  std::vector<int> work;
  for (size_t id = 0; id < nodes.size(); ++id) if (!nodes[id].expanded) work.push_back((int)id);
  parallel_ranges((int)work.size(), 1, [&](int w0, int w1) {
    for (int w = w0; w < w1; ++w) {
      Node &nd = nodes[work[w]];
      const double ta = tnow(); const size_t sz = nd.vs.size();
      if (nd.leaf_only) { for (const std::vector<int> &set : nd.sets) d.leaf_md(set, nd.sc); std::vector<std::vector<int>>().swap(nd.sets); }
      else d.order_region(std::move(nd.vs), nd.sc);
      if (prof) std::fprintf(stderr, "[fgo ordering]   region of %zu: %.1f ms (start %.1f)\n", sz, 1e3 * (tnow() - ta), 1e3 * (ta - t1));
      std::vector<int>().swap(nd.sc.local); std::vector<int>().swap(nd.sc.region); std::vector<int>().swap(nd.sc.lvl);
    }
  });
}
// emit in post-order: A, B, separator (the separators of the top tree are ordered here, in `top`: everything emitted so far is eliminated)
static void emit_postorder(const Dissection &d, std::vector<Node> &nodes, int id, Scratch &top, std::vector<int> &out) {
  Node &nd = nodes[(size_t)id];
  if (!nd.expanded) {
    out.insert(out.end(), nd.sc.out.begin(), nd.sc.out.end());
    if (nodes[0].expanded) for (int v : nd.sc.out) top.region[v] = -1;
    return;
  }
  for (int kid : nd.kids) emit_postorder(d, nodes, kid, top, out);      // (as deep as the top tree: a few dozen frames)
  top.out.clear();
  if (!nd.sep.empty()) d.leaf_md(nd.sep, top);
  out.insert(out.end(), top.out.begin(), top.out.end());
}

// The top of the dissection tree is expanded breadth-first, the regions of one depth being bisected concurrently;
// the subregions below are ordered concurrently, one worker each; the separators of the top tree follow in
// post-order.  Same order as the serial algorithm: what happens inside a region never depends on the other side
// of a separator.
void Dissection::order_all(std::vector<int> vs, std::vector<int> &out, OrderingStats *stats) {
  std::vector<Node> nodes(1); nodes[0].vs = std::move(vs);
  const bool prof = std::getenv("FGO_SYM_PROFILE") != nullptr;
  const double t0 = tnow();
  if (host_threads() > 1) expand_top(*this, nodes);
  const double t1 = tnow();
  if (prof) { std::fprintf(stderr, "[fgo ordering] region sizes:"); for (auto &nd : nodes) if (!nd.expanded) std::fprintf(stderr, " %zu", nd.vs.size()); std::fprintf(stderr, "\n"); }
  order_regions(*this, nodes, prof, t1);
  const double t2 = tnow();
  Scratch top; if (nodes[0].expanded) prepare(top);
  emit_postorder(*this, nodes, 0, top, out);
  for (const Node &nd : nodes) if (stats) add_stats(*stats, nd.sc.stats);      // every worker's counts, and those of the top separators
  if (stats) add_stats(*stats, top.stats);
  if (prof) std::fprintf(stderr, "[fgo ordering] top tree (%zu nodes) %.1f ms, regions %.1f ms, top separators %.1f ms\n", nodes.size(), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (tnow() - t2));
}

}  // namespace fgo::ordering
