// Phases of the nested dissection (ordering.cpp is the driver): the state they share, the settings read from tune(), and what each phase
// file offers the others.  Host only; also built without the HIP headers (tools/symstats.cpp).
#pragma once
#include <atomic>
#include <vector>
#include "fgo_internal.hpp"

namespace fgo::ordering {

// FGO_TUNE settings of the ordering (nd_<member>), read once per process; the measurement behind a default stands where it is used
struct Settings {
  int time = (int)tune("nd_time", 1), time_band = (int)tune("nd_time_band", 32), time_recover = (int)tune("nd_time_recover", 1), time_keep = (int)tune("nd_time_keep", 8);
  double time_frac = tune("nd_time_frac", 0.9), time_frac2 = tune("nd_time_frac2", time_frac);
  int starts = (int)tune("nd_starts", 2), cover = (int)tune("nd_cover", 1);
  double min_side = tune("nd_min_side", 0.03);   // (0.03 leaves the cuts of the Manhattan benchmark graphs alone: cfg 2 keeps 30 levels)
  static const Settings &get() { static const Settings s{}; return s; }
};

// per-worker state.  Regions handled by different workers are never adjacent (a separator lies between them) and a
// worker only needs to know of an outside vertex that it is not eliminated yet (ancestors' separators, hubs), so
// every worker labels its own copy of the per-vertex arrays: shared arrays would be race-free too, but regions
// interleave in index space and the cache lines ping-pong (measured: no speed-up at all from 8 threads).
struct Scratch {
  std::vector<int> region;   // current region label of each vertex (-1 = already ordered)
  std::vector<int> lvl;      // BFS level
  std::vector<int> local;    // global -> local index for the leaf ordering (covers halo vertices, which ARE shared)
  std::vector<int> out;      // elimination order produced by this worker
  std::vector<int> bfs_order, comp, ext, order1, lvl1, cnt, tf, tb;
  std::vector<uint64_t> rows;  // adjacency bit rows of the leaf ordering (kept: big ones would be mmap'ed / unmapped per call)
  std::vector<char> done;
  OrderingStats stats;       // the paths this worker took: plain counts, summed by order_all
};

enum SplitResult { SPLIT, DISCONNECTED, NO_CUT };
struct Item { std::vector<int> vs; bool is_sep; };

// One dissection: the graph, the options and the labels every worker starts from.
struct Dissection {
  const BlockGraph &g;
  const OrderingOptions &opt;     // bal_w, bal_t, time_side, time_weight
  int leaf;
  bool time_mode = false;         // vertex index = time (a pose graph handed over in creation order): dissect by index cuts only
  std::vector<int> tlabel;        // time mode with RECOVERED labels (round 6: a graph whose ids are not creation order): rank of a vertex; empty = its index
  std::vector<int> base_region;   // template of the per-worker label arrays: 0, or -3 for a hub (invisible to the BFS,
                                  // still a fill-receiving neighbour in the leaf ordering)
  std::atomic<int> next_region{1};

  Dissection(const BlockGraph &gg, const OrderingOptions &o) : g(gg), opt(o), leaf(std::max(4, o.leaf)), base_region(gg.n, 0) {}
  void prepare(Scratch &sc) const { if (sc.region.empty()) { sc.region = base_region; sc.lvl.assign(g.n, -1); } }
  // BFS inside region r from s; fills lvl for reached vertices, returns them in `queue` order.
  void bfs(int s, int r, std::vector<int> &order, Scratch &sc) const {
    order.assign(1, s); sc.lvl[s] = 0;
    for (size_t head = 0; head < order.size(); ++head) {
      const int v = order[head];
      for (int p = g.xadj[v]; p < g.xadj[v + 1]; ++p) {
        const int u = g.adj[p];
        if (sc.region[u] == r && sc.lvl[u] < 0) { sc.lvl[u] = sc.lvl[v] + 1; order.push_back(u); }
      }
    }
  }
  void clear_lvl(const std::vector<int> &vs, Scratch &sc) const { for (int v : vs) sc.lvl[v] = -1; }
  // ordering_cuts.cpp.  in: region S.  out: its fresh label r; SPLIT -- A, B, sep (their element order is part of the result); DISCONNECTED --
  // the component of S[0] in sc.bfs_order, levels set
  SplitResult split(const std::vector<int> &S, Scratch &sc, int &r, std::vector<int> &A, std::vector<int> &B, std::vector<int> &sep);
  // ordering_leaves.cpp.  in: a vertex set.  out: appended to sc.out in elimination order, labelled -1 (eliminated)
  void leaf_md(const std::vector<int> &vs, Scratch &sc) const;
  // ordering_tree.cpp.  components: in: a region split() found DISCONNECTED.  out: its components appended to `items`.  order_region: the
  // order of one region appended to sc.out.  order_all: the order of all of vs APPENDED to `out`, the workers' path counts added to *stats
  void components(const std::vector<int> &S, Scratch &sc, int r, std::vector<Item> &items);
  void order_region(std::vector<int> vs, Scratch &sc);
  void order_all(std::vector<int> vs, std::vector<int> &out, OrderingStats *stats);
};

}  // namespace fgo::ordering
