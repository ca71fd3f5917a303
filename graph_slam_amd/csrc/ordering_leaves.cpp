// Nested dissection, the leaves (ordering_build.hpp).
#include "ordering_build.hpp"

namespace fgo::ordering {

// exact minimum degree on a small vertex set with halo (neighbours outside the set count towards
// the degree and receive fill, but are never eliminated here)
void Dissection::leaf_md(const std::vector<int> &vs, Scratch &sc) const {
  prepare(sc);
  std::vector<int> &out = sc.out, &local = sc.local, &region = sc.region;
  const int m = (int)vs.size();
  // tiny sets need no search; very large separators end up (nearly) dense whatever the order
  sc.stats.n[m <= 2 ? ND_LEAF_SMALL : m > 384 ? ND_LEAF_LARGE : ND_LEAF_SEARCHED]++;
  if (m <= 2 || m > 384) { for (int v : vs) { out.push_back(v); region[v] = -1; } return; }
  if (local.empty()) local.assign(g.n, -1);
  std::vector<int> &ext = sc.ext;   // halo vertices: not yet ordered, outside the set
  ext.clear();
  for (int i = 0; i < m; ++i) local[vs[i]] = i;
  for (int i = 0; i < m; ++i)
    for (int p = g.xadj[vs[i]]; p < g.xadj[vs[i] + 1]; ++p) {
      int u = g.adj[p];
      if (region[u] == -1) continue;            // eliminated earlier: cannot receive fill
      if (local[u] < 0) { local[u] = m + (int)ext.size(); ext.push_back(u); }
    }
  const int tot = m + (int)ext.size(), W = (tot + 63) / 64;
  std::vector<uint64_t> &rows = sc.rows;
  rows.assign((size_t)tot * W, 0);
  auto setb = [&](int a, int b) { rows[(size_t)a * W + (b >> 6)] |= 1ull << (b & 63); };
  for (int i = 0; i < m; ++i)
    for (int p = g.xadj[vs[i]]; p < g.xadj[vs[i] + 1]; ++p) {
      int u = g.adj[p];
      if (region[u] == -1) continue;
      int lu = local[u];
      setb(i, lu); setb(lu, i);
    }
  std::vector<char> &done = sc.done;
  done.assign(m, 0);
  for (int step = 0; step < m; ++step) {
    int best = -1, bestd = 1 << 30;
    for (int i = 0; i < m; ++i) {
      if (done[i]) continue;
      int d = 0;
      for (int w = 0; w < W; ++w) d += __builtin_popcountll(rows[(size_t)i * W + w]);
      if (d < bestd) { bestd = d; best = i; }
    }
    const uint64_t *rb = &rows[(size_t)best * W];
    // neighbours of best become a clique
    for (int w = 0; w < W; ++w) {
      uint64_t bits = rb[w];
      while (bits) {
        int u = (w << 6) + __builtin_ctzll(bits);
        bits &= bits - 1;
        uint64_t *ru = &rows[(size_t)u * W];
        for (int x = 0; x < W; ++x) ru[x] |= rb[x];
        ru[u >> 6] &= ~(1ull << (u & 63));
        ru[best >> 6] &= ~(1ull << (best & 63));
      }
    }
    for (int w = 0; w < W; ++w) rows[(size_t)best * W + w] = 0;
    done[best] = 1;
    out.push_back(vs[best]);
  }
  // (marked eliminated only now: a vertex of this set is a fill-receiving neighbour of the others until its turn,
  //  and nobody else looks at these labels meanwhile)
  for (int i = 0; i < m; ++i) { region[vs[i]] = -1; local[vs[i]] = -1; }
  for (int u : ext) local[u] = -1;
}

}  // namespace fgo::ordering
