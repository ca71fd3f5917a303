// Structure phase, pairs: the unique variable pairs of all factors (+ co-visibility pairs of eliminated landmarks, + the phantom
// band of the growth reserve) and the block graph the ordering works on.
#include "structure_build.hpp"

namespace fgo {

// The items of [0, n) that `keep` accepts, compacted in order on all host threads: count per chunk, prefix sums, fill.
// sized(total) makes room once the total is known; emit(i, w) places kept item i at position w.
template <class Keep, class Sized, class Emit>
static void parallel_compact(int64_t n, Keep keep, Sized sized, Emit emit) {
  constexpr int64_t CH = 1 << 16;
  const int nch = (int)((n + CH - 1) / CH);
  std::vector<int64_t> at((size_t)nch + 1, 0);
  parallel_ranges(nch, 1, [&](int c0, int c1) {
    for (int ch = c0; ch < c1; ++ch) {
      int64_t cnt = 0;
      for (int64_t i = ch * CH, i1 = std::min(n, i + CH); i < i1; ++i) cnt += keep(i);
      at[(size_t)ch + 1] = cnt;
    }
  });
  for (int ch = 0; ch < nch; ++ch) at[(size_t)ch + 1] += at[(size_t)ch];
  sized(at[(size_t)nch]);
  parallel_ranges(nch, 1, [&](int c0, int c1) {
    for (int ch = c0; ch < c1; ++ch) {
      int64_t w = at[(size_t)ch];
      for (int64_t i = ch * CH, i1 = std::min(n, i + CH); i < i1; ++i) if (keep(i)) emit(i, w++);
    }
  });
}

int pairs_and_graph(fgo_ctx *c, const VarIndex &V, PairGraph &G, BuildTimer &tm) {
  // binary factors that couple two free variables, in edge order
  parallel_compact(V.E, [&](int64_t e) { return needs_pair(V.hidx[c->ei[e]], V.hidx[c->ej[e]]); },
                   [&](int64_t n) { G.pr.resize((size_t)n); },
                   [&](int64_t e, int64_t w) { const int a = V.hidx[c->ei[e]], b = V.hidx[c->ej[e]]; G.pr[(size_t)w] = {std::min(a, b), std::max(a, b), e}; });
  // the 6-variable IMU factors contribute all 15 variable pairs; encoded as e = -1 - (15 f + pair)
  for (int64_t f = 0; f < V.NI; ++f)
    for (int q = 0; q < 15; ++q) {
      const int a = V.hidx[c->imu_ids[6 * f + IMU_PAIR[q][0]]], b = V.hidx[c->imu_ids[6 * f + IMU_PAIR[q][1]]];
      if (needs_pair(a, b)) G.pr.push_back({std::min(a, b), std::max(a, b), -1 - (15 * f + q)});
    }
  // eliminating a landmark couples all the cameras that see it
  if (V.n_lm > 0) ba_covisibility_pairs(c, V, G.pr);
  for (int64_t k = 0; k < V.R; ++k)                                            // phantom k couples to the `window` variables before it
    for (int64_t u = std::max<int64_t>(0, V.N + k - V.isam_window); u < V.N + k; ++u)
      if (V.hidx[u] >= 0) G.pr.push_back({std::min(V.hidx[u], V.hidx[V.N + k]), std::max(V.hidx[u], V.hidx[V.N + k]), STRUCT_ONLY});
  {   // sort by (a, b, e): counting sort on a (counts and places claimed with atomic increments: the order inside a run does
      // not matter), then the (short) runs of equal a are sorted in parallel
    std::vector<int64_t> start((size_t)V.nfree + 1, 0);
    const int npr = (int)std::min<size_t>(G.pr.size(), (size_t)INT32_MAX);
    parallel_ranges(npr, 1 << 16, [&](int i0, int i1) { for (int i = i0; i < i1; ++i) __atomic_fetch_add(&start[(size_t)G.pr[(size_t)i].a + 1], (int64_t)1, __ATOMIC_RELAXED); });
    for (size_t i = (size_t)npr; i < G.pr.size(); ++i) start[(size_t)G.pr[i].a + 1]++;
    for (int i = 0; i < V.nfree; ++i) start[i + 1] += start[i];
    std::vector<PairRec> sorted(G.pr.size());
    {
      std::vector<int64_t> fill(start.begin(), start.end() - 1);
      parallel_ranges(npr, 1 << 16, [&](int i0, int i1) {
        for (int i = i0; i < i1; ++i) sorted[(size_t)__atomic_fetch_add(&fill[(size_t)G.pr[(size_t)i].a], (int64_t)1, __ATOMIC_RELAXED)] = G.pr[(size_t)i];
      });
      for (size_t i = (size_t)npr; i < G.pr.size(); ++i) sorted[(size_t)fill[(size_t)G.pr[i].a]++] = G.pr[i];
    }
    parallel_ranges(V.nfree, 4096, [&](int ab, int ae) {
      for (int a = ab; a < ae; ++a)
        std::sort(sorted.begin() + start[a], sorted.begin() + start[a + 1],
                  [](const PairRec &x, const PairRec &y) { return x.b != y.b ? x.b < y.b : x.e < y.e; });
    });
    G.pr.swap(sorted);
  }
  // unique pairs: the heads of the runs of equal (a, b), with the index in pr of the first member
  const int64_t np = (int64_t)G.pr.size();
  parallel_compact(np, [&](int64_t i) { return i == 0 || G.pr[(size_t)i].a != G.pr[(size_t)i - 1].a || G.pr[(size_t)i].b != G.pr[(size_t)i - 1].b; },
                   [&](int64_t nu) { G.ua.resize((size_t)nu); G.ub.resize((size_t)nu); G.ufirst.resize((size_t)nu + 1); G.ufirst[(size_t)nu] = np; },
                   [&](int64_t i, int64_t w) { G.ua[(size_t)w] = G.pr[(size_t)i].a; G.ub[(size_t)w] = G.pr[(size_t)i].b; G.ufirst[(size_t)w] = i; });
  G.noff = (int64_t)G.ua.size();
  c->n_offdiag = G.noff;
  G.g.n = V.nfree;
  G.g.xadj.assign((size_t)V.nfree + 1, 0);
  // pair index of every adjacency entry, in the order the block graph lists them
  {   // adjacency lists: a vertex's neighbours ascending (what the serial fill over the sorted pairs produced), places claimed
      // with atomic increments and every list sorted afterwards -- as (neighbour, pair) keys, so that adj_pair comes with it
    const int nh = (int)std::min<int64_t>(G.noff, INT32_MAX);
    parallel_ranges(nh, 1 << 16, [&](int h0, int h1) {
      for (int h = h0; h < h1; ++h) { __atomic_fetch_add(&G.g.xadj[(size_t)G.ua[(size_t)h] + 1], 1, __ATOMIC_RELAXED); __atomic_fetch_add(&G.g.xadj[(size_t)G.ub[(size_t)h] + 1], 1, __ATOMIC_RELAXED); }
    });
    if (G.noff > nh) return fail(c, FGO_EINVAL, "more than 2^31 block pairs");
    for (int i = 0; i < V.nfree; ++i) G.g.xadj[i + 1] += G.g.xadj[i];
    std::vector<uint64_t> key((size_t)G.g.xadj[V.nfree]);
    std::vector<int> fill(G.g.xadj.begin(), G.g.xadj.end() - 1);
    parallel_ranges(nh, 1 << 16, [&](int h0, int h1) {
      for (int h = h0; h < h1; ++h) {
        key[(size_t)__atomic_fetch_add(&fill[(size_t)G.ua[(size_t)h]], 1, __ATOMIC_RELAXED)] = ((uint64_t)(uint32_t)G.ub[(size_t)h] << 32) | (uint32_t)h;
        key[(size_t)__atomic_fetch_add(&fill[(size_t)G.ub[(size_t)h]], 1, __ATOMIC_RELAXED)] = ((uint64_t)(uint32_t)G.ua[(size_t)h] << 32) | (uint32_t)h;
      }
    });
    G.g.adj.resize(key.size()); G.adj_pair.resize(key.size());
    parallel_ranges(V.nfree, 4096, [&](int v0, int v1) {
      for (int v = v0; v < v1; ++v) {
        std::sort(key.begin() + G.g.xadj[v], key.begin() + G.g.xadj[v + 1]);
        for (int p = G.g.xadj[v]; p < G.g.xadj[v + 1]; ++p) { G.g.adj[(size_t)p] = (int)(key[(size_t)p] >> 32); G.adj_pair[(size_t)p] = (int)(uint32_t)key[(size_t)p]; }
      }
    });
  }
  tm.lap("pairs + block graph");
  return FGO_OK;
}

}  // namespace fgo
