// Nested dissection, the cuts: one bisection of a region, by index (vertex index or recovered label = time) or by a BFS level structure;
// both end in a minimum vertex cover of the edges that cross the cut (ordering_build.hpp).
#include <cassert>
#include <cmath>
#include <cstdlib>
#include "ordering_build.hpp"

namespace fgo::ordering {

// minimum vertex cover of a bipartite graph (X: nx vertices with adjacency xptr / xadj2 into Y: ny vertices): Hopcroft-Karp maximum
// matching, then Koenig's construction -- Z = reachable from the unmatched X by alternating paths; cover = (X \ Z) + (Y in Z).
// Returns the membership flags zx / zy of Z.
static void bipartite_cover(int nx, int ny, const std::vector<int> &xptr, const std::vector<int> &xadj2, std::vector<char> &zx, std::vector<char> &zy) {
  std::vector<int> mx((size_t)nx, -1), my((size_t)ny, -1), dist((size_t)nx), q, it((size_t)nx), stack;
  auto bfs_layers = [&]() {
    q.clear();
    bool found = false;
    for (int i = 0; i < nx; ++i) { if (mx[i] < 0) { dist[i] = 0; q.push_back(i); } else dist[i] = -1; }
    for (size_t h = 0; h < q.size(); ++h) {
      const int i = q[h];
      for (int e = xptr[i]; e < xptr[i + 1]; ++e) {
        const int j = my[xadj2[e]];
        if (j < 0) found = true;
        else if (dist[j] < 0) { dist[j] = dist[i] + 1; q.push_back(j); }
      }
    }
    return found;
  };
  auto augment = [&](int root) {                       // iterative DFS along the layers
    stack.clear(); stack.push_back(root);
    while (!stack.empty()) {
      const int i = stack.back();
      if (it[i] == xptr[i + 1]) { dist[i] = -1; stack.pop_back(); continue; }
      const int y = xadj2[it[i]++];
      const int j = my[y];
      if (j < 0) {                                     // free y: flip the path on the stack
        int yy = y;
        for (int k = (int)stack.size() - 1; k >= 0; --k) { const int x = stack[k]; const int prev = mx[x]; mx[x] = yy; my[yy] = x; yy = prev; }
        return true;
      }
      if (dist[j] == dist[i] + 1) stack.push_back(j);
    }
    return false;
  };
  while (bfs_layers()) {
    for (int i = 0; i < nx; ++i) it[i] = xptr[i];
    for (int i = 0; i < nx; ++i) if (mx[i] < 0) augment(i);
  }
  zx.assign((size_t)nx, 0); zy.assign((size_t)ny, 0);
  q.clear();
  for (int i = 0; i < nx; ++i) if (mx[i] < 0) { zx[i] = 1; q.push_back(i); }
  for (size_t h = 0; h < q.size(); ++h) {
    const int i = q[h];
    for (int e = xptr[i]; e < xptr[i + 1]; ++e) {
      const int y = xadj2[e];
      if (zy[y] || mx[i] == y) continue;
      zy[y] = 1;
      const int j = my[y];
      if (j >= 0 && !zx[j]) { zx[j] = 1; q.push_back(j); }
    }
  }
}

// ---- TIME dissection (round 5).  A driver hands the poses over in the order it created them (g2o/g2o_graph.cpp:159-239: the vertex id is
// the key-frame counter), so the vertex index IS time, and a trajectory that does not come back to an earlier place for a while
// leaves cuts "between rank t - 1 and rank t" that are crossed by the odometry / look-back band only.  cfg 2 has such a cut at 33 %
// of the trajectory whose minimum vertex cover is 10 vertices, where the level structures of a BFS -- distorted by every loop
// closure -- settle for a root separator of 101.  Regions stay contiguous in time under these cuts, so the cuts below them stay
// clean as well (mixing them with level cuts does not work: measured, profiles/NOTES.md).  A region is cut at the rank -- smaller
// side >= 30 % of its vertices -- whose crossing edges have the smallest MINIMUM VERTEX COVER (exact for the eight ranks with the fewest
// crossing edges; Hopcroft-Karp + Koenig); no BFS at all.  On five 100k-pose graphs: 20-26 levels instead of 22-32, 0-8 % fewer
// block updates, predicted sweep + backward time -5 .. -15 %.
typedef std::pair<int, int> IntPair;
// in: region S labelled r.  out: ids = S by ascending time, lvl = rank inside the region, diff[t] = crossing edges of cut t minus those of cut t - 1
static void rank_region(const Dissection &d, const std::vector<int> &S, Scratch &sc, int r, std::vector<int> &ids, std::vector<int> &diff) {
  const int n = (int)S.size();
  ids = S;
  if (d.tlabel.empty()) std::sort(ids.begin(), ids.end());
  else std::sort(ids.begin(), ids.end(), [&](int a, int b) { return d.tlabel[(size_t)a] < d.tlabel[(size_t)b]; });
  for (int i = 0; i < n; ++i) sc.lvl[ids[i]] = i;                                   // rank inside the region
  diff.assign((size_t)n + 2, 0);
  for (int i = 0; i < n; ++i) {
    const int v = ids[i];
    for (int p = d.g.xadj[v]; p < d.g.xadj[v + 1]; ++p) {
      const int u = d.g.adj[p];
      if (sc.region[u] != r) continue;
      const int j = sc.lvl[u];
      if (j > i) { diff[(size_t)i + 1]++; diff[(size_t)j + 1]--; }                  // crosses every cut t with i < t <= j
    }
  }
}
// in: diff of a region of n vertices.  out: the candidate cuts (crossing edges, t) inside the balance window, the `nd_time_keep` with the
// fewest crossing edges, best first
static std::vector<IntPair> choose_cuts(const Dissection &d, int n, const std::vector<int> &diff) {
  const double side = d.opt.time_side, wgt = d.opt.time_weight;
  int t_lo = std::max(1, (int)std::ceil(side * n)), t_hi = std::min(n - 1, n - t_lo);
  // (nd_time_weight = w > 0: the balance window is taken in the weight 1 + w * crossing edges instead of in vertices -- a stretch of
  //  the trajectory that many loop closures span will need larger separators further down, i.e. a deeper sub-tree per vertex)
  if (wgt > 0) {
    std::vector<double> acc((size_t)n + 1, 0.0); int cross = 0;
    for (int t = 1; t < n; ++t) { cross += diff[(size_t)t]; acc[(size_t)t] = acc[(size_t)t - 1] + 1.0 + wgt * cross; }
    acc[(size_t)n] = acc[(size_t)n - 1] + 1.0;
    const double tot = acc[(size_t)n];
    t_lo = (int)(std::lower_bound(acc.begin(), acc.end(), side * tot) - acc.begin());
    t_hi = (int)(std::upper_bound(acc.begin(), acc.end(), (1.0 - side) * tot) - acc.begin()) - 1;
    t_lo = std::max(1, std::min(t_lo, n - 1)); t_hi = std::max(t_lo, std::min(t_hi, n - 1));
  }
  std::vector<IntPair> cand; int cross = 0;
  for (int t = 1; t < n; ++t) { cross += diff[(size_t)t]; if (t >= t_lo && t <= t_hi) cand.push_back({cross, t}); }
  const size_t nk = std::min<size_t>((size_t)std::max(1, Settings::get().time_keep), cand.size());
  std::partial_sort(cand.begin(), cand.begin() + (std::ptrdiff_t)nk, cand.end(), [&](const IntPair &x, const IntPair &y) {
    if (x.first != y.first) return x.first < y.first;
    return std::abs(2 * x.second - n) < std::abs(2 * y.second - n);               // ties: the better balanced cut
  });
  cand.resize(nk);
  return cand;
}
// the crossing edges (rank, rank) of ALL kept cuts in one more sweep over the region's edges (a sweep per cut was most of the serial top of the
// ordering: 8 x half the region each): edge (i, j), i < j, crosses the cuts t with i < t <= j.  Left empty if a cut has none: it wins as it is.
static std::vector<std::vector<IntPair>> crossing_edges(const Dissection &d, const Scratch &sc, int r, const std::vector<int> &ids, const std::vector<IntPair> &cand) {
  const size_t nk = cand.size();
  std::vector<std::vector<IntPair>> ces(nk);
  for (size_t c = 0; c < nk; ++c) if (cand[c].first == 0) return ces;
  std::vector<IntPair> ts(nk);                                                     // (t, candidate), ascending t
  for (size_t c = 0; c < nk; ++c) ts[c] = {cand[c].second, (int)c};
  std::sort(ts.begin(), ts.end());
  const int tmin = ts.front().first, tmax = ts.back().first;
  for (size_t c = 0; c < nk; ++c) ces[c].reserve((size_t)cand[c].first);
  for (int i = 0; i < tmax; ++i) {
    const int v = ids[i];
    for (int p = d.g.xadj[v]; p < d.g.xadj[v + 1]; ++p) {
      const int u = d.g.adj[p];
      if (sc.region[u] != r) continue;
      const int j = sc.lvl[u];
      if (j <= i || j < tmin) continue;
      for (size_t q = 0; q < nk; ++q) { const int t = ts[q].first; if (t > j) break; if (t > i) ces[(size_t)ts[q].second].push_back({i, j}); }
    }
  }
  return ces;
}
// in: the crossing edges of one cut (sorted here).  out: the ranks of a minimum vertex cover, left endpoints first, ascending in each part
static void cover_of_cut(std::vector<IntPair> &ce, std::vector<int> &cover) {
  // crossing edges as a bipartite graph: X = their left endpoints (rank < t), Y = their right endpoints
  std::vector<int> X, ys, xptr(1, 0), xadj2;
  std::vector<char> zx, zy;
  std::sort(ce.begin(), ce.end());
  for (auto &e : ce) ys.push_back(e.second);
  std::sort(ys.begin(), ys.end()); ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
  for (size_t k = 0; k < ce.size(); ++k) {
    if (k == 0 || ce[k].first != ce[k - 1].first) { if (k) xptr.push_back((int)xadj2.size()); X.push_back(ce[k].first); }
    xadj2.push_back((int)(std::lower_bound(ys.begin(), ys.end(), ce[k].second) - ys.begin()));
  }
  xptr.push_back((int)xadj2.size());
  bipartite_cover((int)X.size(), (int)ys.size(), xptr, xadj2, zx, zy);
  cover.clear();
  for (size_t i = 0; i < X.size(); ++i) if (!zx[i]) cover.push_back(X[i]);
  for (size_t y = 0; y < ys.size(); ++y) if (zy[y]) cover.push_back(ys[y]);
}
static SplitResult split_by_index(const Dissection &d, const std::vector<int> &S, Scratch &sc, int r, std::vector<int> &A, std::vector<int> &B, std::vector<int> &sep) {
  const int n = (int)S.size();
  std::vector<int> ids, diff, cover, best_cover;
  rank_region(d, S, sc, r, ids, diff);
  std::vector<IntPair> cand = choose_cuts(d, n, diff);
  if (cand.empty()) { d.clear_lvl(ids, sc); return NO_CUT; }
  std::vector<std::vector<IntPair>> ces = crossing_edges(d, sc, r, ids, cand);
  int best_t = -1; size_t best_size = (size_t)-1;
  for (size_t c = 0; c < cand.size(); ++c) {
    const int t = cand[c].second;
    if (cand[c].first == 0) { best_t = t; best_cover.clear(); best_size = 0; break; }   // nothing crosses: the region falls apart here
    cover_of_cut(ces[c], cover);
    if (cover.size() < best_size) { best_size = cover.size(); best_t = t; best_cover = cover; }
  }
  std::vector<char> in_sep((size_t)n, 0);
  for (int q : best_cover) in_sep[(size_t)q] = 1;
  A.clear(); B.clear(); sep.clear();
  for (int i = 0; i < n; ++i) (in_sep[(size_t)i] ? sep : (i < best_t ? A : B)).push_back(ids[i]);
  d.clear_lvl(ids, sc);
  if (A.empty() || B.empty()) return NO_CUT;
  sc.stats.n[ND_INDEX_CUTS]++; sc.stats.n[ND_INDEX_CUTS_CLEAN] += best_size == 0;
  return SPLIT;
}

// ---- level cuts.  Candidate separators of a level structure: the vertices of level l that touch level l+1 ("forward": the rest of level l
// joins the near side) or those that touch level l-1 ("backward": the rest joins the far side); scored by their trimmed size with a
// penalty for unbalanced parts
struct LevelCut { int level = -1, dir = 0, start = -1; double score = 1e300; int other() const { return dir == 0 ? level + 1 : level - 1; } };   // other: the level the separator touches
// pseudo-peripheral start: re-run BFS from the last vertex the connectivity sweep reached (two sweeps)
static int pseudo_peripheral(const Dissection &d, int r, Scratch &sc) {
  const int far = sc.bfs_order.back();
  d.clear_lvl(sc.bfs_order, sc); d.bfs(far, r, sc.bfs_order, sc);
  const int start = sc.bfs_order.back();
  d.clear_lvl(sc.bfs_order, sc);
  return start;
}
// The level structure rooted at `from` (left in lvl / bfs_order) and its best cut against `best`; returns the number of the last level.
static int evaluate(const Dissection &d, int from, int r, int n, Scratch &sc, LevelCut &best) {
  std::vector<int> &bfs_order = sc.bfs_order, &lvl = sc.lvl, &cnt = sc.cnt, &tf = sc.tf, &tb = sc.tb;
  // BFS and the per-level counts in one sweep: when v (level l) leaves the queue every vertex of level l - 1 is labelled,
  // and a neighbour of level l + 1 is either labelled already or gets its label from v right now
  cnt.clear(); tf.clear(); tb.clear();
  bfs_order.assign(1, from); lvl[from] = 0;
  int ml = 0;
  for (size_t head = 0; head < bfs_order.size(); ++head) {
    const int v = bfs_order[head], l = lvl[v];
    if (l >= (int)cnt.size()) { cnt.push_back(0); tf.push_back(0); tb.push_back(0); }
    cnt[l]++;
    bool up = false, down = false;
    for (int p = d.g.xadj[v]; p < d.g.xadj[v + 1]; ++p) {
      const int u = d.g.adj[p];
      if (sc.region[u] != r) continue;
      if (lvl[u] < 0) { lvl[u] = l + 1; ml = l + 1; bfs_order.push_back(u); up = true; }
      else { up = up || lvl[u] == l + 1; down = down || lvl[u] == l - 1; }
    }
    tf[l] += up; tb[l] += down;
  }
  if (ml < 2) return ml;
  const double min_side = Settings::get().min_side;
  int before = 0;
  for (int l = 0; l <= ml; ++l) {
    const int after = n - before - cnt[l];
    if (l >= 1 && l < ml && before > 0 && after > 0) {
      for (int dir = 0; dir < 2; ++dir) {
        const int sz = dir == 0 ? tf[l] : tb[l];
        const int na = dir == 0 ? before + cnt[l] - sz : before, nb2 = dir == 0 ? after : after + cnt[l] - sz;
        const double bal = (double)std::abs(na - nb2) / n;      // 0 = perfect balance
        double score = sz * (1.0 + d.opt.bal_w * std::max(0.0, bal - d.opt.bal_t));
        // Mesh-like graphs (a torus, a 2-D grid): the level sizes GROW from the root, so the first levels are tiny and
        // win on size against any penalty that is linear in the imbalance -- the dissection then peels one vertex at a
        // time (etree height n / 2, fill n^1.5: measured on a 40 x 40 torus).  A cut whose smaller side holds less than
        // min_side of the region only competes among its own kind (used if nothing better exists).
        if (std::min(na, nb2) < min_side * n) score += 1e12;
        if (score < best.score) { best.score = score; best.level = l; best.dir = dir; best.start = from; }
      }
    }
    before += cnt[l];
  }
  return ml;
}
// The level structures of the other starts -- the far end of the first one, i.e. BOTH ends of the pseudo-diameter; nd_starts 3 / 4: the
// ends of a second one -- compete for `best`; lvl / bfs_order are left holding the winner's.
static void try_other_starts(const Dissection &d, const std::vector<int> &S, int r, int start, Scratch &sc, LevelCut &best) {
  const int n = (int)S.size(), n_starts = Settings::get().starts;
  std::vector<int> &bfs_order = sc.bfs_order, &lvl = sc.lvl;
  int last = bfs_order.back();
  // the first level structure is kept (order and levels: two copies instead of one more sweep if it wins)
  std::vector<int> &order1 = sc.order1, &lvl1 = sc.lvl1;
  order1 = bfs_order;
  lvl1.resize(order1.size());
  for (size_t i = 0; i < order1.size(); ++i) lvl1[i] = lvl[order1[i]];
  d.clear_lvl(bfs_order, sc);
  evaluate(d, last, r, n, sc, best);
  if (n_starts > 2) {                                         // a second pseudo-diameter, swept from the middle of the region
    d.clear_lvl(bfs_order, sc); d.bfs(S[S.size() / 2], r, bfs_order, sc);
    last = bfs_order.back();
    d.clear_lvl(bfs_order, sc);
    evaluate(d, last, r, n, sc, best);
    if (n_starts > 3) { last = bfs_order.back(); d.clear_lvl(bfs_order, sc); evaluate(d, last, r, n, sc, best); }
  }
  if (best.start == last) return;
  d.clear_lvl(bfs_order, sc);                                 // back to the winner's levels
  if (best.start == start) { bfs_order = order1; for (size_t i = 0; i < order1.size(); ++i) lvl[order1[i]] = lvl1[i]; sc.stats.n[ND_RESTORE_COPY]++; }
  else { d.bfs(best.start, r, bfs_order, sc); sc.stats.n[ND_RESTORE_BFS]++; }
}
// the cut of the level structure in lvl -> A, B, sep: separator = the cut level trimmed to the vertices that touch the far side, then
// refined by a minimum cover (nd_cover).  Returns whether the cover shrank the separator.
static bool materialize(const Dissection &d, int r, const LevelCut &cut, Scratch &sc, std::vector<int> &A, std::vector<int> &B, std::vector<int> &sep) {
  std::vector<int> &lvl = sc.lvl;
  const int other = cut.other();
  A.clear(); B.clear(); sep.clear();
  for (int v : sc.bfs_order) {
    if (lvl[v] < cut.level) A.push_back(v);
    else if (lvl[v] > cut.level) B.push_back(v);
    else {
      bool touches = false;
      for (int p = d.g.xadj[v]; p < d.g.xadj[v + 1] && !touches; ++p) {
        int u = d.g.adj[p];
        if (sc.region[u] == r && lvl[u] == other) touches = true;
      }
      (touches ? sep : (cut.dir == 0 ? A : B)).push_back(v);
    }
  }
  if (!Settings::get().cover || sep.size() < 2) return false;
  // The trimmed level X is ONE vertex cover of the edges between it and the far side's neighbours Y; a MINIMUM vertex cover of
  // that bipartite graph (maximum matching + Koenig's construction) separates the same two sides with fewer vertices: X minus
  // the cover joins the near side, the cover's part of Y leaves the far side.
  std::vector<int> &nearv = cut.dir == 0 ? A : B, &farv = cut.dir == 0 ? B : A;
  constexpr int XB = 1 << 29, YB = 1 << 30;
  const int nx = (int)sep.size();
  const std::vector<int> Xv = sep;
  std::vector<int> Y, xptr((size_t)nx + 1, 0), xadj2;
  for (int i = 0; i < nx; ++i) lvl[sep[i]] = XB + i;
  for (int i = 0; i < nx; ++i) {
    const int v = sep[i];
    for (int p = d.g.xadj[v]; p < d.g.xadj[v + 1]; ++p) {
      const int u = d.g.adj[p];
      if (sc.region[u] != r) continue;
      if (lvl[u] == other) { lvl[u] = YB + (int)Y.size(); Y.push_back(u); }
      if (lvl[u] >= YB) xadj2.push_back(lvl[u] - YB);
    }
    xptr[(size_t)i + 1] = (int)xadj2.size();
  }
  const int ny = (int)Y.size();
  std::vector<char> zx, zy;
  bipartite_cover(nx, ny, xptr, xadj2, zx, zy);
  int csize = 0;
  for (int i = 0; i < nx; ++i) csize += !zx[i];
  for (int y = 0; y < ny; ++y) csize += zy[y];
  if (csize < nx) {
    std::vector<int> nsep;
    for (int i = 0; i < nx; ++i) (zx[i] ? nearv : nsep).push_back(sep[i]);
    size_t w = 0;
    for (size_t k = 0; k < farv.size(); ++k) {
      const int u = farv[k];
      if (lvl[u] >= YB && zy[lvl[u] - YB]) nsep.push_back(u); else farv[w++] = u;
    }
    farv.resize(w);
    sep.swap(nsep);
  }
  for (int i = 0; i < nx; ++i) lvl[Xv[i]] = cut.level;          // (the level structure serves the next candidate)
  for (int u : Y) lvl[u] = other;
  return csize < nx;
}

// One bisection of the region S.  Time mode: by index.  Otherwise by a BFS level structure from a pseudo-peripheral vertex; DISCONNECTED
// leaves the component of S[0] in sc.bfs_order (levels set) and the region label r on all of S.
SplitResult Dissection::split(const std::vector<int> &S, Scratch &sc, int &r, std::vector<int> &A, std::vector<int> &B, std::vector<int> &sep) {
  prepare(sc);
  r = next_region++;
  for (int v : S) sc.region[v] = r;
  if (time_mode) return split_by_index(*this, S, sc, r, A, B, sep);
  bfs(S[0], r, sc.bfs_order, sc);
  if (sc.bfs_order.size() < S.size()) { sc.stats.n[ND_DISCONNECTED]++; return DISCONNECTED; }
  const int start = pseudo_peripheral(*this, r, sc);
  LevelCut best;
  if (evaluate(*this, start, r, (int)S.size(), sc, best) < 2) { clear_lvl(sc.bfs_order, sc); return NO_CUT; }   // (near-)clique: no useful cut
  if (Settings::get().starts > 1) try_other_starts(*this, S, r, start, sc, best);
  assert(best.level >= 1);           // two levels or more below the root: level 1 has vertices on both sides
  // (the three / six best cuts by trimmed size, compared again after the refinement: 0.5 % less fill, but the level count moves
  //  by +-1-2 either way -- predicted sweep times 3 721 / 3 788 / 3 779 us on cfg 2, three other seeds alike; not kept)
  sc.stats.n[ND_LEVEL_CUTS]++; sc.stats.n[ND_LEVEL_CUTS_COVER] += materialize(*this, r, best, sc, A, B, sep);
  clear_lvl(sc.bfs_order, sc);
  return SPLIT;
}

}  // namespace fgo::ordering
