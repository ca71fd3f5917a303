// Stand-alone check of the host walk of a partial ISAM2 update (graph_slam_amd/csrc/isam_dirty.cpp): reads no files, generates
// its cases from seeds.  Every case runs several CONSECUTIVE calls on the same flag buffer and set lists; after each call the
// whole task_dirty / col_dirty / affected arrays are compared byte for byte with a dense recomputation from the definition
//   affected      = new variables + variables of new factors + moved + everything that shares a factor with a moved variable
//   dirty columns = the columns of the affected and all their ancestors in the elimination tree
//   dirty tasks   = the tasks of those columns;  dirty columns closed over whole tasks
// so an entry that a call forgets to clear (the arrays are all-zero between calls, set and cleared sparsely) shows in the next one.
//   g++ -O1 -g -std=c++17 [-fsanitize=address,undefined] -I. tools/isam_dirty_check.cpp graph_slam_amd/csrc/isam_dirty.cpp
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include "graph_slam_amd/csrc/isam_dirty.hpp"

using namespace fgo;

namespace {

struct Factor { std::vector<int> v; int born; };            // 2 variables: binary, 6: IMU, 1: prior; born: the call that adds it
struct World {
  int64_t NX = 0;
  std::vector<int> pose_col, parent, col_task, task_ptr, task_cols;
  std::vector<Factor> fac;
};
struct Call { int64_t N; std::vector<int64_t> moved; bool look; double full_frac; };

int nb_of(const World &W) { return (int)W.parent.size(); }
int ntask_of(const World &W) { return (int)W.task_ptr.size() - 1; }

// columns for the variables not in `fixed` (in the order `perm`, or identity), tasks from groups of columns
void lay_out(World &W, int64_t NX, const std::vector<int> &fixed, const std::vector<int> &parent, const std::vector<std::vector<int>> &tasks,
             const std::vector<int> *perm = nullptr) {
  W.NX = NX; W.parent = parent;
  W.pose_col.assign((size_t)NX, -1);
  int k = 0;
  for (int64_t i = 0; i < NX; ++i) {
    const int v = perm ? (*perm)[(size_t)i] : (int)i;
    if (std::find(fixed.begin(), fixed.end(), v) == fixed.end()) W.pose_col[(size_t)v] = k++;
  }
  if (k != nb_of(W)) { std::fprintf(stderr, "generator: %d columns for a tree of %d\n", k, nb_of(W)); std::exit(2); }
  W.col_task.assign((size_t)k, -1); W.task_ptr = {0}; W.task_cols.clear();
  for (size_t t = 0; t < tasks.size(); ++t) {
    for (int c : tasks[t]) { W.col_task[(size_t)c] = (int)t; W.task_cols.push_back(c); }
    W.task_ptr.push_back((int)W.task_cols.size());
  }
}
std::vector<std::vector<int>> single_tasks(int nb) { std::vector<std::vector<int>> t; for (int k = 0; k < nb; ++k) t.push_back({k}); return t; }
std::vector<int> chain_tree(int nb) { std::vector<int> p((size_t)nb); for (int k = 0; k < nb; ++k) p[(size_t)k] = k + 1 < nb ? k + 1 : -1; return p; }
int born_with(const std::vector<int> &v, const std::vector<Call> &calls) {      // the first call at which all of v exist
  const int top = *std::max_element(v.begin(), v.end());
  for (size_t c = 0; c < calls.size(); ++c) if (top < calls[c].N) return (int)c;
  std::fprintf(stderr, "generator: factor on variable %d that no call adds\n", top); std::exit(2);
}

// ---- dense recomputation from the definition, into fresh arrays
struct Expect { std::vector<unsigned char> aff, col, task; int64_t n_tasks; };
Expect expect(const World &W, const std::vector<Call> &calls, size_t ci) {
  const Call &C = calls[ci];
  const int nb = nb_of(W), ntask = ntask_of(W);
  Expect X{std::vector<unsigned char>((size_t)W.NX, 0), std::vector<unsigned char>((size_t)nb, 0), std::vector<unsigned char>((size_t)ntask, 0), 0};
  std::vector<unsigned char> moved((size_t)W.NX, 0);
  for (int64_t v : C.moved) moved[(size_t)v] = 1;
  for (int64_t v = ci ? calls[ci - 1].N : 0; v < C.N; ++v) X.aff[(size_t)v] = 1;
  for (int64_t v = 0; v < C.N; ++v) if (moved[(size_t)v]) X.aff[(size_t)v] = 1;
  for (const Factor &f : W.fac) {
    if (f.born > (int)ci) continue;
    bool hit = f.born == (int)ci;
    if (f.v.size() > 1) for (int v : f.v) hit = hit || moved[(size_t)v];       // (a prior couples nothing)
    if (hit) for (int v : f.v) X.aff[(size_t)v] = 1;
  }
  for (int64_t v = 0; v < W.NX; ++v)
    if (X.aff[(size_t)v]) for (int k = W.pose_col[(size_t)v]; k >= 0; k = W.parent[(size_t)k]) X.col[(size_t)k] = 1;   // (the whole path, no early stop)
  for (int k = 0; k < nb; ++k) if (X.col[(size_t)k]) X.task[(size_t)W.col_task[(size_t)k]] = 1;
  for (int t = 0; t < ntask; ++t) {
    if (!X.task[(size_t)t]) continue;
    ++X.n_tasks;
    for (int q = W.task_ptr[(size_t)t]; q < W.task_ptr[(size_t)t + 1]; ++q) X.col[(size_t)W.task_cols[(size_t)q]] = 1;
  }
  if (X.n_tasks > (int64_t)(C.full_frac * ntask)) X.n_tasks = -2;
  return X;
}

int n_cases = 0, n_calls = 0, n_bad = 0, n_full = 0, n_empty = 0;

bool same(const char *name, size_t ci, const char *what, const unsigned char *got, const std::vector<unsigned char> &want) {
  for (size_t i = 0; i < want.size(); ++i)
    if (got[i] != want[i]) { std::printf("FAIL %s call %zu: %s[%zu] = %d, expected %d\n", name, ci, what, i, got[i], want[i]); return false; }
  return true;
}

void run_case(const std::string &name, World W, std::vector<Call> calls) {
  ++n_cases;
  for (Factor &f : W.fac) f.born = std::max(f.born, born_with(f.v, calls));
  std::stable_sort(W.fac.begin(), W.fac.end(), [](const Factor &a, const Factor &b) { return a.born < b.born; });
  const int nb = nb_of(W), ntask = ntask_of(W);
  // one allocation of exactly the reported size: a sanitised build sees a view that reaches past it
  std::vector<unsigned char> buf(isam_flags(nullptr, W.NX, ntask, nb).bytes, 0);
  const IsamFlags F = isam_flags(buf.data(), W.NX, ntask, nb);
  {                                                          // the five arrays tile the allocation
    std::vector<std::pair<const unsigned char *, size_t>> r = {{F.moved, (size_t)W.NX}, {F.task_dirty, (size_t)ntask}, {F.col_dirty, (size_t)nb}, {F.moved_next, (size_t)W.NX}, {F.affected, (size_t)W.NX}};
    std::sort(r.begin(), r.end());
    const unsigned char *at = buf.data();
    for (auto &x : r) { if (x.first != at) { std::printf("FAIL %s: the flag arrays do not tile their allocation\n", name.c_str()); ++n_bad; return; } at += x.second; }
    if (at != buf.data() + F.bytes || F.bytes != buf.size()) { std::printf("FAIL %s: byte count of the flag arrays\n", name.c_str()); ++n_bad; return; }
  }
  IsamSets set;
  IsamAdded seen{0, 0, 0, 0};
  for (size_t ci = 0; ci < calls.size(); ++ci) {
    ++n_calls;
    const Call &C = calls[ci];
    std::vector<int> ei, ej, imu_ids, prior_v, he, imu_inc;   // the factors this call knows, and their incidence lists
    std::vector<std::vector<int>> inc_e((size_t)W.NX), inc_f((size_t)W.NX);
    for (const Factor &f : W.fac) {
      if (f.born > (int)ci) break;
      if (f.v.size() == 2) { for (int s = 0; s < 2; ++s) inc_e[(size_t)f.v[(size_t)s]].push_back((int)ei.size() << 1 | s); ei.push_back(f.v[0]); ej.push_back(f.v[1]); }
      else if (f.v.size() == 6) { for (int s = 0; s < 6; ++s) inc_f[(size_t)f.v[(size_t)s]].push_back((int)(imu_ids.size() / 6) << 3 | s); imu_ids.insert(imu_ids.end(), f.v.begin(), f.v.end()); }
      else prior_v.push_back(f.v[0]);
    }
    std::vector<int64_t> he_ptr = {0}, imu_inc_ptr = {0};
    for (int64_t v = 0; v < W.NX; ++v) {
      he.insert(he.end(), inc_e[(size_t)v].begin(), inc_e[(size_t)v].end()); he_ptr.push_back((int64_t)he.size());
      imu_inc.insert(imu_inc.end(), inc_f[(size_t)v].begin(), inc_f[(size_t)v].end()); imu_inc_ptr.push_back((int64_t)imu_inc.size());
    }
    // what moved arrives in one of two arrays (look-ahead or not); the other holds rubbish that must be neither read nor written
    unsigned char *mv = C.look ? F.moved_next : F.moved, *other = C.look ? F.moved : F.moved_next;
    std::memset(mv, 0, (size_t)W.NX); std::memset(other, 0xAB, (size_t)W.NX);
    for (int64_t v : C.moved) mv[v] = 1;
    const std::vector<unsigned char> mv_before(mv, mv + W.NX), other_before(other, other + W.NX);
    const IsamGraph G{C.N, ei, ej, imu_ids, prior_v, he_ptr, he, imu_inc_ptr, imu_inc, W.pose_col, W.parent, W.col_task, W.task_ptr, W.task_cols};
    isam_mark_added(F, G, seen, set);
    const int64_t got = isam_dirty_tasks(F, mv, G, set, C.full_frac);
    seen = IsamAdded{C.N, (int64_t)ei.size(), (int64_t)imu_ids.size() / 6, (int64_t)prior_v.size()};
    const Expect X = expect(W, calls, ci);
    bool ok = same(name.c_str(), ci, "task_dirty", F.task_dirty, X.task) && same(name.c_str(), ci, "col_dirty", F.col_dirty, X.col) &&
              same(name.c_str(), ci, "affected", F.affected, X.aff) && same(name.c_str(), ci, "moved (input)", mv, mv_before) &&
              same(name.c_str(), ci, "the other moved array", other, other_before);
    if (got != X.n_tasks) { std::printf("FAIL %s call %zu: returned %lld dirty tasks, expected %lld\n", name.c_str(), ci, (long long)got, (long long)X.n_tasks); ok = false; }
    // the set lists name exactly the entries that are set, each once: that is what the next call clears
    const size_t na = (size_t)std::count(X.aff.begin(), X.aff.end(), 1), nc = (size_t)std::count(X.col.begin(), X.col.end(), 1), nt = (size_t)std::count(X.task.begin(), X.task.end(), 1);
    if (set.aff.size() != na || set.cols.size() != nc || set.tasks.size() != nt) { std::printf("FAIL %s call %zu: set lists of %zu / %zu / %zu entries for %zu / %zu / %zu flags\n", name.c_str(), ci, set.aff.size(), set.cols.size(), set.tasks.size(), na, nc, nt); ok = false; }
    n_full += got == -2; n_empty += got == 0;
    if (!ok) { ++n_bad; return; }
  }
}

// ---- the cases
std::vector<Factor> chain_edges(int64_t n) { std::vector<Factor> f; for (int v = 0; v + 1 < n; ++v) f.push_back({{v, v + 1}, 0}); return f; }

void scan_cases() {                                          // the eight-byte scan of `moved` and its tail
  for (int N : {1, 7, 8, 9, 16, 17}) {
    World W; lay_out(W, N, {}, chain_tree(N), single_tasks(N)); W.fac = chain_edges(N);
    std::vector<Call> calls = {{N, {}, false, 2.0}};
    std::vector<int64_t> all;
    for (int64_t i : {0, 7, 8, N - 1}) if (i < N) { calls.push_back({N, {i}, calls.size() % 2 == 1, 2.0}); if (std::find(all.begin(), all.end(), i) == all.end()) all.push_back(i); }
    calls.push_back({N, all, false, 2.0}); calls.push_back({N, {}, true, 2.0}); calls.push_back({N, all, true, 2.0});
    run_case("scan N=" + std::to_string(N), W, calls);
  }
}

void shaped_cases() {
  { World W; lay_out(W, 14, {}, chain_tree(14), single_tasks(14)); W.fac = chain_edges(9);             // phantom slots: NX > N, they are columns too
    run_case("phantom slots", W, {{8, {}, false, 2.0}, {9, {8}, false, 2.0}, {9, {0, 7}, true, 2.0}, {9, {}, false, 2.0}}); }
  { World W; lay_out(W, 12, {}, chain_tree(12), single_tasks(12)); W.fac = chain_edges(12);            // a single chain, growing
    run_case("chain", W, {{10, {}, false, 2.0}, {10, {4}, false, 2.0}, {11, {}, true, 2.0}, {12, {11}, false, 2.0}, {12, {}, true, 2.0}}); }
  { World W; std::vector<int> par(40, 39); par[39] = -1;                                                // a star: hub 0 with a long incidence list
    std::vector<int> perm(40); for (int i = 0; i < 40; ++i) perm[(size_t)i] = (i + 1) % 40;              // (the hub is eliminated last)
    lay_out(W, 40, {}, par, single_tasks(40), &perm); for (int v = 1; v < 40; ++v) W.fac.push_back({{0, v}, 0});
    run_case("star", W, {{40, {}, false, 2.0}, {40, {5}, false, 2.0}, {40, {0}, true, 2.0}, {40, {}, false, 2.0}, {40, {39, 1}, false, 2.0}}); }
  { World W; std::vector<int> par = {1, 2, -1, 4, 5, -1};                                               // a forest with two roots
    lay_out(W, 6, {}, par, single_tasks(6)); W.fac = {{{0, 1}, 0}, {{1, 2}, 0}, {{3, 4}, 0}, {{4, 5}, 0}, {{5}, 3}};
    run_case("two roots", W, {{6, {}, false, 2.0}, {6, {0}, false, 2.0}, {6, {3}, true, 2.0}, {6, {}, false, 2.0}, {6, {2, 5}, false, 2.0}}); }
  { World W; std::vector<int> par = {2, 2, 4, 4, -1};                                                   // a task of several columns, one of them an ancestor
    lay_out(W, 5, {}, par, {{0, 1}, {2, 3}, {4}}); W.fac = {{{0, 2}, 0}, {{1, 2}, 0}, {{3, 4}, 0}};
    run_case("task closure", W, {{5, {}, false, 2.0}, {5, {}, false, 2.0}, {5, {0}, false, 2.0}, {5, {}, true, 2.0}, {5, {3}, true, 2.0}, {5, {1}, false, 2.0}}); }
  { World W; lay_out(W, 6, {0, 3}, chain_tree(4), {{0}, {1, 2}, {3}}); W.fac = chain_edges(6); W.fac.push_back({{0}, 0});   // fixed variables: no column
    run_case("fixed variables", W, {{6, {}, false, 2.0}, {6, {0}, false, 2.0}, {6, {3}, true, 2.0}, {6, {1}, false, 2.0}, {6, {}, false, 2.0}}); }
  { World W; lay_out(W, 10, {}, chain_tree(10), single_tasks(10)); W.fac = chain_edges(10);             // the full_frac threshold: 3 of 10 tasks pass, 4 do not
    run_case("full_frac", W, {{10, {}, false, 2.0}, {10, {8}, false, 0.3}, {10, {7}, false, 0.3}, {10, {}, false, 0.3}, {10, {2}, true, 0.3}, {10, {9}, true, 0.3}, {10, {}, false, 0.0}}); }
  { World W; lay_out(W, 20, {}, chain_tree(20), single_tasks(20));                                      // IMU factors: six variables each
    for (int k = 0; k + 6 <= 18; k += 3) W.fac.push_back({{k, k + 1, k + 2, k + 3, k + 4, k + 5}, 0});
    W.fac.push_back({{14, 15, 16, 17, 18, 19}, 3}); W.fac.push_back({{0, 19}, 4});
    run_case("imu", W, {{18, {}, false, 2.0}, {18, {4}, false, 2.0}, {18, {}, true, 2.0}, {20, {}, false, 2.0}, {20, {17}, true, 2.0}, {20, {}, false, 2.0}}); }
}

void random_cases(int n_seeds) {
  for (int seed = 1; seed <= n_seeds; ++seed) {
    std::mt19937_64 rng((uint64_t)seed);
    auto rnd = [&](int n) { return (int)(rng() % (uint64_t)n); };
    const int N0 = 1 + rnd(30), n_calls_ = 4 + rnd(5), NX = N0 + n_calls_ + rnd(6);
    std::vector<int> fixed, perm((size_t)NX);
    for (int v = 0; v < NX; ++v) { perm[(size_t)v] = v; if (NX > 3 && rnd(12) == 0) fixed.push_back(v); }
    std::shuffle(perm.begin(), perm.end(), rng);
    const int nb = NX - (int)fixed.size();
    std::vector<int> par((size_t)nb), cols((size_t)nb);
    for (int k = 0; k < nb; ++k) { par[(size_t)k] = (k + 1 == nb || rnd(15) == 0) ? -1 : k + 1 + rnd(std::min(4, nb - k - 1)); cols[(size_t)k] = k; }
    std::shuffle(cols.begin(), cols.end(), rng);
    std::vector<std::vector<int>> tasks;
    for (int q = 0; q < nb;) { const int n = std::min(nb - q, 1 + rnd(4)); tasks.emplace_back(cols.begin() + q, cols.begin() + q + n); q += n; }
    World W; lay_out(W, NX, fixed, par, tasks, &perm);
    std::vector<Call> calls;
    int N = N0;
    for (int c = 0; c < n_calls_; ++c) {
      if (c && rnd(2)) ++N;
      Call C{N, {}, rnd(2) == 1, rnd(4) == 0 ? 0.3 : 2.0};
      const int nm = rnd(3) == 0 ? 0 : rnd(4);
      for (int m = 0; m < nm; ++m) { const int64_t v = rnd(N); if (std::find(C.moved.begin(), C.moved.end(), v) == C.moved.end()) C.moved.push_back(v); }
      calls.push_back(C);
    }
    for (int v = 1; v < N; ++v) { W.fac.push_back({{v - 1 - rnd(std::min(v, 3)), v}, 0}); if (rnd(6) == 0) W.fac.push_back({{rnd(v), v}, rnd(n_calls_)}); }
    for (int f = 0, nf = N >= 6 ? rnd(4) : 0; f < nf; ++f) { const int a = rnd(N - 5); W.fac.push_back({{a, a + 1, a + 2, a + 3, a + 4, a + 5}, rnd(n_calls_)}); }
    for (int p = 0, np = rnd(3); p < np; ++p) W.fac.push_back({{rnd(N)}, rnd(n_calls_)});
    run_case("random seed " + std::to_string(seed), W, calls);
  }
}

}  // namespace

int main() {
  scan_cases();
  shaped_cases();
  random_cases(300);
  std::printf("isam_dirty_check: %d cases, %d calls (%d with an empty dirty set, %d over the full-sweep threshold), %d failed\n", n_cases, n_calls, n_empty, n_full, n_bad);
  return n_bad ? 1 : 0;
}
