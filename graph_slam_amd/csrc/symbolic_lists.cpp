// Symbolic phase, part 3: the update lists filled and split [external | internal], the accumulate targets of every level and the
// column-group lists of the very wide levels (symbolic_build.hpp; symbolic.cpp is the driver).
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "symbolic_build.hpp"

namespace fgo {
namespace symbolic {

// ---- fill the update lists, split [external | internal]: external sources live in other (earlier level) tasks and
// are applied by the wide accumulate kernel, internal ones by the task's own workgroup.  Both parts in ascending
// source column order: externals are written from the front, internals from the back and then reversed.
void fill_update_lists(Symbolic &S, const BuildState &st) {
  const std::vector<int> &task_of = st.task_of;
  S.op_a.resize(S.nops);
  S.op_b.resize(S.nops);
  S.op_mid.resize(S.nnzL);
  parallel_ranges(S.nb, 512, [&](int kb, int ke) {
    std::vector<int64_t> front, back;
    for (int k = kb; k < ke; ++k) {
      const int64_t k0 = S.colptr[k], k1 = S.colptr[k + 1];
      const int T = task_of[k];
      front.assign(S.op_ptr.begin() + k0, S.op_ptr.begin() + k1);
      back.assign(S.op_ptr.begin() + k0 + 1, S.op_ptr.begin() + k1 + 1);
      for_each_op_of_column(S, k, [&](int64_t u, int64_t t, int64_t s) {
        const int64_t o = (task_of[S.blkcol[t]] != T) ? front[u - k0]++ : --back[u - k0];
        S.op_a[o] = (int)t; S.op_b[o] = (int)s;
      });
      for (int64_t u = k0; u < k1; ++u) {
        S.op_mid[u] = front[u - k0];
        std::reverse(S.op_a.begin() + S.op_mid[u], S.op_a.begin() + S.op_ptr[u + 1]);
        std::reverse(S.op_b.begin() + S.op_mid[u], S.op_b.begin() + S.op_ptr[u + 1]);
      }
    }
  });
}

// per level: targets, external updates, the longest list, and how many updates come from the level directly below
// (tools/acc_stats.py; profiles/NOTES.md "staged accumulate")
static void print_acc_stats(const Symbolic &S, const BuildState &st) {
  for (int l = 0; l < n_levels(S); ++l) {
    int64_t nt = S.acc_ptr[l + 1] - S.acc_ptr[l], ops = 0, mx = 0, late = 0, mxlate = 0;
    for (int64_t q = S.acc_ptr[l]; q < S.acc_ptr[l + 1]; ++q) {
      const int b = S.acc_targets[q];
      int64_t n = 0, nl = 0;
      for (int64_t o = S.op_mid[b] - ext_ops(S, st, b); o < S.op_mid[b]; ++o) {
        ++n;
        if (st.tlevel[st.task_of[S.blkcol[S.op_a[o]]]] == l - 1) ++nl;
      }
      ops += n; late += nl; mx = std::max(mx, n); mxlate = std::max(mxlate, nl);
    }
    // distinct source blocks of the level: what it has to fetch at least once
    std::vector<int> srcs;
    for (int64_t q = S.acc_ptr[l]; q < S.acc_ptr[l + 1]; ++q) {
      const int b = S.acc_targets[q];
      for (int64_t o = S.op_mid[b] - ext_ops(S, st, b); o < S.op_mid[b]; ++o) { srcs.push_back(S.op_a[o]); srcs.push_back(S.op_b[o]); }
    }
    std::sort(srcs.begin(), srcs.end());
    const int64_t distinct = (int64_t)(std::unique(srcs.begin(), srcs.end()) - srcs.begin());
    {   // columns per task: how full the panels of the level are
      int hist[4] = {0, 0, 0, 0};      // 1-4, 5-8, 9-12, 13-16(+)
      int64_t cols = 0;
      for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t) { const int m = S.task_ptr[t + 1] - S.task_ptr[t]; cols += m; hist[std::min(3, (m - 1) / 4)]++; }
      std::fprintf(stderr, "[acc] level %d columns %lld, tasks with 1-4 / 5-8 / 9-12 / 13+ columns: %d %d %d %d\n", l, (long long)cols, hist[0], hist[1], hist[2], hist[3]);
    }
    std::fprintf(stderr, "[acc] level %d tasks %d targets %lld updates %lld longest list %lld from the level below %lld (longest %lld) distinct sources %lld (%.1f MB)\n", l,
                 S.level_ptr[l + 1] - S.level_ptr[l], (long long)nt, (long long)ops, (long long)mx, (long long)late, (long long)mxlate,
                 (long long)distinct, 288e-6 * (double)distinct);
  }
}

// per level: targets that have external ops
void accumulate_targets(Symbolic &S, const BuildState &st) {
  const int nb = S.nb, nlevels = n_levels(S);
  S.acc_ptr.assign(nlevels + 1, 0);
  // (two passes over the columns in task order -- count, prefix, fill -- both in parallel; the order is the serial one)
  std::vector<int64_t> col_nt((size_t)nb + 1, 0);                 // targets of the q-th entry of task_cols
  parallel_ranges(nb, 1024, [&](int q0, int q1) {
    for (int q = q0; q < q1; ++q) {
      const int k = S.task_cols[q];
      int64_t n = 0;
      for (int64_t b = S.colptr[k]; b < S.colptr[k + 1]; ++b) n += ext_ops(S, st, b) > 0;
      col_nt[(size_t)q + 1] = n;
    }
  });
  for (int q = 0; q < nb; ++q) col_nt[(size_t)q + 1] += col_nt[q];
  S.acc_targets.resize((size_t)col_nt[nb]);
  parallel_ranges(nb, 1024, [&](int q0, int q1) {
    for (int q = q0; q < q1; ++q) {
      const int k = S.task_cols[q];
      int64_t w = col_nt[q];
      for (int64_t b = S.colptr[k]; b < S.colptr[k + 1]; ++b) if (ext_ops(S, st, b) > 0) S.acc_targets[(size_t)w++] = (int)b;
    }
  });
  for (int l = 0; l < nlevels; ++l) {
    S.acc_ptr[l + 1] = col_nt[S.task_ptr[S.level_ptr[l + 1]]];
    // long source lists last: they get a whole workgroup each (hub columns, the top separators)
    static const int64_t long_ops = (int64_t)tune("acc_long", ACC_LONG_OPS);
    auto first_long = std::stable_partition(S.acc_targets.begin() + S.acc_ptr[l], S.acc_targets.begin() + S.acc_ptr[l + 1],
                                            [&](int b) { return ext_ops(S, st, b) <= long_ops; });
    S.acc_mid.push_back((int64_t)(first_long - S.acc_targets.begin()));
  }
  if (tune("acc_stats", 0) != 0) print_acc_stats(S, st);
}

// pass 1 of column_group_lists(): groups and entries of a chunk of 64 columns of a level
struct ChunkOut { std::vector<int> tgt, b, a; std::vector<int64_t> ptr; };

// groups and entries of column k, appended to o
static void column_groups(const Symbolic &S, const BuildState &st, int k, std::vector<int> &T, ChunkOut &o) {
  T.clear();
  for (int64_t u = S.colptr[k]; u < S.colptr[k + 1]; ++u) if (ext_ops(S, st, u) > 0) T.push_back((int)u);
  if (T.empty()) return;
  const int ng = ((int)T.size() + ACC2_G - 1) / ACC2_G;
  const size_t tg0 = o.tgt.size();
  o.tgt.resize(tg0 + (size_t)ng * ACC2_G, -1);
  for (size_t x = 0; x < T.size(); ++x) o.tgt[tg0 + x] = T[x];
  // entries per group, ascending source column: a 10-way merge of the targets' (already filled, ascending) external
  // update lists -- op_b = block (k, j) is the same for all targets of a source column and ascends with j
  for (int gq = 0; gq < ng; ++gq) {
    const int t0 = gq * ACC2_G, t1 = std::min<int>((gq + 1) * ACC2_G, (int)T.size());
    int64_t head[ACC2_G], end[ACC2_G];
    for (int x = t0; x < t1; ++x) { end[x - t0] = S.op_mid[T[x]]; head[x - t0] = end[x - t0] - ext_ops(S, st, T[x]); }
    while (true) {
      int sb = INT32_MAX;
      for (int x = 0; x < t1 - t0; ++x) if (head[x] < end[x]) sb = std::min(sb, S.op_b[head[x]]);
      if (sb == INT32_MAX) break;
      int a[ACC2_G];
      for (int x = 0; x < ACC2_G; ++x) a[x] = -1;
      for (int x = 0; x < t1 - t0; ++x) if (head[x] < end[x] && S.op_b[head[x]] == sb) { a[x] = S.op_a[head[x]]; ++head[x]; }
      o.b.push_back(sb);
      o.a.insert(o.a.end(), a, a + ACC2_G);
    }
    o.ptr.push_back((int64_t)o.b.size());
  }
}

// ---- column-group accumulate lists.  For a column k: T = its blocks with external updates (in block order), cut into
// groups of ACC2_G; the external sources of k are the entries (b = block (k, j), j) of its row list whose column j lies
// in another task (and, distributed, in the top when k is a top column: the domains' part arrives by collective).
// For every (group, j) with at least one target row in pattern(j) one entry is emitted.
void column_group_lists(Symbolic &S, const BuildState &st) {
  const int nlevels = n_levels(S);
  static const bool use_acc2 = tune("acc_v1", 0) == 0;
  S.g2_lvl.assign(nlevels + 1, 0);
  S.g2_ptr.assign(1, 0);
  if (!use_acc2) return;
  // pass 1 (parallel over chunks of 64 columns of a level): groups and entries into chunk-local buffers; pass 2 after
  // ALL levels: one allocation, offsets by a (cheap, serial) prefix pass, the copies in parallel
  // Only the very wide levels take this form: there it saves a third of the instructions and half of the vector
  // loads per update (cfg 5: factor sweep 26.6 -> 23.7 ms).  Narrower levels are latency-bound on the number of
  // dependent steps per wave, and the union of the source columns over ten targets is longer than one target's
  // own list (measured on cfg 2: k_chol_acc2<8> 28 us vs 15 us for the gather form at the top, 45 vs 32-55 us in
  // the middle), so they keep the gather lists.
  static const int64_t g2_min = (int64_t)tune("acc2_min", 8000);
  constexpr int CH = 64;
  std::vector<std::vector<ChunkOut>> all((size_t)nlevels);
  for (int l = 0; l < nlevels; ++l) {
    if (S.acc_ptr[l + 1] - S.acc_ptr[l] < (int64_t)ACC2_G * g2_min) continue;
    const int c0 = S.task_ptr[S.level_ptr[l]], c1 = S.task_ptr[S.level_ptr[l + 1]];
    std::vector<ChunkOut> &outs = all[(size_t)l];
    outs.resize((size_t)((c1 - c0 + CH - 1) / CH));
    parallel_ranges(c1 - c0, CH, [&](int qb, int qe) {
      std::vector<int> T;
      ChunkOut &o = outs[(size_t)(qb / CH)];
      for (int q = qb; q < qe; ++q) column_groups(S, st, S.task_cols[c0 + q], T, o);
    });
  }
  // pass 2
  std::vector<std::pair<int, int>> chunks;                       // (level, chunk)
  std::vector<int64_t> g0(1, 0), e0(1, 0);
  for (int l = 0; l < nlevels; ++l) {
    for (size_t q = 0; q < all[(size_t)l].size(); ++q) {
      chunks.push_back({l, (int)q});
      g0.push_back(g0.back() + (int64_t)all[(size_t)l][q].ptr.size());
      e0.push_back(e0.back() + (int64_t)all[(size_t)l][q].b.size());
    }
    S.g2_lvl[l + 1] = g0.back();
  }
  S.g2_tgt.resize((size_t)g0.back() * ACC2_G);
  S.g2_ptr.resize((size_t)g0.back() + 1);
  S.g2_b.resize((size_t)e0.back());
  S.g2_a.resize((size_t)e0.back() * ACC2_G);
  parallel_ranges((int)chunks.size(), 4, [&](int xb, int xe) {
    for (int x = xb; x < xe; ++x) {
      const ChunkOut &o = all[(size_t)chunks[x].first][(size_t)chunks[x].second];
      if (o.tgt.empty()) continue;
      std::copy(o.tgt.begin(), o.tgt.end(), S.g2_tgt.begin() + g0[x] * ACC2_G);
      std::copy(o.b.begin(), o.b.end(), S.g2_b.begin() + e0[x]);
      std::copy(o.a.begin(), o.a.end(), S.g2_a.begin() + e0[x] * ACC2_G);
      for (size_t y = 0; y < o.ptr.size(); ++y) S.g2_ptr[(size_t)g0[x] + 1 + y] = e0[x] + o.ptr[y];
    }
  });
}

}  // namespace symbolic
}  // namespace fgo
