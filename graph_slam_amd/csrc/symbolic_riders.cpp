// Symbolic phase, part 5: the rider schedule with its hub pieces (symbolic_build.hpp; symbolic.cpp is the driver).
//
// ---- riders.  On the narrow top levels the triangle kernel is a pivot chain (~26 us) on a handful of CUs while the rest of
// the chip idles, and the accumulate launches of those levels keep the whole chip gathering for 10-60 us each.  Only the
// updates whose sources lie in the level directly below a target have to wait for it (10-30 % of a top target's list); the
// others are applied EARLY by spare workgroups ("riders") of the k_panel_tri launch of an earlier level l: a target of
// level lt > l takes its updates with source level <= l - 1 there.  Per target the external list is re-ordered by source
// level (stable: ascending column within a level) so that what a slot applies is a contiguous range; partial values live
// in L (nobody else touches a block of a later level) and the target's own accumulate launch continues from
// acc_start.  Slots are filled earliest-deadline-first (the next level's targets first) against a capacity model
// (a 16-wave rider workgroup = four items, cost t0 + tb * batches of 80 updates; budget = free CUs x window).
// The summation order of a target differs from the unsplit list, so L is not bit-identical to FGO_RIDE=0 -- it is
// deterministic, and partial re-factorisations (task_dirty) repeat exactly the same segments.
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "symbolic_build.hpp"

namespace fgo {
namespace symbolic {
namespace {

// Which levels give slots and which take riders.
// Distributed mode: levels are (dependency level, group) segments and only the TOP (group == world, replicated on every
// rank) takes riders -- its blocks' lists are [domain-sourced (arrive by collective) | top-sourced], ext_ops() is the
// top-sourced tail, and their value so far always sits in L.  `dl` = dependency level of a segment.
struct RideScope {
  const Symbolic &S;
  int nlevels, world, G, n_cu;
  std::vector<char> slot;            // per level: its triangle launch can carry riders
  int first_slot;                    // the first such level (nlevels: none)
  std::vector<int> col_level;        // per column: its dependency level
  int dl(int l) const { return l / G; }
  bool in_scope(int l) const { return world == 1 || S.seg_group[l] == world; }
  bool is_cand(int lt) const { return lt > first_slot && in_scope(lt) && S.g2_lvl[lt + 1] == S.g2_lvl[lt] && S.acc_ptr[lt + 1] > S.acc_ptr[lt]; }
  int lvl_of(int blk) const { return col_level[S.blkcol[blk]]; }
};

// What step 2 hands to the hub pieces and to step 3, per accumulate target (parallel to S.acc_targets)
struct Ridden {
  std::vector<int> cur;                                // updates of a target already given to riders
  std::vector<std::pair<int64_t, int>> hub_piece;      // (target position, scratch block) per piece of a hub target, in schedule order
  std::vector<int> hub_skip;                           // hub targets: entries at the end of the ridden part that the own launch does NOT skip (the piece updates)
};

// 1. external lists of the candidate targets by source level (counting sort, stable: ascending column within a level)
// -> early: updates of a target that can ride at all: source level <= its level - 2
std::vector<int> lists_by_source_level(Symbolic &S, const BuildState &st, const RideScope &sc) {
  const int nlevels = sc.nlevels;
  std::vector<int> early(S.acc_targets.size(), 0);
  for (int lt = sc.first_slot + 1; lt < nlevels; ++lt) {
    if (!sc.is_cand(lt)) continue;
    const int64_t q0 = S.acc_ptr[lt];
    parallel_ranges((int)(S.acc_ptr[lt + 1] - q0), 64, [&](int xb, int xe) {
      std::vector<int> lv, ta, tb2, cnt((size_t)nlevels + 1);
      for (int x = xb; x < xe; ++x) {
        const int b = S.acc_targets[q0 + x];
        const int64_t o1 = S.op_mid[b], o0 = o1 - ext_ops(S, st, b);
        const int n = (int)(o1 - o0);
        lv.resize((size_t)n);
        bool sorted = true;
        int ne = 0;
        for (int i = 0; i < n; ++i) { lv[i] = sc.lvl_of(S.op_a[o0 + i]); if (i > 0 && lv[i] < lv[i - 1]) sorted = false; ne += lv[i] <= sc.dl(lt) - 2; }
        early[q0 + x] = ne;
        if (sorted) continue;
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int i = 0; i < n; ++i) cnt[(size_t)lv[i] + 1]++;
        for (int l = 0; l < nlevels; ++l) cnt[(size_t)l + 1] += cnt[l];
        ta.resize((size_t)n); tb2.resize((size_t)n);
        for (int i = 0; i < n; ++i) { const int w = cnt[lv[i]]++; ta[w] = S.op_a[o0 + i]; tb2[w] = S.op_b[o0 + i]; }
        std::copy(ta.begin(), ta.end(), S.op_a.begin() + o0);
        std::copy(tb2.begin(), tb2.end(), S.op_b.begin() + o0);
      }
    });
  }
  return early;
}

// The rider workgroups of a launch take XCD-contiguous ranges of the items (kernels_factor.hip xcd_contiguous: workgroup b runs
// on XCD b & 7 and takes range element (b & 7) * q + ... ): the items stay in target order ACROSS the eight ranges --
// neighbouring targets share their source blocks, which then hit in that XCD's L2 (sweep traffic 5.41 -> 4.67 GB) --
// and are sorted heavy-first INSIDE a range, so that the long items of an XCD are dispatched first and equal
// neighbours share a workgroup.
void sort_items_inside_xcd_ranges(Symbolic &S, size_t first_item, int sub) {
  const int n_it = (int)(S.ride_items.size() - first_item);
  const int per = sub == 0 ? RIDE_PER_WG : 1;                        // items per rider workgroup (k_panel_tri launch / k_panel_rows launch)
  const int nwg = (n_it + per - 1) / per, q8 = nwg >> 3, r8 = nwg & 7;
  for (int x = 0; x < 8; ++x) {
    const int w0 = x * q8 + std::min(x, r8), w1 = w0 + q8 + (x < r8 ? 1 : 0);
    const int i0 = std::min(n_it, w0 * per), i1 = std::min(n_it, w1 * per);
    std::stable_sort(S.ride_items.begin() + first_item + i0, S.ride_items.begin() + first_item + i1, [](const RideItem &u, const RideItem &v) { return u.n > v.n; });
  }
}

// 2. earliest deadline first over the slots.  A level gives two: its triangle launch (16-wave workgroups, four items each)
// and its row launch (one-wave workgroups, one item each: small items only, the launch is ~11 us long)
// -> S.ride_items, ride_ptr, n_scratch; R.cur, R.hub_piece
void schedule_riders(Symbolic &S, const BuildState &st, const RideScope &sc, const std::vector<int> &early, Ridden &R) {
  static const double t0 = tune("ride_t0", 3.0);     // us per item (index + row round trips, combine)
  static const double tb = tune("ride_tb", 1.2);     // us per batch of 80 updates
  static const double win = tune("ride_win", 22.0);  // us of a triangle launch that riders may fill
  static const int64_t cap_ops = (int64_t)tune("ride_ops", 230000);   // and at most this many updates (gather throughput; round 4, 27-level schedule of cfg 2: 100 / 150 / 200 / 250 / 330 / 450 k -> sweep 3.009 / 2.966 / 2.946 / 2.941 / 3.003 / 3.015 ms)
  static const int ride_min = (int)tune("ride_min", 40);    // smallest item worth a half workgroup (a target's last chance: the slot below its level)
  static const int ride_max = (int)tune("ride_max", 480);     // largest item (the rest waits for a later slot or the level's own launch)
  static const int ride_hub = (int)tune("ride_hub", 4096);    // early updates from which a target is a hub (pieces into scratch blocks)
  static const int hub_force = (int)tune("ride_hub_force", 1); // hub targets ride in full in the slot below their level
  static const int ride_min2 = (int)tune("ride_min2", 120);   // ... in earlier slots: wait until more has gathered
  static const double win2 = tune("ride_win2", 0.0);   // 0: off -- measured neutral (cfg 2: factor sweep 3.303 with, 3.309 ms without)
  static const double tb2 = tune("ride_tb2", 1.0);     // us per batch of 20 updates
  static const int64_t cap_ops2 = (int64_t)tune("ride_ops2", 90000);
  static const int max2 = (int)tune("ride_max2", 100);       // largest item of a row launch
  const int nlevels = sc.nlevels, world = sc.world, n_cu = sc.n_cu;
  std::vector<int> &cur = R.cur;
  // (the targets of a level that can ride at all, in target order: most lists are too short, and `cur` only grows)
  std::vector<std::vector<int64_t>> rideable((size_t)nlevels);
  for (int lt = sc.first_slot + 1; lt < nlevels; ++lt)
    if (sc.is_cand(lt))
      for (int64_t q = S.acc_ptr[lt]; q < S.acc_ptr[lt + 1]; ++q)
        if (early[q] >= ride_min) rideable[(size_t)lt].push_back(q);
  for (int l = 0; l < nlevels; ++l) {
    for (int sub = 0; sub < 2; ++sub) {
      S.ride_ptr[2 * l + sub + 1] = (int)S.ride_items.size();
      if (l < sc.first_slot || l + 1 >= nlevels || !sc.slot[l]) continue;
      const int nt = S.level_ptr[l + 1] - S.level_ptr[l];
      const int busy = sub == 0 ? nt : (S.rchunk_ptr[l + 1] - S.rchunk_ptr[l] + 15) / 16;
      if (sub == 1 && (win2 <= 0 || S.rchunk_ptr[l + 1] == S.rchunk_ptr[l])) continue;
      double budget = (double)(n_cu - busy) * (sub == 0 ? win : win2);
      int64_t ops_left = (sub == 0 ? cap_ops : cap_ops2) * (n_cu - busy) / n_cu;
      const size_t first_item = S.ride_items.size();
      for (int lt = l + 1; lt < nlevels; ++lt) {
        if (!sc.is_cand(lt)) continue;
        // (the slot directly below a level is the last chance of that level's hub targets: they ride whatever the slot holds already)
        const bool last_chance = hub_force && sub == 0 && world == 1 && sc.dl(lt) == sc.dl(l) + 1;
        if (!(budget > 0 && ops_left > 0) && !last_chance) break;
        for (const int64_t q : rideable[(size_t)lt]) {
          const bool room = budget > 0 && ops_left > 0;
          if (!room && !last_chance) break;
          if (!room && early[q] < ride_hub) continue;
          if (early[q] - cur[q] < ride_min) continue;
          const int b = S.acc_targets[q];
          const int64_t o1 = S.op_mid[b], o0 = o1 - ext_ops(S, st, b);
          // updates with source level <= l - 1: a prefix of the (level-sorted) list
          int64_t lo = o0 + cur[q], hi = o0 + early[q];
          while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (sc.lvl_of(S.op_a[mid]) <= sc.dl(l) - 1) lo = mid + 1; else hi = mid; }
          int64_t avail = lo - (o0 + cur[q]);
          const int nmin = sc.dl(lt) == sc.dl(l) + 1 ? ride_min : ride_min2;
          // A HUB target (a plane or place seen from thousands of keyframes: tens of thousands of early updates) would
          // leave most of its list to ONE workgroup of its level's own launch (cfg 4: 54 374 updates, 625 us).  Its early
          // updates are cut into pieces that several rider workgroups of the same slot sum into SCRATCH blocks behind L;
          // the target's own list then holds one update per piece, (scratch block) x (identity block)^T.
          if (sub == 1 && early[q] >= ride_hub) continue;            // (hubs ride in the triangle launches only)
          const bool hub = sub == 0 && world == 1 && early[q] >= ride_hub;
          if (avail < nmin) continue;
          // What a hub target does not get rid of here, ONE workgroup of its level's own launch walks through at ~1.5 us per
          // 80 updates while the chip idles (100 k poses with a dozen places revisited 1 000 times: 510 k updates left to 28
          // workgroups, 359 us); as pieces they cost the triangle launch ~1 us per 15 k.
          const bool force = hub && last_chance;
          if (!room && !force) continue;
          while (avail > 0 && (force || (budget > 0 && ops_left > 0))) {
            int64_t n = force ? avail : std::min(avail, ops_left);
            n = std::min<int64_t>(n, sub == 1 ? max2 : ride_max);   // (an item is one quarter workgroup's serial work)
            if (n < std::min(nmin, max2)) break;
            if (hub) {
              S.ride_items.push_back(RideItem{(int)(S.nnzL + 2 + S.n_scratch), st.task_of[S.blkcol[b]], (long long)(o0 + cur[q]), (int)n, 2});
              R.hub_piece.push_back({q, S.n_scratch});
              ++S.n_scratch;
            } else {
              S.ride_items.push_back(RideItem{b, st.task_of[S.blkcol[b]], (long long)(o0 + cur[q]), (int)n, (cur[q] == 0 && world == 1) ? 1 : 0});
            }
            cur[q] += (int)n;
            avail -= n;
            ops_left -= n;
            budget -= sub == 0 ? 0.25 * (t0 + tb * (double)((n + 79) / 80)) : (t0 + tb2 * (double)((n + 19) / 20)) / 16.0;
            if (!hub) break;                                         // an ordinary target: one item per slot (it writes its own block)
          }
        }
      }
      sort_items_inside_xcd_ranges(S, first_item, sub);
      S.ride_ptr[2 * l + sub + 1] = (int)S.ride_items.size();
    }
  }
}

// hub targets: the ridden part of the list moves to a copy behind the lists (the rider items read it there), and the
// last entries of its place become one update per piece: block (nnzL + 2 + scratch) times the identity block nnzL + 1
// -> S.op_a / op_b grown and rewritten, the o0 of the hub items; R.hub_skip
void place_hub_pieces(Symbolic &S, const BuildState &st, Ridden &R) {
  const std::vector<int> &cur = R.cur;
  std::vector<int> npiece(S.acc_targets.size(), 0);
  for (const auto &hp : R.hub_piece) npiece[(size_t)hp.first]++;
  std::vector<int64_t> copy_at(S.acc_targets.size(), -1);
  int64_t extra = 0;
  for (size_t q = 0; q < npiece.size(); ++q) if (npiece[q] > 0) { copy_at[q] = (int64_t)S.op_a.size() + extra; extra += cur[q]; }
  const size_t base = S.op_a.size();
  S.op_a.resize(base + (size_t)extra); S.op_b.resize(base + (size_t)extra);
  for (size_t q = 0; q < npiece.size(); ++q) {
    if (npiece[q] == 0) continue;
    const int b = S.acc_targets[q];
    const int64_t o0 = S.op_mid[b] - ext_ops(S, st, b);
    std::copy(S.op_a.begin() + o0, S.op_a.begin() + o0 + cur[q], S.op_a.begin() + copy_at[q]);
    std::copy(S.op_b.begin() + o0, S.op_b.begin() + o0 + cur[q], S.op_b.begin() + copy_at[q]);
  }
  // the items of hub targets: re-point their op ranges into the copies
  {
    std::vector<int64_t> q_of_scratch((size_t)S.n_scratch, -1);
    for (const auto &hp : R.hub_piece) q_of_scratch[(size_t)hp.second] = hp.first;
    for (RideItem &it : S.ride_items) {
      if (it.first != 2) continue;
      const int64_t q = q_of_scratch[(size_t)(it.t - (int)(S.nnzL + 2))];
      const int b = S.acc_targets[(size_t)q];
      const int64_t o0 = S.op_mid[b] - ext_ops(S, st, b);
      it.o0 = copy_at[(size_t)q] + (it.o0 - o0);
    }
  }
  // one (scratch, identity) update per piece at the end of the ridden part; `cur` shrinks to what the own launch skips
  std::vector<int> placed(S.acc_targets.size(), 0);
  for (const auto &hp : R.hub_piece) {
    const size_t q = (size_t)hp.first;
    const int b = S.acc_targets[q];
    const int64_t o0 = S.op_mid[b] - ext_ops(S, st, b);
    const int64_t at = o0 + cur[q] - npiece[q] + placed[q]++;
    S.op_a[at] = (int)(S.nnzL + 2 + hp.second);
    S.op_b[at] = (int)(S.nnzL + 1);
  }
  for (size_t q = 0; q < npiece.size(); ++q) if (npiece[q] > 0) R.hub_skip[q] = npiece[q];
}

void print_ride_stats(const Symbolic &S, const BuildState &st, const RideScope &sc, int64_t ridden, int64_t total) {
  const int nlevels = sc.nlevels;
  std::fprintf(stderr, "[ride] %zu items, %lld of %lld updates of the candidate levels ride\n", S.ride_items.size(), (long long)ridden, (long long)total);
  for (int l = 0; l < nlevels; ++l)
    if (S.ride_ptr[2 * l + 2] > S.ride_ptr[2 * l]) {
      int64_t ops[2] = {0, 0};
      for (int sub = 0; sub < 2; ++sub)
        for (int i = S.ride_ptr[2 * l + sub]; i < S.ride_ptr[2 * l + sub + 1]; ++i) ops[sub] += S.ride_items[i].n;
      std::fprintf(stderr, "[ride] slot %d: triangle launch %d items, %lld updates; row launch %d items, %lld updates\n", l, S.ride_ptr[2 * l + 1] - S.ride_ptr[2 * l],
                   (long long)ops[0], S.ride_ptr[2 * l + 2] - S.ride_ptr[2 * l + 1], (long long)ops[1]);
    }
  for (int lt = sc.first_slot + 1; lt < nlevels; ++lt) {
    int64_t tot = 0, left = 0;
    for (int64_t q = S.acc_ptr[lt]; q < S.acc_ptr[lt + 1]; ++q) {
      const int b = S.acc_targets[q];
      tot += ext_ops(S, st, b); left += S.acc_start[q] < 0 ? ext_ops(S, st, b) : S.op_mid[b] - acc_start_op(S.acc_start[q]);
    }
    std::fprintf(stderr, "[ride] level %d: %lld targets (%lld long), %lld updates, %lld left to its own launch\n", lt, (long long)(S.acc_ptr[lt + 1] - S.acc_ptr[lt]),
                 (long long)(S.acc_ptr[lt + 1] - S.acc_mid[lt]), (long long)tot, (long long)left);
  }
}

// 3. what is left to the levels' own accumulate launches; short / long split by the REMAINING list
// -> S.acc_start; acc_targets / acc_mid of the candidate levels
void split_own_launches(Symbolic &S, const BuildState &st, const RideScope &sc, const Ridden &R) {
  const int nlevels = sc.nlevels, world = sc.world;
  const std::vector<int> &cur = R.cur, &hub_skip = R.hub_skip;
  int64_t ridden = 0, total = 0;
  S.acc_start.assign(S.acc_targets.size(), -1);
  static const int64_t long_ops = (int64_t)tune("acc_long", ACC_LONG_OPS);
  for (int lt = sc.first_slot + 1; lt < nlevels; ++lt) {
    if (!sc.is_cand(lt)) continue;
    std::vector<std::pair<int, int64_t>> tg;           // (block, start or -1)
    for (int64_t q = S.acc_ptr[lt]; q < S.acc_ptr[lt + 1]; ++q) {
      const int b = S.acc_targets[q];
      total += ext_ops(S, st, b); ridden += cur[q];
      // (a hub target starts from H like a target without riders -- its pieces sit in scratch blocks --, unless it is a block
      //  of the distributed top, whose value is in L anyway: encoded as start | ACC_START_HUB)
      const int64_t start = S.op_mid[b] - ext_ops(S, st, b) + cur[q] - hub_skip[q];
      tg.push_back({b, cur[q] > 0 ? (hub_skip[q] > 0 && world == 1 ? (start | ACC_START_HUB) : start) : (int64_t)-1});
    }
    // (task order first -- the level's list arrives as [short | long] of the full lists, two runs --: partial sweeps launch the
    //  index range that covers their dirty tasks, structure_upload.cpp "tk_*")
    std::stable_sort(tg.begin(), tg.end(), [&](const std::pair<int, int64_t> &u, const std::pair<int, int64_t> &v) {
      return st.task_of[S.blkcol[u.first]] < st.task_of[S.blkcol[v.first]]; });
    auto first_long = std::stable_partition(tg.begin(), tg.end(), [&](const std::pair<int, int64_t> &u) {
      return (u.second < 0 ? ext_ops(S, st, u.first) : S.op_mid[u.first] - acc_start_op(u.second)) <= long_ops; });
    S.acc_mid[lt] = S.acc_ptr[lt] + (int64_t)(first_long - tg.begin());
    for (size_t x = 0; x < tg.size(); ++x) { S.acc_targets[S.acc_ptr[lt] + x] = tg[x].first; S.acc_start[S.acc_ptr[lt] + x] = tg[x].second; }
  }
  if (tune("ride_stats", 0) != 0) print_ride_stats(S, st, sc, ridden, total);
}

}  // namespace

void build_riders(Symbolic &S, const BuildState &st, Laps &lap) {
  const int nb = S.nb, nlevels = n_levels(S), world = S.world;
  S.ride_ptr.assign(2 * nlevels + 1, 0);
  static const int ride_on = (int)tune("ride", 1);
  RideScope sc{S, nlevels, world, world > 1 ? world + 1 : 1, (int)tune("ride_cus", S.cus), std::vector<char>(nlevels, 0), nlevels, {}};
  for (int l = 0; l < nlevels; ++l) {
    const int nt = S.level_ptr[l + 1] - S.level_ptr[l];
    sc.slot[l] = sc.in_scope(l) && S.level_panel[l] && nt > 0 && nt <= tri_wide_panels(S.cus) && nt < sc.n_cu;
    if (sc.slot[l] && sc.first_slot == nlevels) sc.first_slot = l;
  }
  if (!ride_on || std::getenv("FGO_NO_PANELS") || sc.first_slot + 1 >= nlevels) return;
  sc.col_level.resize((size_t)nb);
  for (int k = 0; k < nb; ++k) sc.col_level[k] = st.tlevel[st.task_of[k]] / sc.G;
  const std::vector<int> early = lists_by_source_level(S, st, sc);
  lap("riders: lists by source level");
  Ridden R{std::vector<int>(S.acc_targets.size(), 0), {}, std::vector<int>(S.acc_targets.size(), 0)};
  schedule_riders(S, st, sc, early, R);
  lap("riders: schedule");
  if (!R.hub_piece.empty()) place_hub_pieces(S, st, R);
  if (!S.ride_items.empty()) split_own_launches(S, st, sc, R);
}

}  // namespace symbolic
}  // namespace fgo
