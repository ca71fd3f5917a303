// Structure phase, host tables: L -> H map, panel sources, factor ownership (distributed), H slots, incidence lists, edge records,
// distributed offsets.
#include "structure_build.hpp"

namespace fgo {

int host_tables(fgo_ctx *c, const VarIndex &V, const PairGraph &G, const Ordering &O, HostTables &T,
                std::vector<unsigned char> &lm_mine, BuildTimer &tm) {
  const Symbolic &S = c->S;
  const int64_t N = V.N, E = V.E, NI = V.NI, NX = V.NX;
  const int nb = O.nb;
  // pose -> elimination position
  T.pose_col = std::vector<int>((size_t)NX, -1);
  for (int64_t v = 0; v < NX; ++v) if (V.hidx[v] >= 0) T.pose_col[v] = S.iperm[V.hidx[v]];
  for (int64_t v = 0; v < N; ++v) if (V.lm_index[v] >= 0) T.pose_col[v] = nb + V.lm_index[v];      // eliminated landmarks: virtual columns (b / x only)
  // L block -> H block: column k's original entries are the graph neighbours of perm[k]; stamp them in a scratch row
  // (per host thread) and read the column's pattern against it
  T.asrc = std::vector<int>((size_t)S.nnzL, -1);
  {
    // one chunk per host thread: the scratch rows are allocated once per chunk
    parallel_ranges(nb, std::max(2048, (nb + host_threads() - 1) / host_threads()), [&](int kb, int ke) {
      std::vector<int> stamp((size_t)nb, -1), pair_of((size_t)nb, -1);
      for (int k = kb; k < ke; ++k) {
        const int ha = S.perm[k];
        for (int p = G.g.xadj[ha]; p < G.g.xadj[ha + 1]; ++p) { const int col = S.iperm[G.g.adj[p]]; stamp[col] = k; pair_of[col] = G.adj_pair[p]; }
        T.asrc[S.colptr[k]] = k;
        for (int64_t t = S.colptr[k] + 1; t < S.colptr[k + 1]; ++t) {
          const int i = S.rowidx[t];
          T.asrc[t] = stamp[i] == k ? nb + pair_of[i] : -1;
        }
      }
    });
  }
  tm.lap("asrc");
  // panel blocks: where a block's value sits when the panel kernels pick it up -- in L (>= 0: block id; the wide
  // accumulate kernel already applied its external updates), still in H (-2 - H block), or nowhere (-1: fill-in
  // without updates).  Structural, so resolved here instead of by three dependent loads per block on the device.
  auto block_src = [&](int t) -> int {
    if (t < 0) return -1;
    if (t >= O.top_blk0) return t;                  // distributed: a top block's value arrives in L through the collective
    if (S.op_mid[t] > S.op_ptr[t]) return t;
    return T.asrc[t] >= 0 ? -2 - T.asrc[t] : -1;
  };
  T.ptri_src = std::vector<int>(S.ptri_blk.size()); T.prow_src = std::vector<int>(S.prow_blk.size());
  parallel_ranges((int)std::min<size_t>(S.ptri_blk.size(), INT32_MAX), 1 << 16, [&](int q0, int q1) { for (int q = q0; q < q1; ++q) T.ptri_src[q] = block_src(S.ptri_blk[q]); });
  parallel_ranges((int)std::min<size_t>(S.prow_blk.size(), INT32_MAX), 1 << 16, [&](int q0, int q1) { for (int q = q0; q < q1; ++q) T.prow_src[q] = block_src(S.prow_blk[q]); });
  tm.lap("panel sources");
  // multi-GPU: which factors this context linearises (everything when world == 1).  A variable belongs to the rank whose
  // domain holds its column (group `world` = top, -1 = fixed); a factor to the rank of any of its domain variables (they
  // all lie in one domain: a factor is a clique of the block graph and domains are separated by the top), factors among
  // top / fixed variables only are dealt round-robin.  So a domain variable sees ALL its factors locally (complete
  // diagonal block), a top variable a partial sum -- completed by the collective on the tail of L.
  c->pose_group.assign((size_t)NX, -1);
  if (O.dist)
    for (int64_t v = 0; v < N; ++v)
      if (T.pose_col[v] >= 0) c->pose_group[v] = (int)(std::upper_bound(S.dom_col0.begin(), S.dom_col0.begin() + O.world + 1, T.pose_col[v]) - S.dom_col0.begin()) - 1;
  auto factor_owner = [&](const int *vars, int nv, int64_t salt) -> int {
    if (!O.dist) return 0;
    int own = -1;
    for (int q = 0; q < nv; ++q) { const int gq = c->pose_group[vars[q]]; if (gq >= 0 && gq < O.world) { if (own >= 0 && own != gq) return -2; own = gq; } }
    return own >= 0 ? own : (int)(salt % O.world);
  };
  lm_mine.clear();
  if (O.dist && V.n_lm > 0) { const int rc = ba_landmark_owners(c, V, O, lm_mine); if (rc) return rc; }
  std::vector<unsigned char> edge_mine((size_t)E, 1), imu_mine((size_t)NI, 1);
  if (O.dist) {
    for (int64_t e = 0; e < E; ++e) {
      const int vars[2] = {c->ei[e], c->ej[e]};
      const int o = factor_owner(vars, 2, e);
      if (o == -2) return fail(c, FGO_EINVAL, "internal: a factor spans two domains");
      edge_mine[e] = o == O.rank;
    }
    for (int64_t f = 0; f < NI; ++f) {
      const int o = factor_owner(&c->imu_ids[6 * f], 6, f);
      if (o == -2) return fail(c, FGO_EINVAL, "internal: an IMU factor spans two domains");
      imu_mine[f] = o == O.rank;
    }
  }
  // this rank's IMU factors, sorted by colour
  c->imu_var_mask.assign((size_t)NX, 0); c->imu_flist.clear(); c->imu_fcolor.clear(); c->imu_extra = 0;
  for (int64_t f = 0; f < NI; ++f) if (imu_mine[f]) imu_colour_add(c, f);
  imu_colour_lists(c, T.imu_list);
  // edge -> slot; duplicate groups
  T.edge_slot = std::vector<int>((size_t)E, -1);
  T.dup_ptr = std::vector<int64_t>{0};
  T.imu_slot = std::vector<int>((size_t)15 * NI, -1);
  {
    // per pair: the slot of its single binary factor / of its IMU entries (in parallel); pairs that carry several binary
    // factors (rare) are collected per chunk and get their duplicate groups in pair order afterwards
    constexpr int64_t CH = 1 << 15;
    const int nch = (int)((G.noff + CH - 1) / CH);
    std::vector<std::vector<int64_t>> multi((size_t)nch);
    parallel_ranges(nch, 1, [&](int c0, int c1) {
      for (int ch = c0; ch < c1; ++ch)
        for (int64_t h = ch * CH, h1 = std::min(G.noff, h + CH); h < h1; ++h) {
          const int64_t m0 = G.ufirst[h], m1 = G.ufirst[h + 1];
          int64_t nbin = 0;
          for (int64_t m = m0; m < m1; ++m) nbin += G.pr[m].e >= 0;
          if (nbin > 1) multi[(size_t)ch].push_back(h);
          for (int64_t m = m0; m < m1; ++m) {
            const int64_t e = G.pr[m].e;
            if (e == STRUCT_ONLY) continue;
            if (e < 0) {                                  // IMU pair (u < w): stored transposed when w is eliminated later
              const int64_t idx = -1 - e, f = idx / 15;
              const unsigned char *uw = IMU_PAIR[idx % 15];
              T.imu_slot[idx] = h_slot(nb, h, T.pose_col[c->imu_ids[6 * f + uw[0]]], T.pose_col[c->imu_ids[6 * f + uw[1]]]);
              continue;
            }
            if (nbin == 1) T.edge_slot[e] = h_slot(nb, h, T.pose_col[c->ei[e]], T.pose_col[c->ej[e]]);
          }
        }
    });
    for (int ch = 0; ch < nch; ++ch)
      for (const int64_t h : multi[(size_t)ch]) {
        for (int64_t m = G.ufirst[h]; m < G.ufirst[h + 1]; ++m) {
          const int64_t e = G.pr[m].e;
          if (e < 0) continue;                            // (STRUCT_ONLY is negative too)
          if (edge_mine[e]) { T.dup_edges.push_back(e); T.dup_slot.push_back(h_slot(nb, h, T.pose_col[c->ei[e]], T.pose_col[c->ej[e]])); }   // owned members only
        }
        if ((int64_t)T.dup_edges.size() > T.dup_ptr.back()) T.dup_ptr.push_back((int64_t)T.dup_edges.size());
      }
  }
  tm.lap("edge slots");
  // per-variable incidence of the IMU factors
  T.imu_inc_ptr.assign((size_t)NX + 1, 0);
  T.imu_inc.resize((size_t)6 * T.imu_list.size());
  {
    for (int f : T.imu_list) for (int u = 0; u < 6; ++u) T.imu_inc_ptr[c->imu_ids[6 * (int64_t)f + u] + 1]++;
    for (int64_t v = 0; v < NX; ++v) T.imu_inc_ptr[v + 1] += T.imu_inc_ptr[v];
    std::vector<int64_t> fill(T.imu_inc_ptr.begin(), T.imu_inc_ptr.end() - 1);
    for (int f : T.imu_list)
      for (int u = 0; u < 6; ++u) T.imu_inc[fill[c->imu_ids[6 * (int64_t)f + u]]++] = (int)(((int64_t)f << 3) | u);
  }
  // half-edge lists (owned edges only)
  T.he_ptr = std::vector<int64_t>((size_t)NX + 1, 0);
  int64_t n_mine = 0;
  // (both sides of an eliminated observation are linearised by kernels_ba.hip: k_ba_linearize / k_ba_cameras)
  // (counts and places by atomic increments on all host threads; a variable's list is then sorted: ascending edge, which is the
  //  order the serial fill produced and the order its contributions are summed in)
  const int En = (int)std::min<int64_t>(E, INT32_MAX);
  parallel_ranges(En, 1 << 16, [&](int e0, int e1) {
    int64_t mine = 0;
    for (int64_t e = e0; e < e1; ++e)
      if (edge_mine[e]) {
        if (V.lm_index[c->ej[e]] < 0) { __atomic_fetch_add(&T.he_ptr[(size_t)c->ei[e] + 1], (int64_t)1, __ATOMIC_RELAXED); __atomic_fetch_add(&T.he_ptr[(size_t)c->ej[e] + 1], (int64_t)1, __ATOMIC_RELAXED); }
        ++mine;
      }
    __atomic_fetch_add(&n_mine, mine, __ATOMIC_RELAXED);
  });
  for (int64_t v = 0; v < NX; ++v) T.he_ptr[v + 1] += T.he_ptr[v];
  T.he = std::vector<int>((size_t)2 * n_mine);
  {
    std::vector<int64_t> fill(T.he_ptr.begin(), T.he_ptr.end() - 1);
    parallel_ranges(En, 1 << 16, [&](int e0, int e1) {
      for (int64_t e = e0; e < e1; ++e) {
        if (!edge_mine[e]) continue;
        if (V.lm_index[c->ej[e]] >= 0) continue;
        T.he[(size_t)__atomic_fetch_add(&fill[(size_t)c->ei[e]], (int64_t)1, __ATOMIC_RELAXED)] = (int)(e << 1);
        T.he[(size_t)__atomic_fetch_add(&fill[(size_t)c->ej[e]], (int64_t)1, __ATOMIC_RELAXED)] = (int)((e << 1) | 1);
      }
    });
    parallel_ranges((int)std::min<int64_t>(NX, INT32_MAX), 4096, [&](int v0, int v1) {
      for (int v = v0; v < v1; ++v) if (T.he_ptr[v + 1] - T.he_ptr[v] > 1) std::sort(T.he.begin() + T.he_ptr[v], T.he.begin() + T.he_ptr[v + 1]);
    });
  }
  // unary terms (priors, the padding identity of 3-dof variables): the variable's rank; top / fixed variables: rank 0
  T.var_mine = std::vector<unsigned char>((size_t)NX, 1);
  if (O.dist) for (int64_t v = 0; v < N; ++v) T.var_mine[v] = (c->pose_group[v] >= 0 && c->pose_group[v] < O.world) ? c->pose_group[v] == O.rank : O.rank == 0;
  // distributed: per top block / top column, where the updates sourced from this rank's domain and from the top start
  if (O.dist) {
    const int64_t ntb = S.nnzL - O.top_blk0;
    const int ntc = nb - O.top_col0;
    const int lo = S.dom_col0[O.rank], hi = S.dom_col0[O.rank + 1];
    T.top_ext0.resize((size_t)ntb); T.own_op0.resize((size_t)ntb); T.own_op1.resize((size_t)ntb);
    T.top_row0.resize((size_t)ntc); T.own_row0.resize((size_t)ntc); T.own_row1.resize((size_t)ntc);
    parallel_ranges((int)std::min<int64_t>(ntb, INT32_MAX), 4096, [&](int qb, int qe) {
      for (int64_t q = qb; q < qe; ++q) {
        const int64_t t = O.top_blk0 + q;
        const int *a0 = S.op_a.data() + S.op_ptr[t], *a1 = S.op_a.data() + S.op_mid[t];     // external ops, ascending source column
        auto first_col_ge = [&](int col) { return (int64_t)(std::partition_point(a0, a1, [&](int blk) { return S.blkcol[blk] < col; }) - S.op_a.data()); };
        T.own_op0[q] = first_col_ge(lo); T.own_op1[q] = first_col_ge(hi); T.top_ext0[q] = first_col_ge(O.top_col0);
      }
    });
    for (int q = 0; q < ntc; ++q) {
      const int k = O.top_col0 + q;
      const int *r0 = S.row_col.data() + S.rowptr[k], *r1 = S.row_col.data() + S.row_mid[k];   // entries outside the column's own panel, ascending
      auto first_ge = [&](int col) { return (int64_t)(std::lower_bound(r0, r1, col) - S.row_col.data()); };
      T.own_row0[q] = first_ge(lo); T.own_row1[q] = first_ge(hi); T.top_row0[q] = first_ge(O.top_col0);
    }
  }
  tm.lap("half-edge lists");
  // edge payload: one 256-byte record per edge (device_plan.hpp EDGE_REC)
  // (incremental mode: room for factors that arrive later)
  T.E_cap = V.R > 0 ? E + std::max<int64_t>(4096, E / 8) : E;
  T.NI_cap = V.R > 0 ? NI + std::max<int64_t>(256, NI / 8) : NI;
  T.erec = std::vector<double, NoInitAlloc<double>>((size_t)EDGE_REC * T.E_cap);   // first touched by the threads that fill it
  parallel_ranges((int)std::min<int64_t>(E, INT32_MAX), 8192, [&](int eb, int ee) {
    for (int64_t e = eb; e < ee; ++e) {
      double *o = &T.erec[(size_t)EDGE_REC * e];
      edge_payload(c, e, o, o + 8);
      o[7] = o[29] = o[30] = o[31] = 0.0;
    }
  });
  tm.lap("edge records");
  return FGO_OK;
}

}  // namespace fgo
