// Structure phase, upload: device buffers (index lists, edge records, hubs, priors, IMU payloads, panel tables, descriptors, chain,
// partial-sweep tables, work buffers), the host schedule and DevPlan -- the pointers and counts every kernel launch receives.
#include "structure_build.hpp"

namespace fgo {
namespace {

// ---- factor side: index lists, edge records, hubs, duplicate groups, priors, IMU payloads, ownership
int upload_factor_side(fgo_ctx *c, const VarIndex &V, const Ordering &O, const HostTables &T, HubPlan &hubs, size_t &hub_cap) {
  hipStream_t s = c->stream;
  HIPCHK(c, c->d_pose_col.upload(T.pose_col, s));
  if (V.R > 0) {     // capacity first (upload() keeps an allocation that is large enough), so that later factors are appended in place
    HIPCHK(c, c->d_edge_i.alloc((size_t)T.E_cap)); HIPCHK(c, c->d_edge_j.alloc((size_t)T.E_cap)); HIPCHK(c, c->d_edge_slot.alloc((size_t)T.E_cap));
    HIPCHK(c, c->d_edge_kind.alloc((size_t)T.E_cap)); HIPCHK(c, c->d_he.alloc((size_t)2 * T.E_cap));
    HIPCHK(c, c->d_imu.alloc((size_t)T.NI_cap)); HIPCHK(c, c->d_imu_ids.alloc((size_t)6 * T.NI_cap)); HIPCHK(c, c->d_imu_slot.alloc((size_t)15 * T.NI_cap));
    HIPCHK(c, c->d_imu_list.alloc((size_t)T.NI_cap));
  }
  HIPCHK(c, c->d_edge_i.upload(c->ei, s));
  HIPCHK(c, c->d_edge_j.upload(c->ej, s));
  HIPCHK(c, c->d_edge_slot.upload(T.edge_slot, s));
  HIPCHK(c, c->d_he_ptr.upload(T.he_ptr, s));
  plan_hubs(T.he_ptr, V.NX, 0, hubs);
  hub_cap = hubs.var.size() + (V.R > 0 ? 256 : 0);                  // entries the scratch buffers have room for
  { const int rc = upload_hubs(c, hubs, hub_cap); if (rc) return rc; }
  HIPCHK(c, c->d_he.upload(T.he, s));
  HIPCHK(c, c->d_dup_ptr.upload(T.dup_ptr, s));
  HIPCHK(c, c->d_dup_edges.upload(T.dup_edges, s));
  HIPCHK(c, c->d_dup_slot.upload(T.dup_slot, s));
  c->n_dup_members = (int64_t)T.dup_edges.size();
  HIPCHK(c, c->d_ainv.upload(T.erec, s));
  { const int rc = upload_priors(c, V.NX, T.var_mine); if (rc) return rc; }
  HIPCHK(c, c->d_imu.upload(c->imu_payload, s));
  HIPCHK(c, c->d_imu_ids.upload(c->imu_ids, s));
  HIPCHK(c, c->d_imu_slot.upload(T.imu_slot, s));
  {
    std::vector<int> vk(c->var_kind);
    vk.resize((size_t)V.NX, 5);                          // phantoms: kind 5 = no degrees of freedom yet (identity block, x = 0)
    HIPCHK(c, c->d_var_kind.upload(vk, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  HIPCHK(c, c->d_edge_kind.upload(c->torder, s));
  HIPCHK(c, c->d_imu_list.upload(T.imu_list, s));
  HIPCHK(c, c->d_pose_group.upload(c->pose_group, s));
  HIPCHK(c, c->d_var_mine.upload(T.var_mine, s));
  HIPCHK(c, c->d_top_ext0.upload(T.top_ext0, s));
  HIPCHK(c, c->d_own_op0.upload(T.own_op0, s));
  HIPCHK(c, c->d_own_op1.upload(T.own_op1, s));
  HIPCHK(c, c->d_top_row0.upload(T.top_row0, s));
  HIPCHK(c, c->d_own_row0.upload(T.own_row0, s));
  HIPCHK(c, c->d_own_row1.upload(T.own_row1, s));
  if (O.dist) HIPCHK(c, c->d_gather.alloc(std::max<size_t>((size_t)V.N * 8, 64)));
  return FGO_OK;
}

// ---- host schedule (HostSchedule: levels, chunk pointers, per-level maxima) and the forward-solve work items
int host_schedule(fgo_ctx *c, const Ordering &O) {
  hipStream_t s = c->stream;
  const Symbolic &S = c->S;
  DevPlan &P = c->plan;
  c->sched.world = O.world; c->sched.rank = O.rank; c->sched.seg_group = S.seg_group;
  c->sched.n_top_blocks = S.nnzL - O.top_blk0; c->sched.n_top_cols = O.nb - O.top_col0;
  c->sched.ride_ptr = S.ride_items.empty() ? std::vector<int>() : S.ride_ptr;
  c->sched.g2_lvl = S.g2_lvl;
  if (S.g2_ptr.size() <= 1) c->sched.g2_lvl.clear();
  c->sched.level_panel = S.level_panel; c->sched.pchunk_ptr = S.pchunk_ptr; c->sched.fchunk_ptr = S.fchunk_ptr; c->sched.rchunk_ptr = S.rchunk_ptr;
  if (std::getenv("FGO_NO_PANELS")) std::fill(c->sched.level_panel.begin(), c->sched.level_panel.end(), 0);
  c->sched.level_leaf = S.level_leaf; c->sched.level_leaf_maxblk = S.level_leaf_maxblk; c->sched.level_leaf_maxops = S.level_leaf_maxops;
  if (tune("no_leaf", 0) != 0) std::fill(c->sched.level_leaf.begin(), c->sched.level_leaf.end(), 0);
  c->sched.n_levels = (int)S.level_ptr.size() - 1;
  c->sched.level_ptr = S.level_ptr;
  c->sched.acc_ptr = S.acc_ptr; c->sched.acc_mid = S.acc_mid;
  c->sched.level_pn0.assign(c->sched.n_levels, 0);
  for (int l = 0; l < c->sched.n_levels; ++l)
    if (S.level_panel[l]) {
      c->sched.level_pn0[l] = S.task_panel[S.level_ptr[l]];
      for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t)
        if (S.task_panel[t] != c->sched.level_pn0[l] + (t - S.level_ptr[l])) return fail(c, FGO_EINVAL, "internal: panel ids of a level are not consecutive");
    }
  c->sched.level_col_ptr.resize(c->sched.n_levels + 1);
  for (int l = 0; l <= c->sched.n_levels; ++l) c->sched.level_col_ptr[l] = S.task_ptr[S.level_ptr[l]];
  {
    // forward-solve work items: one per panel column, or one per chunk of FWD_CHUNK entries where the external part of the
    // column's row is longer than that (not in distributed mode: a top row's domain part arrives by collective)
    static const int fwd_split = (int)tune("fwd_split", 32);     // least number of chunks of FWD_CHUNK entries (0: never split); a level with split rows pays one more (tiny) launch
    std::vector<int> fwg_ci, fwg_ch, fsplit, f0v((size_t)O.nb, 0), fnv((size_t)O.nb, 1);
    c->sched.fwg_ptr.assign((size_t)c->sched.n_levels + 1, 0);
    c->sched.fsplit_ptr.assign((size_t)c->sched.n_levels + 1, 0);
    for (int l = 0; l < c->sched.n_levels; ++l) {
      if (S.level_panel[l])
        for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t) {
          const int pn = S.task_panel[t], m = S.task_ptr[t + 1] - S.task_ptr[t];
          for (int q = 0; q < m; ++q) {
            const int ci = S.task_ptr[t] + q;
            const int f0 = S.pcol_fchunk0[S.col_off(pn) + q], fn = S.pcol_fchunkn[S.col_off(pn) + q];
            if (fn <= 1 || O.dist || !fwd_split || fn < fwd_split) { fwg_ci.push_back(ci); fwg_ch.push_back(-1); continue; }
            f0v[(size_t)ci] = f0; fnv[(size_t)ci] = fn; fsplit.push_back(ci);
            for (int x = 0; x < fn; ++x) { fwg_ci.push_back(ci); fwg_ch.push_back(f0 + x); }
          }
        }
      c->sched.fwg_ptr[(size_t)l + 1] = (int)fwg_ci.size();
      c->sched.fsplit_ptr[(size_t)l + 1] = (int)fsplit.size();
    }
    HIPCHK(c, c->d_fwg_ci.upload(fwg_ci, s)); HIPCHK(c, c->d_fwg_ch.upload(fwg_ch, s));
    HIPCHK(c, c->d_fwd_f0.upload(f0v, s)); HIPCHK(c, c->d_fwd_fn.upload(fnv, s));
    HIPCHK(c, c->d_fsplit_ci.upload(fsplit, s));
    HIPCHK(c, hipStreamSynchronize(s));
    P.fwg_ci = c->d_fwg_ci.p; P.fwg_ch = c->d_fwg_ch.p; P.fwd_f0 = c->d_fwd_f0.p; P.fwd_fn = c->d_fwd_fn.p; P.fsplit_ci = c->d_fsplit_ci.p;
  }
  c->sched.level_maxcol.assign(c->sched.n_levels, 0);
  c->sched.level_maxrow.assign(c->sched.n_levels, 0);
  c->sched.level_maxtaskcols.assign(c->sched.n_levels, 0);
  for (int l = 0; l < c->sched.n_levels; ++l)
    for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t) {
      c->sched.level_maxtaskcols[l] = std::max(c->sched.level_maxtaskcols[l], S.task_ptr[t + 1] - S.task_ptr[t]);
      for (int q = S.task_ptr[t]; q < S.task_ptr[t + 1]; ++q) {
        const int k = S.task_cols[q];
        c->sched.level_maxcol[l] = std::max(c->sched.level_maxcol[l], (int)(S.colptr[k + 1] - S.colptr[k]));
        c->sched.level_maxrow[l] = std::max(c->sched.level_maxrow[l], (int)(S.rowptr[k + 1] - S.rowptr[k]));
      }
    }
  return FGO_OK;
}

// ---- the factor's pattern, update lists and accumulate descriptors
int upload_symbolic(fgo_ctx *c, const Ordering &O, const HostTables &T) {
  hipStream_t s = c->stream;
  Symbolic &S = c->S;
  HIPCHK(c, c->d_colptr.upload(S.colptr, s));
  HIPCHK(c, c->d_rowidx.upload(S.rowidx, s));
  HIPCHK(c, c->d_asrc.upload(T.asrc, s));
  HIPCHK(c, c->d_op_ptr.upload(S.op_ptr, s));
  HIPCHK(c, c->d_op_mid.upload(S.op_mid, s));
  HIPCHK(c, c->d_op_a.upload(S.op_a, s));
  HIPCHK(c, c->d_op_b.upload(S.op_b, s));
  HIPCHK(c, c->d_acc_targets.upload(S.acc_targets, s));
  for (auto &a : S.g2_a) if (a < 0) a = (int)S.nnzL;        // absent (row, source) pairs read the zero block
  HIPCHK(c, c->d_g2_tgt.upload(S.g2_tgt, s));
  HIPCHK(c, c->d_g2_ptr.upload(S.g2_ptr, s));
  HIPCHK(c, c->d_g2_b.upload(S.g2_b, s));
  HIPCHK(c, c->d_g2_a.upload(S.g2_a, s));
  HIPCHK(c, c->d_ride_items.upload(S.ride_items, s));
  HIPCHK(c, c->d_acc_start.upload(S.acc_start, s));
  {
    // one descriptor per accumulate target: the head of k_chol_acc read acc_targets / acc_start, THEN op_ptr / op_mid / asrc / top_ext0 of the
    // block -- two dependent round trips in a launch that is five of them on the narrow levels
    std::vector<AccDesc> ad(S.acc_targets.size());
    parallel_ranges((int)ad.size(), 1 << 14, [&](int q0, int q1) {
      for (int q = q0; q < q1; ++q) {
        const int t = S.acc_targets[(size_t)q];
        const int64_t rsv = S.acc_start.empty() ? -1 : S.acc_start[(size_t)q];
        const bool from_h = rsv >= 0 && (rsv & ACC_START_HUB) != 0;
        const int64_t rs = rsv >= 0 ? acc_start_op(rsv) : -1;
        const bool topb = O.dist && t >= O.top_blk0;
        ad[(size_t)q] = AccDesc{t, (topb || (rs >= 0 && !from_h)) ? -2 : (T.asrc[(size_t)t] >= 0 ? T.asrc[(size_t)t] : -1),
                                (long long)(rs >= 0 ? rs : (topb ? T.top_ext0[(size_t)(t - O.top_blk0)] : S.op_ptr[(size_t)t])), (long long)S.op_mid[(size_t)t]};
      }
    });
    HIPCHK(c, c->d_acc_desc.upload(ad, s));
  }
  return FGO_OK;
}

// ---- partial sweeps (incremental mode): task of every column / accumulate target / column group, item ranges per task
int partial_sweep_tables(fgo_ctx *c, const VarIndex &V, const Ordering &O, const std::vector<int> &task_level, BuildTimer &tm) {
  hipStream_t s = c->stream;
  const Symbolic &S = c->S;
  const int nb = O.nb;
  IsamState &I = c->isam;
  I.col_task.clear();
  if (c->isam_incremental && !O.dist) {               // partial sweeps: task of every column / accumulate target / column group
    const int ntask = (int)S.task_ptr.size() - 1;
    I.col_task.assign((size_t)nb, 0);
    std::vector<int> tcol_task((size_t)nb);
    for (int t = 0; t < ntask; ++t)
      for (int q = S.task_ptr[t]; q < S.task_ptr[t + 1]; ++q) { I.col_task[S.task_cols[q]] = t; tcol_task[(size_t)q] = t; }
    std::vector<int> acc_task(S.acc_targets.size()), g2_task(S.g2_ptr.size() - 1);
    for (size_t q = 0; q < acc_task.size(); ++q) acc_task[q] = I.col_task[S.blkcol[S.acc_targets[q]]];
    for (size_t q = 0; q < g2_task.size(); ++q) {
      int t = -1;
      for (int x = 0; x < ACC2_G && t < 0; ++x) if (S.g2_tgt[q * ACC2_G + x] >= 0) t = I.col_task[S.blkcol[S.g2_tgt[q * ACC2_G + x]]];
      g2_task[q] = t < 0 ? 0 : t;
    }
    // per task: where its items sit in the level-wise lists (partial sweeps launch the covering ranges only)
    {
      const int nl = (int)S.level_ptr.size() - 1;
      I.tk_s0.assign((size_t)ntask, 0); I.tk_s1 = I.tk_s0; I.tk_l0 = I.tk_s0; I.tk_l1 = I.tk_s0;
      I.tk_g0.assign((size_t)ntask, 0); I.tk_g1 = I.tk_g0; I.tk_c0 = I.tk_g0; I.tk_c1 = I.tk_g0;
      I.task_level = task_level;
      I.lvl_lo.assign((size_t)nl, 0); I.lvl_hi.assign((size_t)nl, -1);
      bool ok = true;
      // items [b, e) of a level, task(q) of an item (-1: belongs to whatever task is current) -> per task [first, end)
      auto scan = [&](const char *kind, int l, int64_t b, int64_t e, auto task_at, auto &first, auto &end) {
        const bool was_ok = ok;
        int64_t q = b;
        for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t) {
          first[(size_t)t] = (typename std::decay<decltype(first)>::type::value_type)q;
          while (q < e) { const int tq = task_at(q); if (tq != t && tq >= 0) break; ++q; }
          end[(size_t)t] = (typename std::decay<decltype(end)>::type::value_type)q;
        }
        if (q != e) ok = false;
        if (was_ok && !ok && tm.prof) std::fprintf(stderr, "[fgo build]    %s of level %d not in task order: item %lld of [%lld, %lld) has task %d, level tasks [%d, %d)\n", kind, l, (long long)q, (long long)b, (long long)e, task_at(q), S.level_ptr[l], S.level_ptr[l + 1]);
      };
      for (int l = 0; l < nl; ++l) {
        scan("short targets", l, S.acc_ptr[l], S.acc_mid[l], [&](int64_t q) { return acc_task[(size_t)q]; }, I.tk_s0, I.tk_s1);
        scan("long targets", l, S.acc_mid[l], S.acc_ptr[l + 1], [&](int64_t q) { return acc_task[(size_t)q]; }, I.tk_l0, I.tk_l1);
        if (!S.g2_lvl.empty())
          scan("column groups", l, S.g2_lvl[l], S.g2_lvl[l + 1], [&](int64_t q) {
            for (int x = 0; x < ACC2_G; ++x) if (S.g2_tgt[(size_t)q * ACC2_G + x] >= 0) return I.col_task[S.blkcol[S.g2_tgt[(size_t)q * ACC2_G + x]]];
            return -1; }, I.tk_g0, I.tk_g1);
        scan("row chunks", l, S.rchunk_ptr[l], S.rchunk_ptr[l + 1], [&](int64_t q) { return S.panel_task[S.rchunk_panel[(size_t)q]]; }, I.tk_c0, I.tk_c1);
      }
      I.tk_ok = ok && tune("isam_ranges", 1) != 0;
    }
    HIPCHK(c, I.d_acc_task.upload(acc_task, s));
    HIPCHK(c, I.d_g2_task.upload(g2_task, s));
    HIPCHK(c, I.d_tcol_task.upload(tcol_task, s));
    HIPCHK(c, I.d_task_dirty.alloc((size_t)ntask));
    HIPCHK(c, I.d_col_dirty.alloc((size_t)nb));
    HIPCHK(c, I.d_moved.alloc((size_t)V.NX));
    HIPCHK(c, I.d_moved_next.alloc((size_t)V.NX));
    HIPCHK(c, I.d_lin_mask.alloc((size_t)V.NX));
    HIPCHK(c, I.d_chi_var.alloc((size_t)V.NX));
    HIPCHK(c, I.wild.d_xprev.alloc((size_t)nb * 6));
    HIPCHK(c, I.wild.d_bwd_run.alloc((size_t)ntask));
    HIPCHK(c, I.wild.d_chg.alloc((size_t)nb));
    I.invalidate_carry();                           // (what the previous update left was laid out for the previous structure)
    I.last.clear();
    HIPCHK(c, I.d_y.alloc((size_t)nb * 6));
    const size_t need = isam_flags(nullptr, V.NX, ntask, nb).bytes;
    if (need > I.h_flags_cap) {
      if (I.h_flags) (void)hipHostFree(I.h_flags);
      I.h_flags = nullptr; I.h_flags_cap = 0; I.flags = IsamFlags{};
      HIPCHK(c, hipHostMalloc((void **)&I.h_flags, need + need / 4, hipHostMallocDefault));
      I.h_flags_cap = need + need / 4;
    }
    I.flags = isam_flags(I.h_flags, V.NX, ntask, nb);
    std::memset(I.h_flags, 0, need);                // fgo_isam2_update keeps the flag arrays clean between calls (sparse set / clear)
    HIPCHK(c, hipStreamSynchronize(s));             // the staging vectors die here
  }
  return FGO_OK;
}

// ---- panel lists
int upload_panel_lists(fgo_ctx *c, const HostTables &T) {
  hipStream_t s = c->stream;
  const Symbolic &S = c->S;
  HIPCHK(c, c->d_rowptr.upload(S.rowptr, s));
  HIPCHK(c, c->d_row_blk.upload(S.row_blk, s));
  HIPCHK(c, c->d_row_col.upload(S.row_col, s));
  HIPCHK(c, c->d_task_ptr.upload(S.task_ptr, s));
  HIPCHK(c, c->d_task_cols.upload(S.task_cols, s));
  HIPCHK(c, c->d_task_panel.upload(S.task_panel, s));
  HIPCHK(c, c->d_panel_task.upload(S.panel_task, s));
  HIPCHK(c, c->d_ptri_blk.upload(S.ptri_blk, s));
  HIPCHK(c, c->d_prow_ptr.upload(S.prow_ptr, s));
  HIPCHK(c, c->d_prow_idx.upload(S.prow_idx, s));
  HIPCHK(c, c->d_prow_blk.upload(S.prow_blk, s));
  HIPCHK(c, c->d_pchunk_panel.upload(S.pchunk_panel, s));
  HIPCHK(c, c->d_pchunk_row0.upload(S.pchunk_row0, s));
  HIPCHK(c, c->d_pchunk_nrows.upload(S.pchunk_nrows, s));
  HIPCHK(c, c->d_panel_chunk0.upload(S.panel_chunk0, s));
  HIPCHK(c, c->d_row_mid.upload(S.row_mid, s));
  HIPCHK(c, c->d_fchunk_col.upload(S.fchunk_col, s));
  HIPCHK(c, c->d_fchunk_e0.upload(S.fchunk_e0, s));
  HIPCHK(c, c->d_pcol_fchunk0.upload(S.pcol_fchunk0, s));
  HIPCHK(c, c->d_pcol_fchunkn.upload(S.pcol_fchunkn, s));
  HIPCHK(c, c->d_ptri_src.upload(T.ptri_src, s));
  HIPCHK(c, c->d_prow_src.upload(T.prow_src, s));
  HIPCHK(c, c->d_rchunk_panel.upload(S.rchunk_panel, s));
  HIPCHK(c, c->d_rchunk_s0.upload(S.rchunk_s0, s));
  HIPCHK(c, c->d_fpart.alloc(S.fchunk_col.size() * 6));
  HIPCHK(c, c->d_bpart.alloc(S.pchunk_panel.size() * PANEL_MAX * 6));
  return FGO_OK;
}

// ---- descriptors: PanelDesc, RowChunk, BwdChunk, triangle launch order, LeafDesc, by-chunk row codes, backward chain
// byc_level / byc_c0: row kernel, by-chunk code table: first level / first chunk that use it
int upload_descriptors(fgo_ctx *c, const Ordering &O, const HostTables &T, const std::vector<int> &task_level, int &byc_level, int &byc_c0) {
  hipStream_t s = c->stream;
  const Symbolic &S = c->S;
  std::vector<PanelDesc> pd((size_t)S.n_panels);
  // operand tiles only for panels that run the panel kernels; PanelDesc::top = the panel's first tile in ptop (device_plan.hpp: NTILE
  // slots of PTOP_TILE doubles per panel)
  int64_t n_tiles = 0;
  for (int pn = 0; pn < S.n_panels; ++pn) {
    const int t = S.panel_task[pn];
    const int rows = S.prow_ptr[pn + 1] - S.prow_ptr[pn];
    const bool has = S.level_panel[task_level[t]];
    pd[pn] = PanelDesc{t, S.task_ptr[t + 1] - S.task_ptr[t], S.task_ptr[t], S.prow_ptr[pn], rows, S.panel_chunk0[pn],
                       (rows + PANEL_ROWS - 1) / PANEL_ROWS, has ? (int)n_tiles : -1};
    if (has) n_tiles += NTILE;
  }
  if (n_tiles > INT32_MAX) return fail(c, FGO_ENOMEM, "operand-tile table too large");
  HIPCHK(c, c->d_ptop.alloc((size_t)n_tiles * PTOP_TILE));
  std::vector<RowChunk> rc(S.rchunk_panel.size());
  for (size_t q = 0; q < rc.size(); ++q) {
    const PanelDesc &d = pd[S.rchunk_panel[q]];
    rc[q] = RowChunk{S.rchunk_panel[q], d.m, S.rchunk_s0[q], 6 * d.nrows, d.prow0, d.cols0, d.top, d.task};
  }
  std::vector<BwdChunk> bc(S.pchunk_panel.size());
  for (size_t q = 0; q < bc.size(); ++q) bc[q] = BwdChunk{S.pchunk_panel[q], pd[S.pchunk_panel[q]].m, S.pchunk_row0[q], S.pchunk_nrows[q]};
  HIPCHK(c, c->d_pdesc.upload(pd, s));
  {
    // Launch order of the throughput triangle kernels (k_panel_tri1, k_panel_tri<8>) within a level: by panel WIDTH instead of
    // task order.  A wide level is 1.5-3 rounds of panel workgroups, a panel's time goes with its column count, and k_panel_tri1
    // is 79 KB of straight-line code for a 64 KB instruction cache that two CUs share -- neighbours of equal width run in step
    // and share its lines.  Measured on cfg 2 (us per launch, levels 1 / 2 / 4 / 5; task order 123 / 96 / 62 / 44): widest first
    // 113 / 105 / 47 / 35, narrowest first 105 / 99 / 51 / 37, alternating 148 / 101 / 72 / 45.  -> one wave per panel
    // (k_panel_tri1): narrowest first; eight waves (k_panel_tri<8>): widest first.  FGO_TUNE tri_lpt = 0 task order, 2 / 3 force.
    std::vector<int> order((size_t)S.n_panels);
    for (int pn = 0; pn < S.n_panels; ++pn) order[(size_t)pn] = pn;
    const int mode = (int)tune("tri_lpt", 1);
    // (select_tri reads HostSchedule::cus and level_ptr, nothing else)
    if (mode != 0)
      for (size_t l = 0; l + 1 < S.level_ptr.size(); ++l) {
        const int ntf = S.level_ptr[l + 1] - S.level_ptr[l];
        if (!S.level_panel[l] || ntf <= 0) continue;
        const int p0 = S.task_panel[S.level_ptr[l]], p1 = p0 + ntf;
        if (p0 < 0 || p1 > S.n_panels) continue;
        const bool tri1 = select_tri(c->sched, (int)l) == LF_TRI1;   // (launch_factor's choice)
        const bool ascending = mode == 2 || (mode == 1 && tri1);
        if (ascending) std::stable_sort(order.begin() + p0, order.begin() + p1, [&](int a, int b) { return pd[(size_t)a].m < pd[(size_t)b].m; });
        else std::stable_sort(order.begin() + p0, order.begin() + p1, [&](int a, int b) { return pd[(size_t)a].m > pd[(size_t)b].m; });
      }
    HIPCHK(c, c->d_tri_order.upload(order, s));
  }
  {
    // k_chol_leaf: one descriptor per light sub-tree instead of the chain task -> task_ptr -> task_cols -> colptr -> op_ptr (four
    // dependent round trips at the head of a workgroup that lives ~40 us), and the tasks of a leaf level by DESCENDING work for full
    // sweeps (the last round of a launch -- 3.6 rounds of 768 workgroups at cfg 2 -- is then the light ones)
    const int ntask = (int)S.task_ptr.size() - 1;
    std::vector<LeafDesc> ld((size_t)ntask, LeafDesc{0, 0, 0, 0, 0, 0, 0, 0}), lpt;
    for (size_t l = 0; l + 1 < S.level_ptr.size(); ++l) {
      if (l >= S.level_leaf.size() || !S.level_leaf[l]) continue;
      for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t) {
        const int cb = S.task_ptr[t], m = S.task_ptr[t + 1] - cb, k0 = S.task_cols[cb];
        const int64_t base = S.colptr[k0], nblk = S.colptr[k0 + m] - base, ob = S.op_ptr[base];
        ld[(size_t)t] = LeafDesc{t, cb, m, k0, (long long)base, (long long)ob, (int)nblk, (int)(S.op_ptr[base + nblk] - ob)};
      }
    }
    lpt = ld;
    if (tune("leaf_lpt", 1) != 0)
      for (size_t l = 0; l + 1 < S.level_ptr.size(); ++l)
        if (l < S.level_leaf.size() && S.level_leaf[l])
          std::stable_sort(lpt.begin() + S.level_ptr[l], lpt.begin() + S.level_ptr[l + 1], [](const LeafDesc &a, const LeafDesc &b) { return a.nops + 2 * a.nblk > b.nops + 2 * b.nblk; });
    HIPCHK(c, c->d_leaf_desc.upload(ld, s));
    HIPCHK(c, c->d_leaf_lpt.upload(lpt, s));
  }
  HIPCHK(c, c->d_rchunks.upload(rc, s));
  {
    // NARROW levels (a single round of few row waves: a pure chain of dependent round trips): the source codes of a chunk's 16 scalar rows in a
    // table laid out BY CHUNK, addressed by the chunk index alone and so requested beside the chunk's descriptor instead of after it.  (On the wide
    // levels the 16 code rows per chunk cost more cache lines than the round trip is worth: measured, profiles/NOTES.md.)
    const int thr = (int)tune("rows_byc", 600);                      // row chunks per level below which the table is used (0: never)
    const int nl = (int)S.rchunk_ptr.size() - 1;
    int l0 = nl;
    while (l0 > 0 && S.rchunk_ptr[l0] - S.rchunk_ptr[l0 - 1] < thr) --l0;
    byc_level = l0 < nl && thr > 0 ? l0 : (1 << 30);
    byc_c0 = byc_level < nl ? S.rchunk_ptr[byc_level] : (int)rc.size();
    std::vector<int> rsrc((rc.size() - (size_t)byc_c0) * 16 * PANEL_MAX, -1);
    for (size_t q = (size_t)byc_c0; q < rc.size(); ++q) {
      const RowChunk &r = rc[q];
      for (int nn = 0; nn < 16; ++nn) {
        const int sr = r.s0 + nn;
        int *dst = rsrc.data() + ((q - (size_t)byc_c0) * 16 + nn) * PANEL_MAX;
        if (sr < r.R6) { const size_t ro = S.row_off(r.prow0 + sr / 6); for (int k = 0; k < r.m; ++k) dst[k] = T.prow_src[ro + k]; }
        else if (sr == r.R6) for (int k = 0; k < r.m; ++k) dst[k] = S.task_cols[r.cols0 + k];
      }
    }
    if (!rsrc.empty()) HIPCHK(c, c->d_rchunk_src.upload(rsrc, s)); else c->d_rchunk_src.release();
  }
  // backward chain (k_bwd_chain): the top levels of the tree -- from the root level down while a level consists of panels and
  // has few of them -- run in ONE launch, a workgroup per panel in top-down order, each waiting for the panels above
  {
    static const int chain_on = (int)tune("bwd_chain", 1);
    static const int chain_max = (int)tune("bwd_chain_max", 64);   // panels per level
    std::vector<ChainItem> items;
    const int nl = (int)S.level_ptr.size() - 1;
    int low = nl, chain_levels = 0;
    // (distributed: the segments of the replicated top only -- a rank's own segments run after it, level by level)
    static const int chain_dist = (int)tune("bwd_chain_dist", 1);
    if (chain_on && (O.world == 1 || chain_dist) && !std::getenv("FGO_NO_PANELS"))
      for (int l = nl - 1; l >= 1; --l) {
        if (O.world > 1 && S.seg_group[l] != O.world) continue;
        const int nt = S.level_ptr[l + 1] - S.level_ptr[l];
        if (!S.level_panel[l] || nt > chain_max || nt == 0) break;
        const int need = (int)items.size();
        for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t) items.push_back(ChainItem{S.task_panel[t], need});
        low = l;
        ++chain_levels;
      }
    // a single level gains nothing.  (Counted in LEVELS placed in the chain, not in schedule segments between `low` and the root:
    //  distributed, the domains' segments interleave with the top's and said nothing about the chain's length -- ADVICE r5)
    if (chain_levels < 2) { items.clear(); low = -1; }
    c->sched.bchain_low = items.empty() ? -1 : low;
    c->sched.bchain_n = (int)items.size();
    HIPCHK(c, c->d_bchain.upload(items, s));
    HIPCHK(c, c->d_bchain_done.alloc(1));
    HIPCHK(c, hipMemsetAsync(c->d_bchain_done.p, 0, sizeof(unsigned), s));
  }
  HIPCHK(c, c->d_bchunks.upload(bc, s));
  HIPCHK(c, hipStreamSynchronize(s));       // the staging vectors die at the end of this scope
  return FGO_OK;
}

// ---- work buffers: poses, H / b, x, L, scalars, reduction scratch
int alloc_work_buffers(fgo_ctx *c, const VarIndex &V, const PairGraph &G, const Ordering &O, const HostTables &T, size_t hub_cap) {
  hipStream_t s = c->stream;
  const Symbolic &S = c->S;
  const int64_t N = V.N, R = V.R, NX = V.NX;
  const int nb = O.nb, n_lm = V.n_lm;
  const size_t hblocks = (size_t)nb + (size_t)G.noff;
  c->plan.n_hblocks = (int64_t)hblocks;
  for (int i = 0; i < 2; ++i) {
    HIPCHK(c, c->d_poses[i].alloc((size_t)NX * 8));
    if (R > 0) HIPCHK(c, hipMemsetAsync(c->d_poses[i].p + (size_t)N * 8, 0, sizeof(double) * (size_t)R * 8, s));
    HIPCHK(c, c->d_H[i].alloc(hblocks * 36));
    HIPCHK(c, c->d_b[i].alloc(((size_t)nb + (size_t)n_lm) * 6));          // (+ the virtual columns of eliminated landmarks)
    HIPCHK(c, hipMemsetAsync(c->d_H[i].p, 0, sizeof(double) * hblocks * 36, s));
  }
  HIPCHK(c, c->d_x.alloc(((size_t)nb + (size_t)n_lm) * 6));
  // behind the factor: the zero block (nnzL), an identity block (nnzL + 1) and the scratch blocks of hub targets' rider pieces
  HIPCHK(c, c->d_L.alloc(((size_t)S.nnzL + 2 + (size_t)S.n_scratch) * 36));
  HIPCHK(c, hipMemsetAsync(c->d_L.p + (size_t)S.nnzL * 36, 0, sizeof(double) * 36 * (2 + (size_t)S.n_scratch), s));
  {
    static const double ident[36] = {1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1};
    HIPCHK(c, hipMemcpyAsync(c->d_L.p + ((size_t)S.nnzL + 1) * 36, ident, sizeof(ident), hipMemcpyHostToDevice, s));
  }
  HIPCHK(c, c->d_scal.alloc(8));
  HIPCHK(c, c->d_fail.alloc(1));
  HIPCHK(c, hipMemsetAsync(c->d_fail.p, 0, sizeof(int), s));
  // two-pass reduction scratch, sized from the real launch shapes: linearise = ceil(4N/256) lane-group workgroups + one
  // per hub variable (bounded by 2E / HUB_DEG, NOT by N / HUB_DEG) + one per IMU factor; chi2 <= 2048 + ceil(NI/64);
  // maxdiag <= 1024; update / relinearise ceil(N/256)
  const size_t npart = std::max<size_t>({(size_t)4096, (size_t)((NX * 4 + 255) / 256) + hub_cap + (size_t)T.NI_cap + 64 + (size_t)((n_lm + 255) / 256),
                                         (size_t)2048 + (size_t)((T.NI_cap + 63) / 64) + 64, (size_t)((NX + 255) / 256) + 64});
  HIPCHK(c, c->d_imu_stash.alloc((size_t)T.NI_cap * 150));
  HIPCHK(c, c->d_partial.alloc(npart));
  HIPCHK(c, hipStreamSynchronize(s));
  return FGO_OK;
}

// ---- DevPlan: the pointers, after the uploads they point at
void fill_plan(fgo_ctx *c, const VarIndex &V, const Ordering &O, const HostTables &T, const HubPlan &hubs, int byc_level, int byc_c0, BuildTimer &tm) {
  const Symbolic &S = c->S;
  DevPlan &P = c->plan;
  P.n_poses = V.NX; P.edge_stride = T.E_cap; P.nb = O.nb; P.pose_col = c->d_pose_col.p; P.imu_stash = c->d_imu_stash.p;
  set_factor_plan(c, V.N, V.E, V.NI, hubs, (int64_t)T.dup_ptr.size() - 1);
  P.lin_priors = 1;                               // (the prior CSR above already holds this rank's priors only)
  P.zero_offdiag = O.dist ? 1 : 0;
  P.dist = O.dist ? 1 : 0; P.top_col0 = O.top_col0; P.top_blk0 = O.top_blk0;
  P.top_ext0 = c->d_top_ext0.p; P.own_op0 = c->d_own_op0.p; P.own_op1 = c->d_own_op1.p;
  P.top_row0 = c->d_top_row0.p; P.own_row0 = c->d_own_row0.p; P.own_row1 = c->d_own_row1.p;
  P.var_mine = O.dist ? c->d_var_mine.p : nullptr; P.lambda_rank = O.rank == 0 ? 1 : 0;
  P.colptr = c->d_colptr.p; P.rowidx = c->d_rowidx.p; P.asrc = c->d_asrc.p;
  P.zero_blk = (int)S.nnzL;
  P.prof_tri = std::getenv("FGO_TRI_PROF") ? std::atoi(std::getenv("FGO_TRI_PROF")) : 0;
  P.op_ptr = c->d_op_ptr.p; P.op_mid = c->d_op_mid.p; P.op_a = c->d_op_a.p; P.op_b = c->d_op_b.p;
  P.acc_targets = c->d_acc_targets.p;
  P.g2_tgt = c->d_g2_tgt.p; P.g2_ptr = c->d_g2_ptr.p; P.g2_b = c->d_g2_b.p; P.g2_a = c->d_g2_a.p;
  P.task_dirty = nullptr; P.acc_task = c->isam.d_acc_task.p; P.g2_task = c->isam.d_g2_task.p; P.tcol_task = c->isam.d_tcol_task.p;
  P.ride_xcd = (int)tune("ride_xcd", 1);
  P.ride_items = S.ride_items.empty() ? nullptr : c->d_ride_items.p; P.acc_start = S.acc_start.empty() ? nullptr : c->d_acc_start.p; P.acc_desc = c->d_acc_desc.p;
  P.rowptr = c->d_rowptr.p; P.row_blk = c->d_row_blk.p; P.row_col = c->d_row_col.p;
  P.task_ptr = c->d_task_ptr.p; P.task_cols = c->d_task_cols.p;
  P.partial = c->d_partial.p;
  P.pp.task_panel = c->d_task_panel.p; P.pp.panel_task = c->d_panel_task.p; P.pp.ptri_blk = c->d_ptri_blk.p;
  P.pp.prow_ptr = c->d_prow_ptr.p; P.pp.prow_idx = c->d_prow_idx.p; P.pp.prow_blk = c->d_prow_blk.p;
  P.pp.pchunk_panel = c->d_pchunk_panel.p; P.pp.pchunk_row0 = c->d_pchunk_row0.p; P.pp.pchunk_nrows = c->d_pchunk_nrows.p;
  P.pp.panel_chunk0 = c->d_panel_chunk0.p; P.pp.row_mid = c->d_row_mid.p; P.pp.fchunk_col = c->d_fchunk_col.p;
  P.pp.fchunk_e0 = c->d_fchunk_e0.p; P.pp.pcol_fchunk0 = c->d_pcol_fchunk0.p; P.pp.pcol_fchunkn = c->d_pcol_fchunkn.p;
  P.pp.fpart = c->d_fpart.p; P.pp.bpart = c->d_bpart.p; P.pp.ptop = c->d_ptop.p;
  P.pp.rchunk_panel = c->d_rchunk_panel.p; P.pp.rchunk_s0 = c->d_rchunk_s0.p; P.pp.rchunk_src = c->d_rchunk_src.p; P.pp.rchunk_src0 = byc_c0; c->sched.rows_byc_level = c->d_rchunk_src.p ? byc_level : (1 << 30);
  P.pp.ptri_src = c->d_ptri_src.p; P.pp.prow_src = c->d_prow_src.p;
  P.pp.pdesc = c->d_pdesc.p; P.pp.tri_order = c->d_tri_order.p; P.pp.leaf_desc = c->d_leaf_desc.p; P.pp.leaf_lpt = c->d_leaf_lpt.p; P.pp.rchunks = c->d_rchunks.p; P.pp.bchunks = c->d_bchunks.p; P.pp.bchain = c->d_bchain.p; P.pp.bchain_done = c->d_bchain_done.p;
  if (tm.prof)
    for (size_t l = 0; l < S.level_leaf.size(); ++l)
      if (S.level_leaf[l]) {
        // distribution of the leaf tasks' sizes: the level's launch reserves LDS for the LARGEST task in every workgroup
        std::vector<int64_t> nb_t;
        int64_t cols = 0;
        for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t) {
          const int c0 = S.task_ptr[t], m = S.task_ptr[t + 1] - c0;
          nb_t.push_back(S.colptr[S.task_cols[c0] + m] - S.colptr[S.task_cols[c0]]); cols += m;
        }
        std::sort(nb_t.begin(), nb_t.end());
        std::fprintf(stderr, "[fgo build]    leaf level %zu: %zu tasks, %lld columns, blocks per task min %lld / median %lld / p90 %lld / max %d, most ops %d\n", l,
                     nb_t.size(), (long long)cols, (long long)nb_t.front(), (long long)nb_t[nb_t.size() / 2], (long long)nb_t[nb_t.size() * 9 / 10], S.level_leaf_maxblk[l],
                     S.level_leaf_maxops[l]);
      }
}

}  // namespace

int upload_structure(fgo_ctx *c, const VarIndex &V, const PairGraph &G, const Ordering &O, const HostTables &T, const BaTables &BA, BuildTimer &tm) {
  const Symbolic &S = c->S;
  HubPlan hubs;
  size_t hub_cap = 0;
  int byc_level = 1 << 30, byc_c0 = 0, rc;
  std::vector<int> task_level((size_t)S.task_ptr.size() - 1, 0);
  for (size_t l = 0; l + 1 < S.level_ptr.size(); ++l)
    for (int t = S.level_ptr[l]; t < S.level_ptr[l + 1]; ++t) task_level[t] = (int)l;
  if ((rc = upload_factor_side(c, V, O, T, hubs, hub_cap)) != FGO_OK) return rc;
  if ((rc = host_schedule(c, O)) != FGO_OK) return rc;
  if ((rc = upload_symbolic(c, O, T)) != FGO_OK) return rc;
  claim_L(c);                                        // (d_L is re-allocated below)
  if ((rc = partial_sweep_tables(c, V, O, task_level, tm)) != FGO_OK) return rc;
  if ((rc = upload_panel_lists(c, T)) != FGO_OK) return rc;
  if ((rc = upload_descriptors(c, O, T, task_level, byc_level, byc_c0)) != FGO_OK) return rc;
  if ((rc = alloc_work_buffers(c, V, G, O, T, hub_cap)) != FGO_OK) return rc;
  if ((rc = ba_upload(c, V, O, BA)) != FGO_OK) return rc;
  fill_plan(c, V, O, T, hubs, byc_level, byc_c0, tm);
  if (V.R > 0) snapshot_for_growth(c, V, G, O, T, hubs.deg_limit, hub_cap);
  c->built_N = V.N;
  c->cur = 0;
  c->sinv.release();                                  // the selected inversion's tables belong to the old structure
  c->h_pose_col.clear();
  c->structure_dirty = false;
  c->host_poses_newer = true;
  c->lin_valid = false;
  return FGO_OK;
}

}  // namespace fgo
