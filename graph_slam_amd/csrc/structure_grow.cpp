// Structure phase, growth: the in-place extension of the incremental mode (refresh_factors), the snapshot of the build it works
// on, and the factor-side helpers that the build and the extension both call.
#include "structure_build.hpp"

namespace fgo {

void plan_hubs(const std::vector<int64_t> &he_ptr, int64_t NX, int deg_limit, HubPlan &hp) {
  static const int env_limit = (int)tune("hub_deg", 0);
  if (deg_limit <= 0 && env_limit > 0) deg_limit = env_limit;
  if (deg_limit <= 0) {
    deg_limit = HUB_DEG;
    for (int T = 64; T < HUB_DEG; T *= 2) {
      int64_t n = 0;
      for (int64_t v = 0; v < NX && n <= HUB_MAX_VARS; ++v) n += he_ptr[v + 1] - he_ptr[v] > T;
      if (n <= HUB_MAX_VARS) { deg_limit = T; break; }
    }
  }
  hp.deg_limit = deg_limit;
  hp.var.clear(); hp.slice.clear(); hp.multi.clear();
  for (int64_t v = 0; v < NX; ++v) {
    const int ns = hub_slices(he_ptr[v + 1] - he_ptr[v], deg_limit);
    if (ns == 0) continue;
    if (ns > 1) { hp.multi.push_back((int)v); hp.multi.push_back((int)hp.var.size()); hp.multi.push_back(ns); }
    for (int q = 0; q < ns; ++q) { hp.var.push_back((int)v); hp.slice.push_back(q | (ns << 16)); }
  }
}

// IMU factors by colour.  A factor takes the smallest of 64 colours that none of its six variables carries yet, or -- a
// variable shared by more than 64 factors -- a colour of its own; the factors of one colour therefore touch disjoint H
// blocks, and a launch per colour (launch_linearize_gtsam) adds them into H without atomics, in a fixed order.  A chain of
// CombinedImuFactors (gtsam/test_ba_imu_graph.cpp:239-244: X/V/B of keyframe k shared with the next factor) takes two.
void imu_colour_add(fgo_ctx *c, int64_t f) {
  uint64_t used = 0;
  for (int u = 0; u < 6; ++u) used |= c->imu_var_mask[(size_t)c->imu_ids[6 * f + u]];
  int col;
  if (~used) {
    col = __builtin_ctzll(~used);
    for (int u = 0; u < 6; ++u) c->imu_var_mask[(size_t)c->imu_ids[6 * f + u]] |= (uint64_t)1 << col;
  } else {
    col = 64 + c->imu_extra++;
  }
  c->imu_flist.push_back((int)f);
  c->imu_fcolor.push_back(col);
}
// colour-sorted list (stable: input order inside a colour) and its offsets
void imu_colour_lists(fgo_ctx *c, std::vector<int> &sorted) {
  const int ncol = 64 + c->imu_extra;
  std::vector<int> cnt((size_t)ncol + 1, 0);
  for (int col : c->imu_fcolor) cnt[(size_t)col + 1]++;
  for (int k = 0; k < ncol; ++k) cnt[(size_t)k + 1] += cnt[(size_t)k];
  c->imu_color_ptr = cnt;
  sorted.resize(c->imu_flist.size());
  for (size_t i = 0; i < c->imu_flist.size(); ++i) sorted[(size_t)cnt[(size_t)c->imu_fcolor[i]]++] = c->imu_flist[i];
}

// unary priors: CSR per variable (stable in insertion order) + SoA payload with the inverse mean; `mine` selects the
// priors this rank evaluates (distributed mode)
int upload_priors(fgo_ctx *c, int64_t NX, const std::vector<unsigned char> &mine) {
  hipStream_t s = c->stream;
  const int64_t NPall = (int64_t)c->prior_v.size();
  int64_t NP = 0;
  for (int64_t q = 0; q < NPall; ++q) NP += mine[c->prior_v[q]];
  std::vector<int64_t> prior_ptr((size_t)NX + 1, 0);
  std::vector<int> prior_pose((size_t)NP);
  std::vector<double> prior_minv((size_t)7 * NP), prior_info((size_t)21 * NP);
  for (int64_t q = 0; q < NPall; ++q) if (mine[c->prior_v[q]]) prior_ptr[c->prior_v[q] + 1]++;
  for (int64_t v = 0; v < NX; ++v) prior_ptr[v + 1] += prior_ptr[v];
  std::vector<int64_t> fill(prior_ptr.begin(), prior_ptr.end() - 1);
  for (int64_t q = 0; q < NPall; ++q) {
    if (!mine[c->prior_v[q]]) continue;
    const int64_t o = fill[c->prior_v[q]]++;
    prior_pose[o] = c->prior_v[q];
    double a[7];
    if (c->var_kind[c->prior_v[q]] == 0) pose_inv7(&c->prior_mean[(size_t)q * 7], a);
    else std::memcpy(a, &c->prior_mean[(size_t)q * 7], sizeof(a));     // vector-valued variables: raw mean
    for (int k = 0; k < 7; ++k) prior_minv[(size_t)k * NP + o] = a[k];
    for (int k = 0; k < 21; ++k) prior_info[(size_t)k * NP + o] = c->prior_info[(size_t)q * 21 + k];
  }
  HIPCHK(c, c->d_prior_ptr.upload(prior_ptr, s));
  HIPCHK(c, c->d_prior_pose.upload(prior_pose, s));
  HIPCHK(c, c->d_prior_minv.upload(prior_minv, s));
  HIPCHK(c, c->d_prior_info.upload(prior_info, s));
  HIPCHK(c, hipStreamSynchronize(s));                 // the staging vectors die here
  c->n_priors_dev = NP;
  return FGO_OK;
}

int upload_hubs(fgo_ctx *c, const HubPlan &hp, size_t entry_cap) {
  hipStream_t s = c->stream;
  const size_t cap = std::max(entry_cap, hp.var.size());
  HIPCHK(c, c->d_hub_list.alloc(cap));
  HIPCHK(c, c->d_hub_slice.alloc(cap));
  HIPCHK(c, c->d_hub_part.alloc(cap * HUB_PART));
  HIPCHK(c, c->d_hubm.alloc(3 * cap));
  if (!hp.var.empty()) {
    HIPCHK(c, hipMemcpyAsync(c->d_hub_list.p, hp.var.data(), sizeof(int) * hp.var.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->d_hub_slice.p, hp.slice.data(), sizeof(int) * hp.slice.size(), hipMemcpyHostToDevice, s));
  }
  if (!hp.multi.empty()) HIPCHK(c, hipMemcpyAsync(c->d_hubm.p, hp.multi.data(), sizeof(int) * hp.multi.size(), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipStreamSynchronize(s));        // the caller's HubPlan may die right after
  c->hub_entry_cap = cap;
  c->n_hub_vars = 0;
  for (const int sl : hp.slice) c->n_hub_vars += (sl & 0xffff) == 0;
  return FGO_OK;
}

// Every factor-side field of DevPlan: edges, half-edges, hubs, duplicate groups, priors, IMU factors, gravity and camera -- after the
// uploads they point at (the build, and again whenever refresh_factors extended the lists in place)
void set_factor_plan(fgo_ctx *c, int64_t N, int64_t E, int64_t NI, const HubPlan &hubs, int64_t n_dup_groups) {
  DevPlan &P = c->plan;
  P.n_real = N; P.n_edges = E; P.edge_i = c->d_edge_i.p; P.edge_j = c->d_edge_j.p;
  P.ainv = c->d_ainv.p; P.info = c->d_ainv.p + 8; P.edge_slot = c->d_edge_slot.p;
  P.he_ptr = c->d_he_ptr.p; P.he = c->d_he.p;
  P.hub_list = c->d_hub_list.p; P.hub_slice = c->d_hub_slice.p; P.n_hubs = (int)hubs.var.size(); P.hub_deg = hubs.deg_limit;
  P.hub_part = c->d_hub_part.p; P.hubm = c->d_hubm.p; P.n_hub_multi = (int)(hubs.multi.size() / 3);
  P.n_dup_groups = n_dup_groups; P.dup_ptr = c->d_dup_ptr.p; P.dup_edges = c->d_dup_edges.p; P.dup_slot = c->d_dup_slot.p;
  P.n_priors = c->n_priors_dev; P.prior_ptr = c->d_prior_ptr.p; P.prior_pose = c->d_prior_pose.p;
  P.prior_minv = c->d_prior_minv.p; P.prior_info = c->d_prior_info.p;
  P.var_kind = c->d_var_kind.p; P.edge_kind = c->d_edge_kind.p; P.cam = c->cam;
  P.n_imu = NI; P.imu = c->d_imu.p; P.imu_ids = c->d_imu_ids.p; P.imu_slot = c->d_imu_slot.p;
  P.imu_fn = (int64_t)c->imu_flist.size(); P.imu_list = c->d_imu_list.p;
  P.imu_ncolor = (int)c->imu_color_ptr.size() - 1; P.imu_color_ptr_h = c->imu_color_ptr.data();
  for (int k = 0; k < 3; ++k) P.gravity[k] = c->gravity[k];
}

// Appends the entries `ins` (variable, entry) to the per-variable CSR (ptr, list) in one merge pass: per-variable insert counts ->
// new offsets by a prefix sum -> the old lists copied in order with the new entries behind each variable's old ones, in the order
// given (the order inside a list is the summation order): O(NX + moved suffix), however many entries.  Returns the lowest variable
// touched (NX: none): `list` changed from ptr[v_lo] on, `ptr` from v_lo + 1 on.
static int64_t csr_insert(std::vector<int64_t> &ptr, std::vector<int> &list, std::vector<std::pair<int, int>> &ins) {
  const int64_t NX = (int64_t)ptr.size() - 1;
  if (ins.empty()) return NX;
  std::stable_sort(ins.begin(), ins.end(), [](const std::pair<int, int> &a, const std::pair<int, int> &b) { return a.first < b.first; });
  const int64_t v_lo = ins.front().first, p_lo = ptr[v_lo];
  std::vector<int> tail(list.begin() + p_lo, list.end());    // old entries of the variables >= v_lo
  list.resize(list.size() + ins.size());
  size_t q = 0;
  int64_t w = p_lo, shift = 0;
  for (int64_t v = v_lo; v < NX; ++v) {
    const int64_t o0 = ptr[v] - shift - p_lo, o1 = ptr[v + 1] - p_lo;   // ptr[v] already carries `shift`, ptr[v+1] not yet
    for (int64_t r = o0; r < o1; ++r) list[w++] = tail[(size_t)r];
    while (q < ins.size() && ins[q].first == v) { list[w++] = ins[q].second; ++q; ++shift; }
    ptr[v + 1] += shift;
  }
  return v_lo;
}

// what refresh_factors needs to append factors / claim phantom slots without touching the structure
void snapshot_for_growth(fgo_ctx *c, const VarIndex &V, const PairGraph &G, const Ordering &O, const HostTables &T, int hub_deg, size_t hub_cap) {
  const int64_t noff = G.noff;
  fgo_ctx::Incr &I = c->inc;
  I.NX = V.NX; I.N_done = V.N; I.E_done = V.E; I.NI_done = V.NI; I.NP_done = (int64_t)c->prior_v.size(); I.nb = O.nb;
  I.hidx = V.hidx; I.pose_col = T.pose_col;
  I.ukey.resize((size_t)noff);
  for (int64_t h = 0; h < noff; ++h) I.ukey[h] = pair_key(G.ua[h], G.ub[h]);
  I.edge_h.assign((size_t)V.E, -1);
  I.pair_nbin.assign((size_t)noff, 0); I.pair_first.assign((size_t)noff, -1);
  I.dups.clear();
  for (int64_t h = 0; h < noff; ++h)
    for (int64_t m = G.ufirst[h]; m < G.ufirst[h + 1]; ++m) {
      const int64_t e = G.pr[m].e;
      if (e < 0) continue;                         // IMU pair or structure-only
      I.edge_h[e] = (int)h;
      if (I.pair_nbin[h]++ == 0) I.pair_first[h] = (int)e;
    }
  for (int64_t h = 0; h < noff; ++h)
    if (I.pair_nbin[h] > 1)
      for (int64_t m = G.ufirst[h]; m < G.ufirst[h + 1]; ++m) if (G.pr[m].e >= 0) I.dups[(int)h].push_back(G.pr[m].e);
  I.edge_slot = T.edge_slot;
  I.he_ptr = T.he_ptr; I.he = T.he; I.imu_inc_ptr = T.imu_inc_ptr; I.imu_inc = T.imu_inc;
  I.hub_deg = hub_deg; I.hub_cap = hub_cap;
  I.E_cap = T.E_cap; I.NI_cap = T.NI_cap; I.valid = true;
}

// Incremental mode: the graph grew since the structure was built.  If the new variables fit the phantom slots, every
// new factor couples variables whose pair already exists in the structure (a fixed end needs none), the factors fit the
// capacities laid down at the build and the hub entries of the extended graph fit hub_cap, the factor-side device arrays are
// extended in place: returns FGO_OK (done), 1 (does not fit: the caller rebuilds), or an error.  DESIGN.md "Growing graphs" has
// the table; tests/test_gpu_growth_forms.py holds its rows on variables, factors, duplicates, hubs and priors to H / b.
int refresh_factors(fgo_ctx *c) {
  fgo_ctx::Incr &I = c->inc;
  const bool growing = c->gtsam_mode ? c->isam_incremental : c->grow_incremental;
  if (!I.valid || !growing || c->shard_world > 1) return 1;
  const double t0 = now_s();
  const int64_t N = (int64_t)c->ids.size(), E = (int64_t)c->ei.size(), NI = (int64_t)c->imu_payload.size();
  if (N > I.NX || E > I.E_cap || NI > I.NI_cap || N < I.N_done || E < I.E_done || NI < I.NI_done) return 1;
  for (int64_t v = I.N_done; v < N; ++v) if (c->fixed[v]) return 1;
  // (a context holds either g2o-semantics edges or GTSAM-semantics factors: anything that would change the mode rebuilds, and the
  //  build reports it)
  for (int64_t e = I.E_done; e < E; ++e) if ((c->torder[e] == FGO_TANGENT_G2O) == c->gtsam_mode || (c->torder[e] == 3 && !c->cam_set)) return 1;
  if (!c->gtsam_mode) {
    if (!c->prior_v.empty() || NI > 0) return 1;
    for (int64_t v = I.N_done; v < N; ++v) if (c->var_kind[v] != 0) return 1;
  }
  auto find_pair = [&](int va, int vb) -> int {            // variable indices -> pair index, -1 none needed, -2 missing
    const int a = I.hidx[va], b = I.hidx[vb];
    if (!needs_pair(a, b)) return -1;
    const uint64_t key = pair_key(a, b);
    auto it = std::lower_bound(I.ukey.begin(), I.ukey.end(), key);
    return (it != I.ukey.end() && *it == key) ? (int)(it - I.ukey.begin()) : -2;
  };
  // ---- check everything first: nothing is modified unless the whole delta fits
  std::vector<int> new_h((size_t)(E - I.E_done));
  for (int64_t e = I.E_done; e < E; ++e) { const int h = find_pair(c->ei[e], c->ej[e]); if (h == -2) return 1; new_h[(size_t)(e - I.E_done)] = h; }
  std::vector<int> new_imu_slot((size_t)15 * (NI - I.NI_done), -1);
  for (int64_t f = I.NI_done; f < NI; ++f)
    for (int q = 0; q < 15; ++q) {
      const int vu = c->imu_ids[6 * f + IMU_PAIR[q][0]], vw = c->imu_ids[6 * f + IMU_PAIR[q][1]];
      const int h = find_pair(vu, vw);
      if (h == -2) return 1;
      if (h >= 0) new_imu_slot[(size_t)15 * (f - I.NI_done) + q] = h_slot(I.nb, h, I.pose_col[vu], I.pose_col[vw]);
    }
  {   // hub entries (one workgroup per slice of a hub variable) after the extension: the scratch buffers have room for hub_cap
    std::unordered_map<int, int64_t> deg;
    for (int64_t e = I.E_done; e < E; ++e)
      for (const int v : {c->ei[e], c->ej[e]}) {
        auto it = deg.find(v);
        if (it == deg.end()) it = deg.emplace(v, I.he_ptr[v + 1] - I.he_ptr[v]).first;
        ++it->second;
      }
    int64_t n_entries = (int64_t)c->plan.n_hubs;
    for (auto &kv : deg) n_entries += hub_slices(kv.second, I.hub_deg) - hub_slices(I.he_ptr[kv.first + 1] - I.he_ptr[kv.first], I.hub_deg);
    if (n_entries > (int64_t)I.hub_cap) return 1;
  }
  if (c->dev_poses_newer) { const int rc = download_poses(c); if (rc) return rc; }
  destroy_graphs(c);                                           // captured trials hold the factor counts by value
  hipStream_t s = c->stream;
  I.valid = false;                                             // (an error below leaves the lists half-extended: the next call rebuilds)
  // ---- variables: claim phantom slots (kind; the value goes up with upload_poses)
  if (N > I.N_done) {
    HIPCHK(c, hipMemcpyAsync(c->d_var_kind.p + I.N_done, c->var_kind.data() + I.N_done, sizeof(int) * (size_t)(N - I.N_done), hipMemcpyHostToDevice, s));
    c->host_poses_newer = true;
  }
  // ---- binary factors: slots, duplicate groups, payload, incidence lists
  I.edge_h.resize((size_t)E, -1); I.edge_slot.resize((size_t)E, -1);
  int64_t slot_lo = E;                                          // lowest edge whose slot entry changed
  for (int64_t e = I.E_done; e < E; ++e) {
    const int h = new_h[(size_t)(e - I.E_done)];
    I.edge_h[e] = h;
    if (h < 0) continue;
    const int slot = h_slot(I.nb, h, I.pose_col[c->ei[e]], I.pose_col[c->ej[e]]);
    if (I.pair_nbin[h] == 0) { I.pair_first[h] = (int)e; I.edge_slot[e] = slot; }
    else {
      if (I.pair_nbin[h] == 1) { const int f0 = I.pair_first[h]; I.dups[h].push_back(f0); I.edge_slot[f0] = -1; slot_lo = std::min<int64_t>(slot_lo, f0); }
      I.dups[h].push_back(e);
    }
    ++I.pair_nbin[h];
  }
  slot_lo = std::min(slot_lo, I.E_done);
  if (E > slot_lo) HIPCHK(c, hipMemcpyAsync(c->d_edge_slot.p + slot_lo, I.edge_slot.data() + slot_lo, sizeof(int) * (size_t)(E - slot_lo), hipMemcpyHostToDevice, s));
  std::vector<int64_t> dup_ptr{0}, dup_edges;
  std::vector<int> dup_slot;
  for (auto &kv : I.dups) {
    for (int64_t e : kv.second) {
      dup_edges.push_back(e);
      dup_slot.push_back(h_slot(I.nb, kv.first, I.pose_col[c->ei[e]], I.pose_col[c->ej[e]]));
    }
    dup_ptr.push_back((int64_t)dup_edges.size());
  }
  HIPCHK(c, c->d_dup_ptr.upload(dup_ptr, s));
  HIPCHK(c, c->d_dup_edges.upload(dup_edges, s));
  HIPCHK(c, c->d_dup_slot.upload(dup_slot, s));
  c->n_dup_members = (int64_t)dup_edges.size();
  const int64_t dE = E - I.E_done;
  std::vector<double> stage((size_t)28 * dE);
  if (dE > 0) {
    HIPCHK(c, hipMemcpyAsync(c->d_edge_i.p + I.E_done, c->ei.data() + I.E_done, sizeof(int) * (size_t)dE, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->d_edge_j.p + I.E_done, c->ej.data() + I.E_done, sizeof(int) * (size_t)dE, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->d_edge_kind.p + I.E_done, c->torder.data() + I.E_done, sizeof(int) * (size_t)dE, hipMemcpyHostToDevice, s));
    for (int64_t e = I.E_done; e < E; ++e) {                    // SoA payload: staged contiguously, scattered by a kernel
      double *o = &stage[(size_t)28 * (e - I.E_done)];
      edge_payload(c, e, o, o + 7);
    }
    HIPCHK(c, c->d_stage.alloc(stage.size()));
    HIPCHK(c, hipMemcpyAsync(c->d_stage.p, stage.data(), sizeof(double) * stage.size(), hipMemcpyHostToDevice, s));
    launch_scatter_edges(c->d_stage.p, dE, I.E_done, c->d_ainv.p, s);
  }
  // incidence lists: a new factor's half-edges go to the END of its variables' lists (edge order inside a list is what keeps
  // the sums deterministic); everything behind the lowest touched variable moves up and is uploaded again -- new factors
  // attach to the newest variables, so that is a short suffix
  HubPlan hubs;
  {
    std::vector<std::pair<int, int>> ins;                      // (variable, half-edge), edge order
    ins.reserve((size_t)2 * (E - I.E_done));
    for (int64_t e = I.E_done; e < E; ++e) { ins.push_back({c->ei[e], (int)(e << 1)}); ins.push_back({c->ej[e], (int)((e << 1) | 1)}); }
    const int64_t v_lo = csr_insert(I.he_ptr, I.he, ins);
    if (v_lo < I.NX) {
      const int64_t p0 = I.he_ptr[v_lo];
      HIPCHK(c, hipMemcpyAsync(c->d_he.p + p0, I.he.data() + p0, sizeof(int) * (size_t)((int64_t)I.he.size() - p0), hipMemcpyHostToDevice, s));
      HIPCHK(c, hipMemcpyAsync(c->d_he_ptr.p + v_lo, I.he_ptr.data() + v_lo, sizeof(int64_t) * (size_t)(I.NX + 1 - v_lo), hipMemcpyHostToDevice, s));
    }
    plan_hubs(I.he_ptr, I.NX, I.hub_deg, hubs);
    { const int rc = upload_hubs(c, hubs, I.hub_cap); if (rc) return rc; }
  }
  // ---- priors (few): rebuilt
  if ((int64_t)c->prior_v.size() != I.NP_done) {
    std::vector<unsigned char> all((size_t)I.NX, 1);
    const int rc = upload_priors(c, I.NX, all);
    if (rc) return rc;
  }
  // ---- IMU factors: payload / ids / slots appended, incidence rebuilt
  const int64_t dI = NI - I.NI_done;
  std::vector<int> imu_sorted;
  if (dI > 0) {
    HIPCHK(c, hipMemcpyAsync(c->d_imu.p + I.NI_done, c->imu_payload.data() + I.NI_done, sizeof(ImuPayload) * (size_t)dI, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->d_imu_ids.p + 6 * I.NI_done, c->imu_ids.data() + 6 * I.NI_done, sizeof(int) * (size_t)(6 * dI), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->d_imu_slot.p + 15 * I.NI_done, new_imu_slot.data(), sizeof(int) * (size_t)(15 * dI), hipMemcpyHostToDevice, s));
    std::vector<std::pair<int, int>> ins;                        // (variable, incidence entry), factor order
    for (int64_t f = I.NI_done; f < NI; ++f)
      for (int u = 0; u < 6; ++u) ins.push_back({c->imu_ids[6 * f + u], (int)((f << 3) | u)});
    csr_insert(I.imu_inc_ptr, I.imu_inc, ins);
    // the new factors' colours; the colour-sorted list again
    for (int64_t f = I.NI_done; f < NI; ++f) imu_colour_add(c, f);
    imu_colour_lists(c, imu_sorted);
    HIPCHK(c, hipMemcpyAsync(c->d_imu_list.p, imu_sorted.data(), sizeof(int) * imu_sorted.size(), hipMemcpyHostToDevice, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));                           // the staging vectors die here
  // ---- plan
  set_factor_plan(c, N, E, NI, hubs, (int64_t)dup_ptr.size() - 1);
  I.N_done = N; I.E_done = E; I.NI_done = NI; I.NP_done = (int64_t)c->prior_v.size();
  c->n_phantom = (int)(I.NX - N);                               // the new variables took the first phantom slots: the dense read-backs report them
  I.valid = true;
  c->structure_dirty = false;
  c->lin_valid = false;
  drop_undamped(c);
  fgo_stats &st = c->last;
  st.structure_rebuilt = 0;
  c->last_phase_rebuilt = 0;
  st.t_symbolic = now_s() - t0;                                 // host time of the in-place extension
  st.t_upload = 0;
  st.n_edges = E;
  st.n_free = I.nb - c->n_phantom;
  return FGO_OK;
}

}  // namespace fgo
