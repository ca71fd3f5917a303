// Structure phase, bundle adjustment: free Point3 variables that carry reprojection factors (and unary priors) only are eliminated
// analytically (kernels_ba.hip, device_plan.hpp "BaPlan") instead of becoming columns of the block system.  Which landmarks, the
// co-visibility pairs they leave between their cameras, who eliminates them (distributed), the tables and their upload.
#include "structure_build.hpp"

namespace fgo {

// numbers the landmarks to eliminate in V.lm_index (classify; V.lm_index is all -1 and V.n_lm 0 on entry)
void ba_select_landmarks(const fgo_ctx *c, VarIndex &V) {
  const int64_t N = V.N, E = V.E;
  const int ba_on = std::getenv("FGO_BA_SCHUR") ? std::atoi(std::getenv("FGO_BA_SCHUR")) : 1;       // (read per build: tests switch it)
  const int ba_min = std::getenv("FGO_BA_MIN") ? std::atoi(std::getenv("FGO_BA_MIN")) : 1000;
  // (distributed mode: every rank eliminates the SAME set -- the structure is replicated -- and takes the landmarks of its own
  //  domain's cameras, lm_mine below)
  if (ba_on && !c->ba_disable && c->gtsam_mode && !c->isam_incremental && c->cam_set) {
    std::vector<char> ok((size_t)N, 0);
    std::vector<int> deg((size_t)N, 0);
    for (int64_t v = 0; v < N; ++v) ok[v] = c->var_kind[v] == 2 && !c->fixed[v];
    for (int64_t e = 0; e < E; ++e) {
      if (c->torder[e] == 3) { ok[c->ei[e]] = 0; deg[c->ej[e]]++; }
      else { ok[c->ei[e]] = 0; ok[c->ej[e]] = 0; }
    }
    for (int64_t f = 0; f < V.NI; ++f) for (int u = 0; u < 6; ++u) ok[c->imu_ids[6 * f + u]] = 0;
    int cnt = 0;
    for (int64_t v = 0; v < N; ++v) cnt += ok[v] && deg[v] > 0;
    if (cnt >= ba_min) {
      // numbered by the first camera that sees them (then by id): a camera's observations are stored by landmark number, so
      // the landmarks of neighbouring lanes of the per-landmark kernels then sit next to each other in every per-observation
      // array (k_ba_back read 2.1 GB for 0.72 GB of W with the landmarks in id order of a generator that scatters them; a front
      // end that creates landmarks keyframe by keyframe -- gtsam/gtsam_graph.cpp:387-394 -- has this order anyway)
      std::vector<int> first_cam((size_t)N, INT32_MAX);
      for (int64_t e = 0; e < E; ++e) if (c->torder[e] == 3 && ok[c->ej[e]]) first_cam[c->ej[e]] = std::min(first_cam[c->ej[e]], c->ei[e]);
      std::vector<int64_t> start((size_t)N + 1, 0);
      for (int64_t v = 0; v < N; ++v) if (ok[v] && deg[v] > 0) start[(size_t)first_cam[v] + 1]++;
      for (int64_t v = 0; v < N; ++v) start[(size_t)v + 1] += start[(size_t)v];
      for (int64_t v = 0; v < N; ++v) if (ok[v] && deg[v] > 0) { V.lm_index[v] = (int)start[(size_t)first_cam[v]]++; ++V.n_lm; }
    }
  }
}

// the co-visibility pairs, found per camera (in parallel) from its landmarks' camera lists and de-duplicated there
void ba_covisibility_pairs(const fgo_ctx *c, const VarIndex &V, std::vector<PairRec> &pr) {
  const int64_t E = V.E;
  const int n_lm = V.n_lm, nfree = V.nfree;
  std::vector<int64_t> lc_ptr((size_t)n_lm + 1, 0), cl_ptr((size_t)nfree + 1, 0);
  for (int64_t e = 0; e < E; ++e)
    if (c->torder[e] == 3 && V.lm_index[c->ej[e]] >= 0 && V.hidx[c->ei[e]] >= 0) { lc_ptr[V.lm_index[c->ej[e]] + 1]++; cl_ptr[V.hidx[c->ei[e]] + 1]++; }
  for (int p = 0; p < n_lm; ++p) lc_ptr[p + 1] += lc_ptr[p];
  for (int a = 0; a < nfree; ++a) cl_ptr[a + 1] += cl_ptr[a];
  std::vector<int> lc((size_t)lc_ptr[n_lm]), cl((size_t)cl_ptr[nfree]);       // cameras of a landmark / landmarks of a camera
  {
    std::vector<int64_t> f1(lc_ptr.begin(), lc_ptr.end() - 1), f2(cl_ptr.begin(), cl_ptr.end() - 1);
    for (int64_t e = 0; e < E; ++e)
      if (c->torder[e] == 3 && V.lm_index[c->ej[e]] >= 0 && V.hidx[c->ei[e]] >= 0) {
        const int p = V.lm_index[c->ej[e]], a = V.hidx[c->ei[e]];
        lc[f1[p]++] = a; cl[f2[a]++] = p;
      }
  }
  std::vector<std::vector<int>> nbrs((size_t)nfree);
  parallel_ranges(nfree, 64, [&](int a0, int a1) {
    std::vector<int> tmp;
    for (int a = a0; a < a1; ++a) {
      tmp.clear();
      for (int64_t q = cl_ptr[a]; q < cl_ptr[a + 1]; ++q) {
        const int p = cl[q];
        for (int64_t w = lc_ptr[p]; w < lc_ptr[p + 1]; ++w) if (lc[w] > a) tmp.push_back(lc[w]);
      }
      std::sort(tmp.begin(), tmp.end());
      tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
      nbrs[a] = tmp;
    }
  });
  for (int a = 0; a < nfree; ++a) for (int b : nbrs[a]) pr.push_back({a, b, STRUCT_ONLY});
}

// eliminated landmarks: the cameras of one landmark are a clique of the reduced graph (co-visibility pairs), i.e. they lie in ONE
// domain plus the top -- the rank of that domain eliminates the landmark (all of its observations, its prior, its step); landmarks
// seen from top cameras only are dealt round-robin.  Its variable counts as that rank's (unary terms, LM scale, final gather).
int ba_landmark_owners(fgo_ctx *c, const VarIndex &V, const Ordering &O, std::vector<unsigned char> &lm_mine) {
  std::vector<int> owner((size_t)V.n_lm, -1);
  for (int64_t e = 0; e < V.E; ++e) {
    if (c->torder[e] != 3) continue;
    const int p = V.lm_index[c->ej[e]];
    if (p < 0) continue;
    const int gq = c->pose_group[c->ei[e]];
    if (gq >= 0 && gq < O.world) {
      if (owner[p] >= 0 && owner[p] != gq) return fail(c, FGO_EINVAL, "internal: the cameras of an eliminated landmark span two domains");
      owner[p] = gq;
    }
  }
  lm_mine.assign((size_t)V.n_lm, 0);
  for (int64_t v = 0; v < V.N; ++v) {
    const int p = V.lm_index[v];
    if (p < 0) continue;
    if (owner[p] < 0) owner[p] = p % O.world;
    c->pose_group[v] = owner[p];
    lm_mine[p] = owner[p] == O.rank;
  }
  return FGO_OK;
}

// ---- landmark elimination tables (device_plan.hpp "BaPlan")
int ba_tables(fgo_ctx *c, const VarIndex &V, const PairGraph &G, const Ordering &O, const HostTables &T, BaTables &BA, BuildTimer &tm) {
  if (V.n_lm == 0) return FGO_OK;
  const Symbolic &S = c->S;
  const int64_t N = V.N, E = V.E;
  const int n_lm = V.n_lm, nb = O.nb;
  BA.lm_var.resize((size_t)n_lm);
  for (int64_t v = 0; v < N; ++v) if (V.lm_index[v] >= 0) BA.lm_var[V.lm_index[v]] = (int)v;
  // observations camera-major: counting sort on the camera's column (fixed cameras, column -1, first), landmarks ascending inside
  std::vector<int64_t> cstart((size_t)nb + 2, 0);
  int64_t n_obs = 0;
  auto obs_here = [&](int64_t e) { return c->torder[e] == 3 && V.lm_index[c->ej[e]] >= 0 && (BA.lm_mine.empty() || BA.lm_mine[V.lm_index[c->ej[e]]]); };
  for (int64_t e = 0; e < E; ++e) if (obs_here(e)) { cstart[T.pose_col[c->ei[e]] + 2]++; ++n_obs; }
  for (int k = 0; k <= nb; ++k) cstart[k + 1] += cstart[k];
  BA.obs_edge.resize((size_t)n_obs);
  {
    std::vector<int64_t> fill(cstart.begin(), cstart.end() - 1);
    for (int64_t e = 0; e < E; ++e) if (obs_here(e)) BA.obs_edge[fill[T.pose_col[c->ei[e]] + 1]++] = (int)e;
  }
  parallel_ranges(nb + 1, 16, [&](int k0, int k1) {
    for (int k = k0; k < k1; ++k)
      std::sort(BA.obs_edge.begin() + cstart[k], BA.obs_edge.begin() + cstart[k + 1], [&](int x, int y) {
        const int px = V.lm_index[c->ej[x]], py = V.lm_index[c->ej[y]];
        return px != py ? px < py : x < y; });
  });
  tm.lap("  ba: observations camera-major");
  BA.obs_cam.resize((size_t)n_obs); BA.obs_col.resize((size_t)n_obs); BA.obs_lm.resize((size_t)n_obs);
  BA.pt_ptr.assign((size_t)n_lm + 1, 0);
  parallel_ranges((int)std::min<int64_t>(n_obs, INT32_MAX), 1 << 16, [&](int ob, int oe) {
    for (int64_t o = ob; o < oe; ++o) {
      const int e = BA.obs_edge[o];
      BA.obs_cam[o] = c->ei[e]; BA.obs_col[o] = T.pose_col[c->ei[e]]; BA.obs_lm[o] = V.lm_index[c->ej[e]];
    }
  });
  for (int64_t o = 0; o < n_obs; ++o) BA.pt_ptr[BA.obs_lm[o] + 1]++;
  for (int p = 0; p < n_lm; ++p) BA.pt_ptr[p + 1] += BA.pt_ptr[p];
  BA.pt_obs.resize((size_t)n_obs);
  {
    std::vector<int64_t> fill(BA.pt_ptr.begin(), BA.pt_ptr.end() - 1);
    for (int64_t o = 0; o < n_obs; ++o) BA.pt_obs[fill[BA.obs_lm[o]]++] = (int)o;       // ascending o = ascending column
  }
  tm.lap("  ba: per-observation arrays, landmark lists");
  BA.cam_ptr.push_back(cstart[1]);
  for (int k = 0; k < nb; ++k) if (cstart[k + 2] > cstart[k + 1]) { BA.cam_col.push_back(k); BA.cam_ptr.push_back(cstart[k + 2]); }
  // blocks of the reduced system with landmark terms, per column camera k: for its observation o and every observation o2 of
  // the same landmark from a camera of column >= k: block (col(o2), k) -= Y(o2) Y(o)^T
  std::vector<int64_t> ustart((size_t)V.nfree + 1, 0);
  for (int64_t h = 0; h < G.noff; ++h) ustart[G.ua[h] + 1]++;
  for (int a = 0; a < V.nfree; ++a) ustart[a + 1] += ustart[a];
  const int ncam = (int)BA.cam_col.size();
  // two passes over the (observation, observation of the same landmark from a later-or-equal column) pairs of every column
  // camera, both in the same order: count per (camera, row column), prefix sums, fill -- no sorting, no growing vectors.
  // Within a block the pairs keep the emission order (the camera's observations ascending, then the landmark's list).
  std::vector<std::vector<int>> cam_rows((size_t)ncam);          // distinct row columns of a camera, ascending
  std::vector<std::vector<int64_t>> cam_cnt((size_t)ncam);       // pairs per row column
  std::atomic<int> missing{0};
  auto for_each_pair = [&](int i, auto &&fn) {
    const int k = BA.cam_col[i];
    for (int64_t o = BA.cam_ptr[i]; o < BA.cam_ptr[i + 1]; ++o) {
      const int p = BA.obs_lm[o];
      for (int64_t q = BA.pt_ptr[p]; q < BA.pt_ptr[p + 1]; ++q) {
        const int o2 = BA.pt_obs[q];
        if (BA.obs_col[o2] >= k) fn(BA.obs_col[o2], o2, (int)o);
      }
    }
  };
  parallel_ranges(ncam, 4, [&](int i0, int i1) {
    static thread_local std::vector<int> slot;                   // column -> local row index + 1 (0: unseen); reset after use
    if ((int)slot.size() < nb) slot.assign((size_t)nb, 0);
    for (int i = i0; i < i1; ++i) {
      std::vector<int> &rows = cam_rows[(size_t)i];
      for_each_pair(i, [&](int row, int, int) { if (!slot[row]) { slot[row] = 1; rows.push_back(row); } });
      std::sort(rows.begin(), rows.end());
      for (size_t x = 0; x < rows.size(); ++x) slot[rows[x]] = (int)x + 1;
      std::vector<int64_t> &cnt = cam_cnt[(size_t)i];
      cnt.assign(rows.size(), 0);
      for_each_pair(i, [&](int row, int, int) { cnt[slot[row] - 1]++; });
      for (int r : rows) slot[r] = 0;
    }
  });
  tm.lap("  ba: pair counts");
  std::vector<int64_t> t0v((size_t)ncam + 1, 0), e0v((size_t)ncam + 1, 0);
  for (int i = 0; i < ncam; ++i) {
    t0v[i + 1] = t0v[i] + (int64_t)cam_rows[i].size();
    int64_t n = 0;
    for (int64_t x : cam_cnt[i]) n += x;
    e0v[i + 1] = e0v[i] + n;
  }
  BA.tgt_blk.resize((size_t)t0v[ncam]); BA.tgt_ptr.assign((size_t)t0v[ncam] + 1, 0);
  BA.op_a.resize((size_t)e0v[ncam]); BA.op_b.resize((size_t)e0v[ncam]); BA.op_lm.resize((size_t)e0v[ncam]);
  parallel_ranges(ncam, 4, [&](int i0, int i1) {
    static thread_local std::vector<int> slot;
    if ((int)slot.size() < nb) slot.assign((size_t)nb, 0);
    std::vector<int64_t> cur;
    for (int i = i0; i < i1; ++i) {
      const int k = BA.cam_col[i];
      const std::vector<int> &rows = cam_rows[(size_t)i];
      cur.resize(rows.size());
      int64_t at = e0v[i];
      for (size_t x = 0; x < rows.size(); ++x) {
        const int row = rows[x];
        slot[row] = (int)x + 1;
        cur[x] = at;
        at += cam_cnt[(size_t)i][x];
        BA.tgt_ptr[(size_t)t0v[i] + x + 1] = at;
        int blk = -1;
        if (row == k) blk = k;
        else {
          const int ha = std::min(S.perm[k], S.perm[row]), hb = std::max(S.perm[k], S.perm[row]);
          const int *b0 = G.ub.data() + ustart[ha], *b1 = G.ub.data() + ustart[ha + 1];
          const int *f = std::lower_bound(b0, b1, hb);
          if (f != b1 && *f == hb) blk = nb + (int)(f - G.ub.data());
        }
        if (blk < 0) missing++;
        BA.tgt_blk[(size_t)t0v[i] + x] = blk;
      }
      for_each_pair(i, [&](int row, int o2, int o) { const int64_t w = cur[slot[row] - 1]++; BA.op_a[w] = o2; BA.op_b[w] = o; BA.op_lm[w] = BA.obs_lm[o]; });
      for (int r : rows) slot[r] = 0;
    }
  });
  if (missing.load() > 0) return fail(c, FGO_EINVAL, "internal: a co-visibility pair has no block in the reduced system");
  tm.lap("  ba: pair lists");
  // k_ba_schur_cam takes the blocks of a COLUMN camera together (its observations' B = (H_pp + lambda I)^-1 W^T staged in LDS
  // once for all of the camera's blocks); a camera with more row blocks than the kernel has accumulator slots keeps the
  // block-by-block kernel: short lists first (one wave per block), long ones behind (four waves)
  {
    static const int small_max = (int)tune("ba_small", 80);
    static const int cam_on = (int)tune("ba_schur_cam", 1);
    constexpr int CAM_SLOTS = 80;                                 // kernels_ba.hip: lane groups of a k_ba_schur_cam workgroup
    BA.cam_t0 = t0v;
    for (int i = 0; i < ncam; ++i) {
      const bool staged = cam_on && t0v[i + 1] - t0v[i] <= CAM_SLOTS;
      if (staged) BA.cam_list.push_back(i);
      else for (int64_t t = t0v[i]; t < t0v[i + 1]; ++t) BA.tgt_list.push_back((int)t);
    }
    auto mid = std::stable_partition(BA.tgt_list.begin(), BA.tgt_list.end(), [&](int t) { return BA.tgt_ptr[t + 1] - BA.tgt_ptr[t] <= small_max; });
    BA.n_small = (int)(mid - BA.tgt_list.begin());
  }
  BA.obs_uvw.resize(3 * (size_t)n_obs);
  parallel_ranges((int)std::min<int64_t>(n_obs, INT32_MAX), 1 << 16, [&](int ob, int oe) {
    for (int64_t o = ob; o < oe; ++o) {
      const int e = BA.obs_edge[o];
      BA.obs_uvw[3 * o] = c->meas[(size_t)e * 7]; BA.obs_uvw[3 * o + 1] = c->meas[(size_t)e * 7 + 1]; BA.obs_uvw[3 * o + 2] = c->info[(size_t)e * 21];
    }
  });
  BA.o_first = cstart[1];
  if (tm.prof) std::fprintf(stderr, "[fgo build]    landmark elimination: %d landmarks, %lld observations, %d cameras, %zu reduced blocks (%d with <= 80 pairs), %zu pairs\n",
                         n_lm, (long long)n_obs, ncam, BA.tgt_blk.size(), BA.n_small, BA.op_a.size());
  tm.lap("landmark elimination tables");
  return FGO_OK;
}

// ---- landmark elimination: device tables, buffers and BaPlan
int ba_upload(fgo_ctx *c, const VarIndex &V, const Ordering &O, const BaTables &BA) {
  hipStream_t s = c->stream;
  const int n_lm = V.n_lm;
  fgo_ctx::BaSchur &ba = c->ba;
  ba.on = n_lm > 0; ba.n_lm = n_lm;
  BaPlan &B = c->plan.ba;
  std::memset(&B, 0, sizeof(B));
  if (n_lm > 0) {
    const size_t n_obs = BA.obs_edge.size();
    HIPCHK(c, ba.d_lm_var.upload(BA.lm_var, s)); HIPCHK(c, ba.d_pt_ptr.upload(BA.pt_ptr, s)); HIPCHK(c, ba.d_pt_obs.upload(BA.pt_obs, s));
    HIPCHK(c, ba.d_obs_uvw.upload(BA.obs_uvw, s)); HIPCHK(c, ba.d_tgt_list.upload(BA.tgt_list, s));
    HIPCHK(c, ba.d_cam_t0.upload(BA.cam_t0, s)); HIPCHK(c, ba.d_cam_list.upload(BA.cam_list, s));
    // the same measurements in the landmarks' order (k_ba_linearize: one lane per landmark streams its observations instead of
    // gathering 24 bytes from a different cache line each -- the PMC pass showed 1.6 GB of reads for 0.15 GB of data)
    std::vector<double> pt_uvw(3 * n_obs);
    std::vector<int> pt_cam(n_obs);
    parallel_ranges((int)std::min<size_t>(n_obs, (size_t)INT32_MAX), 1 << 16, [&](int q0, int q1) {
      for (int64_t q = q0; q < q1; ++q) {
        const int o = BA.pt_obs[(size_t)q];
        pt_uvw[3 * q] = BA.obs_uvw[3 * (size_t)o]; pt_uvw[3 * q + 1] = BA.obs_uvw[3 * (size_t)o + 1]; pt_uvw[3 * q + 2] = BA.obs_uvw[3 * (size_t)o + 2];
        pt_cam[(size_t)q] = BA.obs_cam[(size_t)o];
      }
    });
    HIPCHK(c, ba.d_pt_uvw.upload(pt_uvw, s)); HIPCHK(c, ba.d_pt_cam.upload(pt_cam, s));
    // ... and the landmarks' unary priors (PriorFactor<Point3>: mean, information in the upper-left 3x3 of the padded block)
    // packed in their order: the generic prior arrays are stored by variable, a gather of nine lines per landmark
    std::vector<int64_t> lp_ptr((size_t)n_lm + 1, 0);
    const int64_t NPall = (int64_t)c->prior_v.size();
    for (int64_t q = 0; q < NPall; ++q) { const int p = V.lm_index[c->prior_v[q]]; if (p >= 0) lp_ptr[(size_t)p + 1]++; }
    for (int p = 0; p < n_lm; ++p) lp_ptr[(size_t)p + 1] += lp_ptr[(size_t)p];
    std::vector<double> lp_val(9 * (size_t)lp_ptr[(size_t)n_lm]);
    {
      std::vector<int64_t> fill(lp_ptr.begin(), lp_ptr.end() - 1);
      for (int64_t q = 0; q < NPall; ++q) {                     // (ascending q: the order of the generic list of the variable)
        const int p = V.lm_index[c->prior_v[q]];
        if (p < 0) continue;
        double *o = &lp_val[9 * (size_t)fill[(size_t)p]++];
        const double *m = &c->prior_mean[(size_t)q * 7], *w = &c->prior_info[(size_t)q * 21];
        o[0] = m[0]; o[1] = m[1]; o[2] = m[2]; o[3] = w[0]; o[4] = w[1]; o[5] = w[2]; o[6] = w[6]; o[7] = w[7]; o[8] = w[11];
      }
    }
    HIPCHK(c, ba.d_lp_ptr.upload(lp_ptr, s)); HIPCHK(c, ba.d_lp_val.upload(lp_val, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, ba.d_obs_cam.upload(BA.obs_cam, s)); HIPCHK(c, ba.d_obs_col.upload(BA.obs_col, s));
    HIPCHK(c, ba.d_obs_lm.upload(BA.obs_lm, s)); HIPCHK(c, ba.d_cam_ptr.upload(BA.cam_ptr, s)); HIPCHK(c, ba.d_cam_col.upload(BA.cam_col, s));
    HIPCHK(c, ba.d_tgt_blk.upload(BA.tgt_blk, s)); HIPCHK(c, ba.d_tgt_ptr.upload(BA.tgt_ptr, s));
    HIPCHK(c, ba.d_op_a.upload(BA.op_a, s)); HIPCHK(c, ba.d_op_b.upload(BA.op_b, s)); HIPCHK(c, ba.d_op_lm.upload(BA.op_lm, s));
    for (int i = 0; i < 2; ++i) {
      HIPCHK(c, ba.d_W[i].alloc(n_obs * 18)); HIPCHK(c, ba.d_Hpp[i].alloc((size_t)n_lm * 6)); HIPCHK(c, ba.d_bp[i].alloc((size_t)n_lm * 3));
      // the observations of fixed cameras (the first o_first) have no coupling block and k_ba_cameras never writes one, but the
      // padding entries of k_ba_schur read block 0 and multiply it by zero: whatever the allocation held must not be a NaN
      if (BA.o_first > 0) HIPCHK(c, hipMemsetAsync(ba.d_W[i].p, 0, sizeof(double) * 18 * (size_t)BA.o_first, s));
    }
    HIPCHK(c, ba.d_Hinv.alloc((size_t)n_lm * 6)); HIPCHK(c, ba.d_zp.alloc((size_t)n_lm * 3)); HIPCHK(c, ba.d_pt_val.alloc((size_t)n_lm * 3));
    HIPCHK(c, ba.d_Hred.alloc((size_t)c->plan.n_hblocks * 36)); HIPCHK(c, ba.d_bred.alloc((size_t)O.nb * 6));
    HIPCHK(c, hipStreamSynchronize(s));                  // the staging vectors die with this function
    HIPCHK(c, ba.d_lm_mine.upload(BA.lm_mine, s));
    HIPCHK(c, hipStreamSynchronize(s));
    B.lm_mine = BA.lm_mine.empty() ? nullptr : ba.d_lm_mine.p;
    B.n_lm = n_lm; B.n_obs = (int64_t)n_obs; B.n_tgt = (int)BA.tgt_blk.size(); B.n_cam = (int)BA.cam_col.size();
    B.lm_var = ba.d_lm_var.p; B.pt_ptr = ba.d_pt_ptr.p; B.pt_obs = ba.d_pt_obs.p; B.obs_uvw = ba.d_obs_uvw.p; B.obs_cam = ba.d_obs_cam.p; B.pt_uvw = ba.d_pt_uvw.p; B.pt_cam = ba.d_pt_cam.p; B.lp_ptr = ba.d_lp_ptr.p; B.lp_val = ba.d_lp_val.p;
    B.o_first = BA.o_first; B.n_tgt_small = BA.n_small; B.tgt_list = ba.d_tgt_list.p; B.n_tgt_list = (int)BA.tgt_list.size();
    B.cam_t0 = ba.d_cam_t0.p; B.cam_list = ba.d_cam_list.p; B.n_cam_list = (int)BA.cam_list.size();
    B.obs_col = ba.d_obs_col.p; B.obs_lm = ba.d_obs_lm.p; B.cam_ptr = ba.d_cam_ptr.p; B.cam_col = ba.d_cam_col.p;
    B.tgt_blk = ba.d_tgt_blk.p; B.tgt_ptr = ba.d_tgt_ptr.p; B.op_a = ba.d_op_a.p; B.op_b = ba.d_op_b.p; B.op_lm = ba.d_op_lm.p;
    B.Hinv = ba.d_Hinv.p; B.zp = ba.d_zp.p; B.pt_val = ba.d_pt_val.p;
    if (c->cfg.verbose)
      std::fprintf(stderr, "[fgo] landmark elimination: %d landmarks, %zu observations, %d reduced blocks with %zu landmark terms\n", n_lm, n_obs,
                   B.n_tgt, BA.op_a.size());
  }
  return FGO_OK;
}

}  // namespace fgo
