// Marginal covariances (g2o SparseOptimizer::computeMarginals, GTSAM Marginals::marginalCovariance /
// jointMarginalCovariance).  Every request is served by one undamped factorisation of the current linearisation, kept
// resident in d_L (fgo_ctx::L_holds) until the estimate or the structure changes:
//  - chosen diagonal blocks (fgo_marginal_cov, fgo_marginal_cov_many): column solves through that factor;
//  - every diagonal block, and pairs (fgo_marginal_cov_all, fgo_marginal_cov_pairs): blocks of Sigma = H^-1 on the pattern
//    of L by selected inversion (kernels_sinv.hip), recomputed once per factorisation; pairs off that pattern by column solves.
//  - gating of candidate edges (fgo_gate_edges_se3): the same blocks, left on the device and consumed by kernels_gate.hip, which
//    returns the squared Mahalanobis distance of each candidate's innovation; fgo_edge_chi2_se3 is its residual-only form.
//  - gating and association of plane observations (fgo_gate_plane_factors, fgo_associate_planes): the same host steps for a
//    (pose, plane) pair, consumed by kernels_plane_gate.hip.
// The pair tables of the inversion are built on its first request after a structure build (never in the structure phase, so
// neither the symbolic time nor the optimiser's timings move) and kept until the structure is rebuilt.
#include <set>
#include "fgo_ctx.hpp"

using namespace fgo;

namespace {

int host_pose_cols(fgo_ctx *c) {                        // permuted column of every variable (host copy, once per structure)
  if (c->h_pose_col.size() != c->ids.size()) {
    c->h_pose_col.resize(c->ids.size());
    HIPCHK(c, hipMemcpy(c->h_pose_col.data(), c->d_pose_col.p, sizeof(int) * c->h_pose_col.size(), hipMemcpyDeviceToHost));
  }
  return FGO_OK;
}

int common_checks(fgo_ctx *c) {
  (void)hipSetDevice(c->cfg.device);
  if (c->shard_world > 1) return fail(c, FGO_ESTATE, "marginal covariances: not available in distributed mode");
  return ensure_ready(c);
}

// the variables of ids appended to idx
int lookup(fgo_ctx *c, int64_t n, const int64_t *ids, std::vector<int> &idx) {
  for (int64_t q = 0; q < n; ++q) {
    auto it = c->id2idx.find(ids[q]);
    if (it == c->id2idx.end()) return fail(c, FGO_EINVAL, "unknown variable id");
    if (c->fixed[it->second]) return fail(c, FGO_EINVAL, "a fixed vertex has no marginal covariance");
    idx.push_back(it->second);
  }
  return FGO_OK;
}

// every variable of idx (nullptr: of the graph) gets a column of the factor.  With the landmarks eliminated the inverse of the
// reduced system IS the cameras' joint marginal, but an eliminated landmark has no column: asking for one -> generic form
int ensure_columns(fgo_ctx *c, const std::vector<int> *idx) {
  if (!c->ba.on) return FGO_OK;
  bool lm = idx == nullptr;
  if (idx) {
    const int rc = host_pose_cols(c);
    if (rc) return rc;
    for (int v : *idx) lm = lm || c->h_pose_col[v] >= c->plan.nb;
  }
  if (!lm) return FGO_OK;
  ba_off(c);
  return ensure_ready(c);
}

// the undamped factor of the current linearisation in d_L
int undamped_factor(fgo_ctx *c) {
  int rc;
  if (!c->lin_valid && (rc = linearize_current(c, false)) != FGO_OK) return rc;
  if (c->L_holds == LHolds::undamped || c->L_holds == LHolds::undamped_sigma) return FGO_OK;
  hipStream_t s = c->stream;
  claim_L(c);
  HIPCHK(c, stage_lambda(c, 0.0));
  HIPCHK(c, hipEventRecord(c->ev[0], s));
  ctx_factor(c, c->cur, false);
  HIPCHK(c, hipEventRecord(c->ev[1], s));
  HIPCHK(c, hipMemcpyAsync(c->h_fail, c->d_fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (*c->h_fail) return fail(c, FGO_ENUM, "information matrix not positive definite (gauge freedom left?)");
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
  c->sinv.ms_factor = ms;
  record_L(c, LHolds::undamped);
  return FGO_OK;
}

// The six columns of H^-1 at block column cb, one after the other through the undamped factor: after(k) is enqueued behind the
// solve of column 6 cb + k, whose solution d_x then holds.  rhs: 6 nb doubles of scratch.
template <class F>
int solve_block_column(fgo_ctx *c, DevBuf<double> &rhs, int cb, F &&after) {
  hipStream_t s = c->stream;
  const int nb = c->plan.nb;
  for (int k = 0; k < 6; ++k) {
    HIPCHK(c, hipMemsetAsync(rhs.p, 0, sizeof(double) * (size_t)nb * 6, s));
    const double one = 1.0;
    HIPCHK(c, hipMemcpyAsync(rhs.p + 6 * (size_t)cb + k, &one, sizeof(double), hipMemcpyHostToDevice, s));
    launch_solve(c->plan, c->sched, c->d_L.p, rhs.p, c->d_x.p, s);
    after(k);
  }
  return FGO_OK;
}

// Blocks (a, b) of H^-1 through the undamped factor, for the queries q grouped by the column of b (by_b), a's column of every
// query in col_a.  Per column b: six unit right-hand sides, each solved and the rows of the group's a-columns gathered, then one
// copy and one synchronisation.  cov36[q]: rows in a's tangent, columns in b's.
int column_solves(fgo_ctx *c, const std::map<int, std::vector<int64_t>> &by_b, const std::vector<int> &col_a, double *cov36) {
  if (by_b.empty()) return FGO_OK;
  hipStream_t s = c->stream;
  const int nb = c->plan.nb;
  DevBuf<double> rhs, rows;
  DevBuf<int> d_cols;
  HIPCHK(c, rhs.alloc((size_t)nb * 6));
  std::vector<int> cols;
  std::vector<double> h_rows;
  for (const auto &grp : by_b) {
    const int cb = grp.first;
    const std::vector<int64_t> &qs = grp.second;
    const int64_t na = (int64_t)qs.size();
    cols.resize((size_t)na);
    for (int64_t i = 0; i < na; ++i) cols[(size_t)i] = col_a[(size_t)qs[(size_t)i]];
    HIPCHK(c, d_cols.upload(cols, s));
    HIPCHK(c, rows.alloc((size_t)na * 36));
    // column 6 cb + k of H^-1: only the a-columns' rows come back
    const int rc = solve_block_column(c, rhs, cb, [&](int k) { launch_sinv_rows(d_cols.p, na, c->d_x.p, rows.p + (size_t)k * na * 6, s); });
    if (rc) return rc;
    h_rows.resize((size_t)na * 36);
    HIPCHK(c, hipMemcpyAsync(h_rows.data(), rows.p, sizeof(double) * h_rows.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (int64_t i = 0; i < na; ++i)
      for (int k = 0; k < 6; ++k)
        for (int r = 0; r < 6; ++r) cov36[36 * qs[(size_t)i] + r * 6 + k] = h_rows[((size_t)k * na + i) * 6 + r];
  }
  HIPCHK(c, hipGetLastError());
  return FGO_OK;
}

// The same solves with the blocks left on the device: slot t of `blocks` (row-major 6x6) = rows of column row_col[t], columns of
// the group's column.  by_col: slots grouped by the solved column.  No copy, no synchronisation (rhs, d_cols: the caller's scratch).
int column_solves_resident(fgo_ctx *c, const std::map<int, std::vector<int64_t>> &by_col, const std::vector<int> &row_col,
                           DevBuf<double> &rhs, DevBuf<int> &d_cols, double *blocks) {
  if (by_col.empty()) return FGO_OK;
  hipStream_t s = c->stream;
  HIPCHK(c, rhs.alloc((size_t)c->plan.nb * 6));
  HIPCHK(c, d_cols.upload(row_col, s));                            // (slots are numbered group after group: a group is a range)
  for (const auto &grp : by_col) {
    const int64_t t0 = grp.second.front(), nt = (int64_t)grp.second.size();
    const int rc = solve_block_column(c, rhs, grp.first, [&](int k) { launch_sinv_rows(d_cols.p + t0, nt, c->d_x.p, blocks + 36 * t0 + k, s, 36, 6); });
    if (rc) return rc;
  }
  HIPCHK(c, hipGetLastError());
  return FGO_OK;
}

// Pair tables of the recursion: for column j with off-diagonal rows r_0 < ... < r_{m-1}, entry p (p + 1) / 2 + q (q <= p)
// is the block of L at (r_p, r_q) -- the diagonal block of r_p when p == q.  These are the factor's update lists transposed
// (the op L[(r_p, r_q)] -= L[(r_p, j)] L[(r_q, j)]^T becomes a term of both targets (r_p, j) and (r_q, j)), read from the
// column patterns, which hold every pair -- panel interiors included -- while the factor's own op lists are not kept on the
// host after the build.  S_j is a clique of the filled graph, so (r_p, r_q) is always in column r_q's pattern.
int selinv_lists(fgo_ctx *c) {
  const double t0 = now_s();
  const Symbolic &S = c->S;
  const int nb = c->plan.nb;
  std::vector<int64_t> sptr((size_t)nb + 1);
  sptr[0] = 0;
  for (int j = 0; j < nb; ++j) {
    const int64_t m = S.colptr[j + 1] - S.colptr[j] - 1;
    sptr[j + 1] = sptr[j] + m * (m + 1) / 2;
  }
  IntList sidx((size_t)sptr[nb]);
  std::atomic<int> missing{0};
  parallel_ranges(nb, 512, [&](int j0, int j1) {
    for (int j = j0; j < j1; ++j) {
      const int64_t b0 = S.colptr[j] + 1;
      const int m = (int)(S.colptr[j + 1] - b0);
      int *E = sidx.data() + sptr[j];
      for (int q = 0; q < m; ++q) {
        const int rq = S.rowidx[b0 + q];
        E[(int64_t)q * (q + 1) / 2 + q] = (int)S.colptr[rq];
        const int *lo = S.rowidx.data() + S.colptr[rq] + 1, *hi = S.rowidx.data() + S.colptr[rq + 1];
        for (int p = q + 1; p < m; ++p) {
          const int rp = S.rowidx[b0 + p];
          lo = std::lower_bound(lo, hi, rp);
          if (lo == hi || *lo != rp) { missing.store(1); return; }
          E[(int64_t)p * (p + 1) / 2 + q] = (int)(lo - S.rowidx.data());
        }
      }
    }
  });
  if (missing.load()) return fail(c, FGO_EINVAL, "selected inversion: a column pattern is not closed under elimination");
  hipStream_t s = c->stream;
  HIPCHK(c, c->sinv.d_sptr.upload(sptr, s));
  HIPCHK(c, c->sinv.d_sidx.upload(sidx, s));
  HIPCHK(c, hipStreamSynchronize(s));
  c->sinv.lists = true;
  c->sinv.n_entries = sptr[nb];
  c->sinv.list_bytes = (int64_t)(sizeof(int) * sidx.size() + sizeof(int64_t) * sptr.size());
  c->sinv.t_build = now_s() - t0;
  if (c->cfg.verbose)
    std::fprintf(stderr, "[fgo] selected inversion: pair tables %.1f ms, %lld entries (%.1f MB), %lld blocks of L\n", 1e3 * c->sinv.t_build,
                 (long long)c->sinv.n_entries, 1e-6 * (double)c->sinv.list_bytes, (long long)S.nnzL);
  return FGO_OK;
}

// Sigma on the pattern of the undamped factor
int sigma_ready(fgo_ctx *c) {
  int rc = undamped_factor(c);
  if (rc) return rc;
  if (!c->sinv.lists && (rc = selinv_lists(c)) != FGO_OK) return rc;
  if (c->L_holds == LHolds::undamped_sigma) return FGO_OK;
  hipStream_t s = c->stream;
  const size_t nnzL = (size_t)c->S.nnzL;
  HIPCHK(c, c->sinv.d_U.alloc(nnzL * 36));
  HIPCHK(c, c->sinv.d_Sig.alloc(nnzL * 36));
  SinvPlan Q{};
  Q.nb = c->plan.nb;
  Q.colptr = c->d_colptr.p;
  Q.task_ptr = c->d_task_ptr.p;
  Q.task_cols = c->d_task_cols.p;
  Q.sptr = c->sinv.d_sptr.p;
  Q.sidx = c->sinv.d_sidx.p;
  Q.U = c->sinv.d_U.p;
  Q.Sig = c->sinv.d_Sig.p;
  HIPCHK(c, hipEventRecord(c->ev[0], s));
  launch_sinv_prep(Q, c->d_L.p, c->sinv.d_U.p, s);
  HIPCHK(c, hipEventRecord(c->ev[1], s));
  launch_sinv_sweep(Q, c->sched, s);
  HIPCHK(c, hipEventRecord(c->ev[2], s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  float ms_prep = 0, ms_sweep = 0;
  HIPCHK(c, hipEventElapsedTime(&ms_prep, c->ev[0], c->ev[1]));
  HIPCHK(c, hipEventElapsedTime(&ms_sweep, c->ev[1], c->ev[2]));
  c->sinv.d_U.release();                               // only Sigma is read afterwards (and U would hold another nnzL x 288 B)
  c->sinv.ms_prep = ms_prep;
  c->sinv.ms_sweep = ms_sweep;
  record_L(c, LHolds::undamped_sigma);
  if (c->cfg.verbose) {
    const HostSchedule &H = c->sched;
    int n_leaf = 0, n_panel = 0, widest = 0;
    for (int l = 0; l < H.n_levels; ++l) {
      n_leaf += (int)H.level_leaf.size() > l && H.level_leaf[l] ? 1 : 0;
      n_panel += (int)H.level_panel.size() > l && H.level_panel[l] ? 1 : 0;
      widest = std::max(widest, H.level_ptr[l + 1] - H.level_ptr[l]);
    }
    std::fprintf(stderr, "[fgo] selected inversion: prep %.3f ms, sweep %.3f ms; levels %d (leaf %d, panel %d), widest %d tasks\n", ms_prep,
                 ms_sweep, H.n_levels, n_leaf, n_panel, widest);
  }
  return FGO_OK;
}

// Where Cov(a, b) sits in Sigma for the columns ca, cb: block << 1 | transpose, or -1 off the pattern of L.  Block (hi, lo) of
// Sigma holds rows of the later column -- transposed when a is the earlier one
int64_t pattern_code(const Symbolic &S, int ca, int cb) {
  if (ca == cb) return S.colptr[ca] << 1;
  const int lo = std::min(ca, cb), hi = std::max(ca, cb);
  const int *r0 = S.rowidx.data() + S.colptr[lo] + 1, *r1 = S.rowidx.data() + S.colptr[lo + 1];
  const int *t = std::lower_bound(r0, r1, hi);
  if (t == r1 || *t != hi) return -1;
  return ((int64_t)(t - S.rowidx.data()) << 1) | (ca == lo ? 1 : 0);
}

// blocks of Sigma named by enc (block << 1 | transpose) -> out (n x 36)
int selinv_fetch(fgo_ctx *c, const std::vector<int64_t> &enc, double *out) {
  if (enc.empty()) return FGO_OK;
  hipStream_t s = c->stream;
  HIPCHK(c, c->sinv.d_enc.upload(enc, s));
  HIPCHK(c, c->sinv.d_out.alloc(enc.size() * 36));
  launch_sinv_gather(c->sinv.d_enc.p, (int64_t)enc.size(), c->sinv.d_Sig.p, c->sinv.d_out.p, s);
  HIPCHK(c, hipMemcpyAsync(out, c->sinv.d_out.p, sizeof(double) * 36 * enc.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  return FGO_OK;
}

}  // namespace

extern "C" {

// Marginals(graph, values, CHOLESKY).marginalCovariance(key): the (id, id) block of (J' Omega J)^-1 at the current
// linearisation (gtsam/gtsam_graph.cpp:598-601).  The reference pays a full batch factorisation per Marginals object (and
// builds one it never uses at :1357); here the factor stays resident in HBM across calls.
int fgo_marginal_cov(fgo_ctx *c, int64_t id, double *cov36) { return fgo_marginal_cov_many(c, 1, &id, cov36); }

int fgo_marginal_cov_many(fgo_ctx *c, int64_t n, const int64_t *ids, double *cov36) try {
  if (!c || n < 0 || (n > 0 && (!ids || !cov36))) return FGO_EINVAL;
  if (n == 0) return FGO_OK;
  int rc = common_checks(c);
  if (rc) return rc;
  std::vector<int> idx;
  if ((rc = lookup(c, n, ids, idx)) != FGO_OK) return rc;
  if ((rc = ensure_columns(c, &idx)) != FGO_OK) return rc;
  if ((rc = undamped_factor(c)) != FGO_OK) return rc;
  if ((rc = host_pose_cols(c)) != FGO_OK) return rc;
  std::vector<int> col((size_t)n);
  std::map<int, std::vector<int64_t>> by_col;                     // a variable asked for twice is solved for once
  for (int64_t q = 0; q < n; ++q) {
    col[(size_t)q] = c->h_pose_col[idx[(size_t)q]];
    by_col[col[(size_t)q]].push_back(q);
  }
  return column_solves(c, by_col, col, cov36);
} FGO_CATCH_INT(c)

int64_t fgo_marginal_cov_all(fgo_ctx *c, int64_t cap, int64_t *ids_out, double *cov36_out) try {
  if (!c || cap < 0) return FGO_EINVAL;
  int rc = common_checks(c);
  if (rc) return rc;
  int64_t n = 0;
  for (size_t v = 0; v < c->ids.size(); ++v) n += c->fixed[v] ? 0 : 1;
  if (cap == 0 && !ids_out && !cov36_out) return n;
  if (cap < n) return fail(c, FGO_EINVAL, "fgo_marginal_cov_all: cap is smaller than the number of free variables");
  if (!ids_out || !cov36_out) return FGO_EINVAL;
  if ((rc = ensure_columns(c, nullptr)) != FGO_OK) return rc;
  if ((rc = sigma_ready(c)) != FGO_OK) return rc;
  if ((rc = host_pose_cols(c)) != FGO_OK) return rc;
  std::vector<int64_t> enc;
  enc.reserve((size_t)n);
  for (size_t v = 0; v < c->ids.size(); ++v) {
    if (c->fixed[v]) continue;
    ids_out[enc.size()] = c->ids[v];
    enc.push_back(c->S.colptr[c->h_pose_col[v]] << 1);
  }
  if ((rc = selinv_fetch(c, enc, cov36_out)) != FGO_OK) return rc;
  return n;
} FGO_CATCH_INT(c)

int fgo_marginal_cov_pairs(fgo_ctx *c, int64_t n, const int64_t *id_a, const int64_t *id_b, double *cov36) try {
  if (!c || n < 0 || (n > 0 && (!id_a || !id_b || !cov36))) return FGO_EINVAL;
  if (n == 0) return FGO_OK;
  int rc = common_checks(c);
  if (rc) return rc;
  std::vector<int> idx;                                           // a of every pair, then b of every pair
  if ((rc = lookup(c, n, id_a, idx)) != FGO_OK || (rc = lookup(c, n, id_b, idx)) != FGO_OK) return rc;
  if ((rc = ensure_columns(c, &idx)) != FGO_OK) return rc;
  if ((rc = sigma_ready(c)) != FGO_OK) return rc;
  if ((rc = host_pose_cols(c)) != FGO_OK) return rc;
  std::vector<int> col(idx.size());
  for (size_t q = 0; q < idx.size(); ++q) col[q] = c->h_pose_col[idx[q]];
  std::vector<int64_t> enc, on_pat;
  std::map<int, std::vector<int64_t>> by_b;                       // the pairs off the pattern of L, by b's column
  for (int64_t q = 0; q < n; ++q) {
    const int64_t code = pattern_code(c->S, col[(size_t)q], col[(size_t)(n + q)]);
    if (code >= 0) { enc.push_back(code); on_pat.push_back(q); }
    else by_b[col[(size_t)(n + q)]].push_back(q);
  }
  std::vector<double> blk(enc.size() * 36);
  if ((rc = selinv_fetch(c, enc, blk.data())) != FGO_OK) return rc;
  for (size_t k = 0; k < on_pat.size(); ++k) std::memcpy(cov36 + 36 * on_pat[k], &blk[36 * k], 36 * sizeof(double));
  c->sinv.n_fallback = n - (int64_t)on_pat.size();
  return column_solves(c, by_b, col, cov36);
} FGO_CATCH_INT(c)

int fgo_debug_selinv_stats(const fgo_ctx *c, double out[7]) {
  if (!c || !out) return FGO_EINVAL;
  out[0] = c->sinv.t_build;
  out[1] = (double)c->sinv.list_bytes;
  out[2] = c->sinv.ms_factor;
  out[3] = c->sinv.ms_prep;
  out[4] = c->sinv.ms_sweep;
  out[5] = (double)c->sinv.n_entries;
  out[6] = (double)c->sinv.n_fallback;
  return FGO_OK;
}

// tests: what a selected inversion of the built structure launches (see include/fgo.h).  Host tables only; the form of a level
// is asked of sinv_sweep_waves, as launch_sinv_sweep asks it
int fgo_debug_selinv_census(const fgo_ctx *c, int64_t out[16]) {
  if (!c || !out) return FGO_EINVAL;
  if (c->structure_dirty || c->shard_world > 1) return FGO_ESTATE;
  const Symbolic &S = c->S;
  const HostSchedule &H = c->sched;
  std::fill(out, out + 16, (int64_t)0);
  for (int l = H.n_levels - 1; l >= 0; --l) {
    const int t0 = H.level_ptr[l], nt = H.level_ptr[l + 1] - t0;
    if (nt <= 0) continue;
    const int waves = sinv_sweep_waves(nt, H.cus);
    int64_t *o = out + (waves == 16 ? 0 : 6);
    o[0] += 1;
    o[1] += nt;
    for (int t = t0; t < t0 + nt; ++t) {
      const int ncols = S.task_ptr[t + 1] - S.task_ptr[t];
      o[2] += ncols;
      o[5] = std::max<int64_t>(o[5], ncols);
      for (int ci = S.task_ptr[t]; ci < S.task_ptr[t + 1]; ++ci) {
        const int j = S.task_cols[ci];
        const int64_t m = S.colptr[j + 1] - S.colptr[j] - 1;
        o[3] = std::max(o[3], m);
        o[4] += m > waves * SINV_WAVE_GROUPS ? 1 : 0;
      }
    }
  }
  out[12] = S.nb;
  for (int j = 0; j < S.nb; ++j) out[13] += S.colptr[j + 1] - S.colptr[j] == 1 ? 1 : 0;
  out[14] = sinv_prep_workgroups(S.nb);
  out[15] = H.cus;
  return FGO_OK;
}

}  // extern "C"

namespace {

// e, chi2 and (with_cov) d2 / P of n staged candidates in ONE launch, then one copy and one synchronisation.  va / vb: variable of
// either endpoint, rec: GATE_REC doubles per candidate, enc: three covariance codes per candidate (with_cov only).
// out: [n] d2 | [n] chi2 | [n] status | [n][36] P (want_P)
int run_gate(fgo_ctx *c, int64_t n, const std::vector<int> &vab, const std::vector<double> &rec, const std::vector<int64_t> &enc, bool with_cov,
             bool want_P, std::vector<double> &out) {
  hipStream_t s = c->stream;
  fgo_ctx::Gate &G = c->gate;
  HIPCHK(c, G.d_v.upload(vab, s));
  HIPCHK(c, G.d_rec.upload(rec, s));
  if (with_cov) HIPCHK(c, G.d_enc.upload(enc, s));
  out.resize((size_t)n * (want_P ? 39 : 3));
  HIPCHK(c, G.d_out.alloc(out.size()));
  GatePlan A{};
  A.n = n;
  A.va = G.d_v.p; A.vb = G.d_v.p + n;
  A.rec = G.d_rec.p;
  A.enc = G.d_enc.p;
  A.Sig = c->sinv.d_Sig.p; A.extra = G.d_extra.p;
  A.out = G.d_out.p;
  A.want_P = want_P ? 1 : 0;
  HIPCHK(c, hipEventRecord(c->ev[2], s));
  launch_gate(A, c->d_poses[c->cur].p, c->gtsam_mode, with_cov, s);
  HIPCHK(c, hipEventRecord(c->ev[3], s));
  HIPCHK(c, hipMemcpyAsync(out.data(), G.d_out.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
  G.ms_kernel = ms;
  return FGO_OK;
}

// The covariance blocks of n candidates between the variables vab[q] (a) and vab[n + q] (b): enc = three codes per candidate
// (Sigma_aa, Sigma_bb, Sigma_ab; GATE_ZERO for a fixed endpoint), the blocks off the pattern of L solved into gate.d_extra, and the
// gate's figures reset / filled.  with_cov = false: every endpoint is fixed, P = 0 and nothing was factored.  The solves' time is
// between ev[0] and ev[1] when gate.n_groups > 0 (read after the caller's synchronisation).
int gate_blocks(fgo_ctx *c, int64_t n, const std::vector<int> &vab, std::vector<int64_t> &enc, bool &with_cov) {
  int rc;
  std::vector<int> idx;                                           // the free endpoints
  for (int v : vab)
    if (!c->fixed[v]) idx.push_back(v);
  fgo_ctx::Gate &G = c->gate;
  G.n_off = G.n_groups = 0;
  G.ms_solves = 0;
  enc.clear();
  with_cov = !idx.empty();                                        // (every endpoint fixed: P = 0, no factorisation)
  if (!with_cov) return FGO_OK;
  if ((rc = ensure_columns(c, &idx)) != FGO_OK) return rc;
  if ((rc = sigma_ready(c)) != FGO_OK) return rc;
  if ((rc = host_pose_cols(c)) != FGO_OK) return rc;
  const Symbolic &S = c->S;
  enc.assign((size_t)(3 * n), GATE_ZERO);
  std::vector<int64_t> off;                                       // candidates whose Sigma_ab is off the pattern of L
  for (int64_t q = 0; q < n; ++q) {
    const int va = vab[(size_t)q], vb = vab[(size_t)(n + q)];
    const int ca = c->fixed[va] ? -1 : c->h_pose_col[va], cb = c->fixed[vb] ? -1 : c->h_pose_col[vb];
    if (ca >= 0) enc[(size_t)(3 * q)] = S.colptr[ca] << 1;
    if (cb >= 0) enc[(size_t)(3 * q + 1)] = S.colptr[cb] << 1;
    if (ca < 0 || cb < 0) continue;
    const int64_t code = pattern_code(S, ca, cb);
    if (code >= 0) enc[(size_t)(3 * q + 2)] = code; else off.push_back(q);
  }
  if (off.empty()) return FGO_OK;
  // Sigma_ab = Sigma_ba^T: solve for the columns of whichever side has fewer distinct ones among these candidates (many old
  // poses against the newest one: one group, whichever way round the pairs were written)
  std::map<int, std::vector<int64_t>> by_a, by_b;
  for (int64_t q : off) {
    by_a[c->h_pose_col[vab[(size_t)q]]].push_back(q);
    by_b[c->h_pose_col[vab[(size_t)(n + q)]]].push_back(q);
  }
  const bool solve_a = by_a.size() < by_b.size();
  std::map<int, std::vector<int64_t>> by_col;                     // slots of the device buffer, numbered group after group
  std::vector<int> row_col;
  for (const auto &grp : solve_a ? by_a : by_b) {
    std::vector<int64_t> &slots = by_col[grp.first];
    for (int64_t q : grp.second) {
      const int64_t t = (int64_t)row_col.size();
      slots.push_back(t);
      row_col.push_back(c->h_pose_col[vab[(size_t)(solve_a ? n + q : q)]]);
      // solved for b's columns: the slot holds rows a, columns b; for a's: rows b, columns a = Sigma_ab^T
      enc[(size_t)(3 * q + 2)] = gate_extra_code(t, solve_a);
    }
  }
  hipStream_t s = c->stream;
  HIPCHK(c, G.d_extra.alloc(row_col.size() * 36));
  HIPCHK(c, hipEventRecord(c->ev[0], s));
  if ((rc = column_solves_resident(c, by_col, row_col, G.d_rhs, G.d_cols, G.d_extra.p)) != FGO_OK) return rc;
  HIPCHK(c, hipEventRecord(c->ev[1], s));
  G.n_off = (int64_t)off.size();
  G.n_groups = (int64_t)by_col.size();
  return FGO_OK;
}

// the record of one candidate / edge: inverse measurement (unit quaternion), information
void gate_record(const double *meas7, const double *info21, double *rec) {
  const double *q = meas7 + 3;
  const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double z[7] = {meas7[0], meas7[1], meas7[2], q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq};
  pose_inv7(z, rec);
  std::memcpy(rec + 7, info21, 21 * sizeof(double));
}

}  // namespace

extern "C" {

int fgo_gate_edges_se3(fgo_ctx *c, int64_t n, const int64_t *id_a, const int64_t *id_b, const double *meas7, const double *info_ut21,
                       int tangent_order, double *d2_out, double *chi2_out, double *pred_cov36_out) try {
  if (!c || n < 0) return FGO_EINVAL;
  if (n == 0) return FGO_OK;
  if (!id_a || !id_b || !meas7 || !info_ut21 || !d2_out) return FGO_EINVAL;
  if (tangent_order != FGO_TANGENT_G2O && tangent_order != FGO_TANGENT_GTSAM) return fail(c, FGO_EINVAL, "bad tangent order");
  const auto at = [](int64_t q) { return "candidate " + std::to_string(q) + ": "; };
  std::vector<int> vab((size_t)(2 * n));
  for (int64_t q = 0; q < n; ++q) {
    const auto a = c->id2idx.find(id_a[q]), b = c->id2idx.find(id_b[q]);
    if (a == c->id2idx.end() || b == c->id2idx.end()) return fail(c, FGO_EINVAL, at(q) + "unknown variable id");
    if (a->second == b->second) return fail(c, FGO_EINVAL, at(q) + "edge endpoints must differ");
    if (c->var_kind[a->second] != 0 || c->var_kind[b->second] != 0) return fail(c, FGO_EINVAL, at(q) + "SE3 edges connect poses");
    const double *qz = meas7 + 7 * q + 3;
    if (!(qz[0] * qz[0] + qz[1] * qz[1] + qz[2] * qz[2] + qz[3] * qz[3] > 0)) return fail(c, FGO_EINVAL, at(q) + "zero quaternion");
    vab[(size_t)q] = a->second; vab[(size_t)(n + q)] = b->second;
  }
  int rc = common_checks(c);
  if (rc) return rc;
  if ((tangent_order == FGO_TANGENT_GTSAM) != c->gtsam_mode)
    return fail(c, FGO_EINVAL, "candidate edges must use the tangent order of the context's own semantics");
  std::vector<int64_t> enc;
  bool with_cov = false;
  if ((rc = gate_blocks(c, n, vab, enc, with_cov)) != FGO_OK) return rc;
  fgo_ctx::Gate &G = c->gate;
  std::vector<double> rec((size_t)n * GATE_REC), out;
  for (int64_t q = 0; q < n; ++q) gate_record(meas7 + 7 * q, info_ut21 + 21 * q, &rec[(size_t)q * GATE_REC]);
  if ((rc = run_gate(c, n, vab, rec, enc, with_cov, with_cov && pred_cov36_out, out)) != FGO_OK) return rc;
  if (G.n_groups > 0) {
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    G.ms_solves = ms;
  }
  for (int64_t q = 0; q < n; ++q) {
    const double st = out[(size_t)(2 * n + q)];
    if (st == 1.0) return fail(c, FGO_ENUM, at(q) + "information matrix not positive definite");
    if (st != 0.0) return fail(c, FGO_ENUM, at(q) + "innovation covariance not positive definite");
  }
  std::memcpy(d2_out, out.data(), sizeof(double) * (size_t)n);
  if (chi2_out) std::memcpy(chi2_out, out.data() + n, sizeof(double) * (size_t)n);
  if (pred_cov36_out) {
    if (with_cov) std::memcpy(pred_cov36_out, out.data() + 3 * n, sizeof(double) * 36 * (size_t)n);
    else std::memset(pred_cov36_out, 0, sizeof(double) * 36 * (size_t)n);
  }
  return FGO_OK;
} FGO_CATCH_INT(c)

int fgo_edge_chi2_se3(fgo_ctx *c, int64_t first, int64_t n, double *chi2_out) try {
  if (!c || first < 0 || n < 0 || (n > 0 && !chi2_out)) return FGO_EINVAL;
  std::vector<int64_t> edges;                                     // the SE3 edges [first, first + n) of the store
  int64_t k = 0;
  for (size_t e = 0; e < c->torder.size() && (int64_t)edges.size() < n; ++e) {
    if (c->torder[e] > FGO_TANGENT_GTSAM) continue;
    if (k++ >= first) edges.push_back((int64_t)e);
  }
  if ((int64_t)edges.size() < n) return fail(c, FGO_EINVAL, "fgo_edge_chi2_se3: the graph has fewer SE3 edges than first + n");
  if (n == 0) return FGO_OK;
  const int rc = common_checks(c);
  if (rc) return rc;
  std::vector<int> vab((size_t)(2 * n));
  std::vector<double> rec((size_t)n * GATE_REC), out;
  for (int64_t q = 0; q < n; ++q) {
    const size_t e = (size_t)edges[(size_t)q];
    vab[(size_t)q] = c->ei[e]; vab[(size_t)(n + q)] = c->ej[e];
    gate_record(&c->meas[e * 7], &c->info[e * 21], &rec[(size_t)q * GATE_REC]);
  }
  const int rg = run_gate(c, n, vab, rec, std::vector<int64_t>(), false, false, out);
  if (rg) return rg;
  std::memcpy(chi2_out, out.data() + n, sizeof(double) * (size_t)n);
  return FGO_OK;
} FGO_CATCH_INT(c)

int fgo_debug_gate_stats(const fgo_ctx *c, double out[4]) {
  if (!c || !out) return FGO_EINVAL;
  out[0] = (double)c->gate.n_off;
  out[1] = (double)c->gate.n_groups;
  out[2] = c->gate.ms_kernel;
  out[3] = c->gate.ms_solves;
  return FGO_OK;
}

}  // extern "C"

namespace {

// one candidate plane observation: pose and plane variable, record.  Checks follow fgo_add_plane_factor (same normalisation of z)
int plane_gate_stage(fgo_ctx *c, const std::string &at, int64_t pose_id, int64_t plane_id, const double *z, const double *cov6, int &vx, int &vp,
                     double *rec) {
  const auto x = c->id2idx.find(pose_id), p = c->id2idx.find(plane_id);
  if (x == c->id2idx.end() || p == c->id2idx.end()) return fail(c, FGO_EINVAL, at + "unknown variable id");
  if (c->var_kind[x->second] != 0) return fail(c, FGO_EINVAL, at + "the first variable of a plane observation is a pose");
  if (c->var_kind[p->second] != 1) return fail(c, FGO_EINVAL, at + "the second variable of a plane observation is a plane");
  vx = x->second; vp = p->second;
  if (!z) return FGO_OK;
  const double n = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
  if (!(n > 0)) return fail(c, FGO_EINVAL, at + "zero plane normal");
  rec[0] = z[0] / n; rec[1] = z[1] / n; rec[2] = z[2] / n; rec[3] = z[3];
  std::memcpy(rec + 4, cov6, 6 * sizeof(double));
  return FGO_OK;
}

// the plane gate's single launch over n staged candidates (vxp: pose variable of every candidate, then plane variable); the output
// stays in gate.d_out.  Timed between ev[2] and the caller's ev[3]
int launch_plane_request(fgo_ctx *c, int64_t n, const std::vector<int> &vxp, const std::vector<double> &rec, const std::vector<int64_t> &enc, bool want_P) {
  hipStream_t s = c->stream;
  fgo_ctx::Gate &G = c->gate;
  HIPCHK(c, G.d_v.upload(vxp, s));
  HIPCHK(c, G.d_rec.upload(rec, s));
  HIPCHK(c, G.d_enc.upload(enc, s));
  HIPCHK(c, G.d_out.alloc((size_t)n * (want_P ? 16 : 7)));
  PlaneGatePlan A{};
  A.n = n;
  A.vx = G.d_v.p; A.vp = G.d_v.p + n;
  A.rec = G.d_rec.p;
  A.enc = G.d_enc.p;
  A.Sig = c->sinv.d_Sig.p; A.extra = G.d_extra.p;
  A.out = G.d_out.p;
  A.want_P = want_P ? 1 : 0;
  HIPCHK(c, hipEventRecord(c->ev[2], s));
  launch_plane_gate(A, c->d_poses[c->cur].p, s);
  return FGO_OK;
}

// after the request's synchronisation: the device times of its kernels and of the column solves
int plane_gate_times(fgo_ctx *c) {
  fgo_ctx::Gate &G = c->gate;
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
  G.ms_kernel = ms;
  if (G.n_groups > 0) {
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    G.ms_solves = ms;
  }
  return FGO_OK;
}

int plane_gate_checks(fgo_ctx *c) {
  const int rc = common_checks(c);
  if (rc) return rc;
  if (!c->gtsam_mode) return fail(c, FGO_EINVAL, "plane observations need a GTSAM-semantics context");
  return FGO_OK;
}

}  // namespace

extern "C" {

int fgo_gate_plane_factors(fgo_ctx *c, int64_t n, const int64_t *pose_id, const int64_t *plane_id, const double *z_abcd, const double *cov_ut6,
                           double *d2_out, double *chi2_out, double *cos_out, double *resid3_out, double *pred_cov9_out) try {
  if (!c || n < 0) return FGO_EINVAL;
  if (n == 0) return FGO_OK;
  if (!pose_id || !plane_id || !z_abcd || !cov_ut6 || !d2_out) return FGO_EINVAL;
  const auto at = [](int64_t q) { return "candidate " + std::to_string(q) + ": "; };
  std::vector<int> vxp((size_t)(2 * n));
  std::vector<double> rec((size_t)n * PGATE_REC);
  int rc;
  for (int64_t q = 0; q < n; ++q)
    if ((rc = plane_gate_stage(c, at(q), pose_id[q], plane_id[q], z_abcd + 4 * q, cov_ut6 + 6 * q, vxp[(size_t)q], vxp[(size_t)(n + q)],
                               &rec[(size_t)q * PGATE_REC])) != FGO_OK)
      return rc;
  if ((rc = plane_gate_checks(c)) != FGO_OK) return rc;
  std::vector<int64_t> enc;
  bool with_cov = false;
  if ((rc = gate_blocks(c, n, vxp, enc, with_cov)) != FGO_OK) return rc;
  if (!with_cov) enc.assign((size_t)(3 * n), GATE_ZERO);
  const bool want_P = pred_cov9_out != nullptr;
  if ((rc = launch_plane_request(c, n, vxp, rec, enc, want_P)) != FGO_OK) return rc;
  hipStream_t s = c->stream;
  std::vector<double> out((size_t)n * (want_P ? 16 : 7));
  HIPCHK(c, hipEventRecord(c->ev[3], s));
  HIPCHK(c, hipMemcpyAsync(out.data(), c->gate.d_out.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  if ((rc = plane_gate_times(c)) != FGO_OK) return rc;
  for (int64_t q = 0; q < n; ++q) {
    const double st = out[(size_t)(3 * n + q)];
    if (st == 1.0) return fail(c, FGO_ENUM, at(q) + "measurement covariance not positive definite");
    if (st != 0.0) return fail(c, FGO_ENUM, at(q) + "innovation covariance not positive definite");
  }
  std::memcpy(d2_out, out.data(), sizeof(double) * (size_t)n);
  if (chi2_out) std::memcpy(chi2_out, out.data() + n, sizeof(double) * (size_t)n);
  if (cos_out) std::memcpy(cos_out, out.data() + 2 * n, sizeof(double) * (size_t)n);
  if (resid3_out) std::memcpy(resid3_out, out.data() + 4 * n, sizeof(double) * 3 * (size_t)n);
  if (pred_cov9_out) std::memcpy(pred_cov9_out, out.data() + 7 * n, sizeof(double) * 9 * (size_t)n);
  return FGO_OK;
} FGO_CATCH_INT(c)

int fgo_associate_planes(fgo_ctx *c, int64_t pose_id, int64_t k, const double *z_abcd, const double *cov_ut6, int64_t m, const int64_t *plane_ids,
                         double d2_gate, double cos_min, int64_t *match_out, double *best2_out, double *d2_matrix_out) try {
  if (!c || k < 0 || m < 0) return FGO_EINVAL;
  if (k == 0) return FGO_OK;
  if (!z_abcd || !cov_ut6 || !match_out || !best2_out || (m > 0 && !plane_ids)) return FGO_EINVAL;
  if (m == 0) {
    for (int64_t i = 0; i < k; ++i) { match_out[i] = -1; best2_out[2 * i] = best2_out[2 * i + 1] = HUGE_VAL; }
    return FGO_OK;
  }
  // the m pairs (pose, plane j) first: the k observations of a pair share its three covariance blocks
  std::vector<int> pair_v((size_t)(2 * m));
  std::set<int64_t> seen;
  int rc;
  for (int64_t j = 0; j < m; ++j) {
    const std::string at = "plane " + std::to_string(j) + ": ";
    if ((rc = plane_gate_stage(c, at, pose_id, plane_ids[j], nullptr, nullptr, pair_v[(size_t)j], pair_v[(size_t)(m + j)], nullptr)) != FGO_OK) return rc;
    if (!seen.insert(plane_ids[j]).second) return fail(c, FGO_EINVAL, at + "listed twice");
  }
  const int64_t n = k * m;
  std::vector<double> rec((size_t)n * PGATE_REC);
  for (int64_t i = 0; i < k; ++i) {                                // candidate j k + i = observation i against plane j
    int vx, vp;
    double *r0 = &rec[(size_t)i * PGATE_REC];
    if ((rc = plane_gate_stage(c, "observation " + std::to_string(i) + ": ", pose_id, plane_ids[0], z_abcd + 4 * i, cov_ut6 + 6 * i, vx, vp, r0)) != FGO_OK)
      return rc;
    for (int64_t j = 1; j < m; ++j) std::memcpy(&rec[(size_t)(j * k + i) * PGATE_REC], r0, PGATE_REC * sizeof(double));
  }
  if ((rc = plane_gate_checks(c)) != FGO_OK) return rc;
  std::vector<int64_t> pair_enc;
  bool with_cov = false;
  if ((rc = gate_blocks(c, m, pair_v, pair_enc, with_cov)) != FGO_OK) return rc;
  if (!with_cov) pair_enc.assign((size_t)(3 * m), GATE_ZERO);
  fgo_ctx::Gate &G = c->gate;
  G.n_off *= k;                                                    // (candidates, not pairs)
  std::vector<int> vxp((size_t)(2 * n));
  std::vector<int64_t> enc((size_t)(3 * n));
  for (int64_t j = 0; j < m; ++j)
    for (int64_t i = 0; i < k; ++i) {
      const int64_t q = j * k + i;
      vxp[(size_t)q] = pair_v[(size_t)j]; vxp[(size_t)(n + q)] = pair_v[(size_t)(m + j)];
      for (int t = 0; t < 3; ++t) enc[(size_t)(3 * q + t)] = pair_enc[(size_t)(3 * j + t)];
    }
  if ((rc = launch_plane_request(c, n, vxp, rec, enc, false)) != FGO_OK) return rc;
  hipStream_t s = c->stream;
  const bool want_matrix = d2_matrix_out != nullptr;
  std::vector<double> res((size_t)(3 * k + (want_matrix ? n : 0)));
  HIPCHK(c, G.d_res.alloc(res.size()));
  launch_plane_assoc(G.d_out.p, k, m, d2_gate, cos_min, want_matrix, G.d_res.p, s);
  HIPCHK(c, hipEventRecord(c->ev[3], s));
  HIPCHK(c, hipMemcpyAsync(res.data(), G.d_res.p, sizeof(double) * res.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  if ((rc = plane_gate_times(c)) != FGO_OK) return rc;
  for (int64_t i = 0; i < k; ++i) match_out[i] = res[(size_t)i] < 0 ? -1 : plane_ids[(int64_t)res[(size_t)i]];
  std::memcpy(best2_out, res.data() + k, sizeof(double) * 2 * (size_t)k);
  if (want_matrix) std::memcpy(d2_matrix_out, res.data() + 3 * k, sizeof(double) * (size_t)n);
  return FGO_OK;
} FGO_CATCH_INT(c)

}  // extern "C"
