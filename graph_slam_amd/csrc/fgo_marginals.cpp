// Marginal covariances (g2o SparseOptimizer::computeMarginals, GTSAM Marginals::marginalCovariance /
// jointMarginalCovariance).  Every request is served by one undamped factorisation of the current linearisation, kept
// resident in d_L (fgo_ctx::L_holds) until the estimate or the structure changes:
//  - chosen diagonal blocks (fgo_marginal_cov, fgo_marginal_cov_many): column solves through that factor;
//  - every diagonal block, and pairs (fgo_marginal_cov_all, fgo_marginal_cov_pairs): blocks of Sigma = H^-1 on the pattern
//    of L by selected inversion (kernels_sinv.hip), recomputed once per factorisation; pairs off that pattern by column solves.
// The pair tables of the inversion are built on its first request after a structure build (never in the structure phase, so
// neither the symbolic time nor the optimiser's timings move) and kept until the structure is rebuilt.
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
    for (int k = 0; k < 6; ++k) {                              // column 6 cb + k of H^-1: only the a-columns' rows come back
      HIPCHK(c, hipMemsetAsync(rhs.p, 0, sizeof(double) * (size_t)nb * 6, s));
      const double one = 1.0;
      HIPCHK(c, hipMemcpyAsync(rhs.p + 6 * (size_t)cb + k, &one, sizeof(double), hipMemcpyHostToDevice, s));
      launch_solve(c->plan, c->sched, c->d_L.p, rhs.p, c->d_x.p, s);
      launch_sinv_rows(d_cols.p, na, c->d_x.p, rows.p + (size_t)k * na * 6, s);
    }
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
  const Symbolic &S = c->S;
  // pairs on the pattern of L: block (hi, lo) of Sigma holds rows of the later column -- transposed when a is the earlier one
  std::vector<int64_t> enc, on_pat;
  std::map<int, std::vector<int64_t>> by_b;                       // the others, by b's column
  for (int64_t q = 0; q < n; ++q) {
    const int ca = col[(size_t)q], cb = col[(size_t)(n + q)];
    if (ca == cb) { enc.push_back(S.colptr[ca] << 1); on_pat.push_back(q); continue; }
    const int lo = std::min(ca, cb), hi = std::max(ca, cb);
    const int *r0 = S.rowidx.data() + S.colptr[lo] + 1, *r1 = S.rowidx.data() + S.colptr[lo + 1];
    const int *t = std::lower_bound(r0, r1, hi);
    if (t != r1 && *t == hi) {
      enc.push_back(((int64_t)(t - S.rowidx.data()) << 1) | (ca == lo ? 1 : 0));
      on_pat.push_back(q);
    } else {
      by_b[cb].push_back(q);
    }
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

}  // extern "C"
