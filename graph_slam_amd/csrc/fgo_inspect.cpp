// Read-back, stand-alone solve and the bench hooks of libfgo.
#include "fgo_ctx.hpp"

using namespace fgo;

extern "C" {

int fgo_debug_read_system(fgo_ctx *c, double *H, double *b, double *chi2) try {
  if (!c) return FGO_EINVAL;
  (void)hipSetDevice(c->cfg.device);
  ba_off(c);                                            // the caller wants the whole system: no landmark elimination
  int rc = ensure_ready(c);
  if (rc) return rc;
  if (c->n_phantom > 0) return fail(c, FGO_ESTATE, "fgo_debug_read_system: the structure carries the growth reserve of the incremental mode (fgo_isam2_reset drops it)");
  // linearise WITHOUT the all-reduce so a shard's partial sums can be inspected
  hipStream_t s = c->stream;
  if (c->gtsam_mode) launch_linearize_gtsam(c->plan, c->d_poses[c->cur].p, c->d_H[c->cur].p, c->d_b[c->cur].p, c->d_scal.p + 0, s);
  else launch_linearize(c->plan, c->d_poses[c->cur].p, c->d_H[c->cur].p, c->d_b[c->cur].p, c->d_scal.p + 0, s);
  c->lin_valid = false;
  drop_undamped(c);
  if (H) HIPCHK(c, hipMemcpyAsync(H, c->d_H[c->cur].p, sizeof(double) * 36 * (size_t)c->plan.n_hblocks, hipMemcpyDeviceToHost, s));
  if (b) HIPCHK(c, hipMemcpyAsync(b, c->d_b[c->cur].p, sizeof(double) * 6 * (size_t)c->plan.nb, hipMemcpyDeviceToHost, s));
  if (chi2) HIPCHK(c, hipMemcpyAsync(chi2, c->d_scal.p, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  return FGO_OK;
} FGO_CATCH_INT(c)

// profiling hook: the first n doubles of the reduction scratch (FGO_TRI_PROF stamps of k_panel_tri land there)
int fgo_debug_read_scratch(fgo_ctx *c, double *out, int64_t n) try {
  if (!c || !out || n <= 0 || (size_t)n > c->d_partial.n) return FGO_EINVAL;
  (void)hipSetDevice(c->cfg.device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->d_partial.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  return FGO_OK;
} FGO_CATCH_INT(c)

int fgo_trace(const fgo_ctx *c, double *chi2s, double *lambdas, int cap) {
  if (!c || cap < 0) return FGO_EINVAL;
  const int m = std::min<int>(cap, (int)c->tr_chi2.size());
  if (chi2s) std::memcpy(chi2s, c->tr_chi2.data(), sizeof(double) * m);
  if (lambdas) std::memcpy(lambdas, c->tr_lambda.data(), sizeof(double) * m);
  return m;
}

int fgo_get_stats(const fgo_ctx *c, fgo_stats *st) {
  if (!c || !st) return FGO_EINVAL;
  *st = c->last;
  return FGO_OK;
}

// dense image of a block system in the structure's H layout (diagonal blocks in elimination order, then the oriented
// off-diagonal blocks): rows / columns in free-variable (hessian) order, phantom slots left out
static int dense_from_blocks(fgo_ctx *c, const double *dH, const double *db, double *H_dense, double *b_dense) {
  const int nb = c->plan.nb;
  const int nreal = nb - c->n_phantom;
  if (nreal > 4096) return fail(c, FGO_EINVAL, "dense read-back is limited to 4096 free poses");
  const size_t hblocks = (size_t)nb + (size_t)c->n_offdiag;
  std::vector<double> H(hblocks * 36), b((size_t)nb * 6);
  std::vector<int> asrc((size_t)c->S.nnzL);
  HIPCHK(c, hipMemcpy(H.data(), dH, sizeof(double) * H.size(), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(b.data(), db, sizeof(double) * b.size(), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(asrc.data(), c->d_asrc.p, sizeof(int) * asrc.size(), hipMemcpyDeviceToHost));
  const size_t m = (size_t)nreal * 6;
  if (H_dense) {
    std::memset(H_dense, 0, sizeof(double) * m * m);
    for (int k = 0; k < nb; ++k)
      for (int64_t t = c->S.colptr[k]; t < c->S.colptr[k + 1]; ++t) {
        if (asrc[t] < 0) continue;
        const int hr = c->S.perm[c->S.rowidx[t]], hc = c->S.perm[k];   // hessian (ascending-id) indices
        if (hr >= nreal || hc >= nreal) continue;                       // phantom slot
        const double *B = &H[(size_t)asrc[t] * 36];
        for (int r = 0; r < 6; ++r)
          for (int q = 0; q < 6; ++q) {
            H_dense[((size_t)hr * 6 + r) * m + (size_t)hc * 6 + q] = B[r * 6 + q];
            H_dense[((size_t)hc * 6 + q) * m + (size_t)hr * 6 + r] = B[r * 6 + q];
          }
      }
  }
  if (b_dense)
    for (int k = 0; k < nb; ++k) if (c->S.perm[k] < nreal) std::memcpy(b_dense + (size_t)c->S.perm[k] * 6, &b[(size_t)k * 6], 6 * sizeof(double));
  return FGO_OK;
}

int fgo_linearize(fgo_ctx *c, double *chi2_out, double *H_dense, double *b_dense, int64_t *n_free_out) try {
  if (!c) return FGO_EINVAL;
  (void)hipSetDevice(c->cfg.device);
  if (H_dense || b_dense) ba_off(c);                    // the dense system covers every free variable
  int rc = ensure_ready(c);
  if (rc) return rc;
  rc = linearize_current(c, false);
  if (rc) return rc;
  if (chi2_out) *chi2_out = c->chi_cur;
  // the phantom slots of the incremental mode (the last n_phantom hessian indices) are not the caller's variables: the
  // dense system has 6 * (nb - n_phantom) rows, the phantom rows / columns (identity blocks, zero gradient) are left out.
  // Eliminated landmarks ARE the caller's variables: the count is the same whether or not the dense system is asked for,
  // so the usual query-then-allocate pattern sizes its buffers for the system the second call writes
  if (n_free_out) *n_free_out = (int64_t)c->plan.nb - c->n_phantom + (c->ba.on ? c->ba.n_lm : 0);
  if (!H_dense && !b_dense) return FGO_OK;
  return dense_from_blocks(c, c->d_H[c->cur].p, c->d_b[c->cur].p, H_dense, b_dense);
} FGO_CATCH_INT(c)

// tests: the REDUCED camera system of a structure built with the landmarks eliminated (kernels_ba.hip), i.e.
// S = H_cc - W (H_pp + lambda I)^-1 W^T and g = b_c - W (H_pp + lambda I)^-1 b_p at the current estimate, dense, rows / columns =
// the free non-landmark variables in the order they were added.  lambda enters the landmark blocks only (the cameras' own
// damping is added by the factorisation).  FGO_ESTATE when the context's structure has no eliminated landmarks.
int fgo_debug_read_reduced(fgo_ctx *c, double lambda, double *H_dense, double *b_dense, int64_t *n_out) try {
  if (!c || !(lambda >= 0)) return FGO_EINVAL;
  (void)hipSetDevice(c->cfg.device);
  int rc = ensure_ready(c);
  if (rc) return rc;
  if (!c->ba.on) return fail(c, FGO_ESTATE, "fgo_debug_read_reduced: no landmarks are eliminated in this structure");
  rc = linearize_current(c, false);
  if (rc) return rc;
  if (n_out) *n_out = (int64_t)c->plan.nb - c->n_phantom;
  if (!H_dense && !b_dense) return FGO_OK;
  hipStream_t s = c->stream;
  HIPCHK(c, stage_lambda(c, lambda));
  launch_ba_reduce(c->plan, c->ba.d_W[c->cur].p, c->ba.d_Hpp[c->cur].p, c->ba.d_bp[c->cur].p, c->d_H[c->cur].p, c->d_b[c->cur].p,
                   c->ba.d_Hred.p, c->ba.d_bred.p, c->d_scal.p + 3, c->d_fail.p, s);
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  return dense_from_blocks(c, c->ba.d_Hred.p, c->ba.d_bred.p, H_dense, b_dense);
} FGO_CATCH_INT(c)

// one damped solve, read back in free-variable order.  fused: as an LM trial runs it -- the forward solve riding in the factor sweep
// (launch_factor with b / x: the accumulate, row and leaf kernels carry the right-hand side, k_fwd_combine joins split rows), then the
// backward sweep alone; else the stand-alone forward kernels.  One body, so refusals and phantom slots cannot drift apart.
static int solve_once(fgo_ctx *c, double lambda, double *delta_out, bool fused, const char *who) {
  if (!c || !delta_out) return FGO_EINVAL;
  if (c->shard_world > 1) return fail(c, FGO_ESTATE, (std::string(who) + ": not available in distributed mode").c_str());
  (void)hipSetDevice(c->cfg.device);
  ba_off(c);                                            // delta_out covers every free variable
  int rc = ensure_ready(c);
  if (rc) return rc;
  if (!c->lin_valid) { rc = linearize_current(c, false); if (rc) return rc; }
  hipStream_t s = c->stream;
  claim_L(c);
  HIPCHK(c, stage_lambda(c, lambda));
  launch_factor(c->plan, c->sched, c->d_H[c->cur].p, c->d_L.p, c->d_scal.p + 3, c->d_fail.p, s, fused ? c->d_b[c->cur].p : nullptr, fused ? c->d_x.p : nullptr);
  launch_solve(c->plan, c->sched, c->d_L.p, c->d_b[c->cur].p, c->d_x.p, s, fused);
  const int nb = c->plan.nb;
  std::vector<double> x((size_t)nb * 6);
  HIPCHK(c, hipMemcpyAsync(x.data(), c->d_x.p, sizeof(double) * x.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(c->h_fail, c->d_fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  for (int k = 0; k < nb; ++k)                                     // phantom slots (the last hessian indices) are not reported
    if (c->S.perm[k] < nb - c->n_phantom) std::memcpy(delta_out + (size_t)c->S.perm[k] * 6, &x[(size_t)k * 6], 6 * sizeof(double));
  if (*c->h_fail) return fail(c, FGO_ENUM, "block Cholesky: matrix not positive definite");
  return FGO_OK;
}
int fgo_solve_step(fgo_ctx *c, double lambda, double *delta_out) try { return solve_once(c, lambda, delta_out, false, "fgo_solve_step"); } FGO_CATCH_INT(c)
int fgo_debug_solve_fused(fgo_ctx *c, double lambda, double *delta_out) try { return solve_once(c, lambda, delta_out, true, "fgo_debug_solve_fused"); } FGO_CATCH_INT(c)

// tests: which kernel instantiations one factor + solve of the built structure launches (fused != 0: as an LM trial, else as
// fgo_solve_step).  The launchers themselves are walked with their launches switched off, so the answer cannot drift from them.
int fgo_debug_launch_census(fgo_ctx *c, int fused, int64_t *launches, int64_t *workgroups, int64_t *items, int form_cap, int *level_riders, int *level_long,
                            int level_cap, int *chain2, char *names, int names_cap) try {
  if (!c || form_cap < 0 || level_cap < 0 || names_cap < 0) return FGO_EINVAL;
  if (c->shard_world > 1) return fail(c, FGO_ESTATE, "fgo_debug_launch_census: not available in distributed mode");
  (void)hipSetDevice(c->cfg.device);
  if (fused != 2) ba_off(c);                            // the structure fgo_solve_step / fgo_debug_solve_fused run on
  // fused == 2: the factor sweep as the last fgo_isam2_update ran it -- its dirty flags in the walked plan and, where it was ranged,
  // its PartialSweep -- so the launcher's own range arithmetic answers
  if (fused == 2 && (c->structure_dirty || c->isam.last.sweep == IsamState::Sweep::full || c->isam.col_task.empty()))
    return fail(c, FGO_ESTATE, "fgo_debug_launch_census: the last fgo_isam2_update on this structure was not a partial sweep");
  int rc = ensure_ready(c);
  if (rc) return rc;
  LaunchCensus cz;
  double *const b = c->d_b[c->cur].p, *const x = c->d_x.p;
  // (launch_factor takes "b / x given" as its sign of the fused form: without the buffers the walk would silently be the stand-alone one)
  if (!b || !x) return fail(c, FGO_ESTATE, "fgo_debug_launch_census: the right-hand side / solution buffers are not allocated");
  DevPlan plan = c->plan;
  PartialSweep ps{};
  if (fused == 2) { plan.task_dirty = c->isam.d_task_dirty.p; if (c->isam.last.sweep == IsamState::Sweep::ranged) ps = c->isam.partial_sweep(c->S); }
  launch_factor(plan, c->sched, c->d_H[c->cur].p, c->d_L.p, c->d_scal.p + 3, c->d_fail.p, c->stream, fused ? b : nullptr, fused ? x : nullptr, PHASE_ALL,
                fused == 2 && c->isam.last.sweep == IsamState::Sweep::ranged ? &ps : nullptr, nullptr, &cz);
  launch_solve(c->plan, c->sched, c->d_L.p, b, x, c->stream, fused != 0, PHASE_ALL, nullptr, &cz);
  for (int f = 0; f < std::min<int>(form_cap, LF_COUNT); ++f) {
    if (launches) launches[f] = cz.launches[f];
    if (workgroups) workgroups[f] = cz.workgroups[f];
    if (items) items[f] = cz.items[f];
  }
  for (int l = 0; l < std::min(level_cap, c->sched.n_levels); ++l) {
    if (level_riders) level_riders[l] = cz.level_riders[(size_t)l];
    if (level_long) level_long[l] = cz.level_long[(size_t)l];
  }
  if (chain2) { chain2[0] = cz.chain_on; chain2[1] = cz.chain_mode; }
  if (names && names_cap > 0) {                         // the forms' names, one per line
    std::string all;
    for (int f = 0; f < LF_COUNT; ++f) { all += launch_form_name(f); all += '\n'; }
    if ((int)all.size() + 1 > names_cap) return fail(c, FGO_EINVAL, "fgo_debug_launch_census: names buffer too small");
    std::memcpy(names, all.c_str(), all.size() + 1);
  }
  return LF_COUNT;
} FGO_CATCH_INT(c)

// tests: what the next linearisation of this context launches (see include/fgo.h).  Counts only: nothing is launched, nothing is
// read from the device
int fgo_debug_linearize_census(fgo_ctx *c, int64_t out[12]) try {
  if (!c || !out) return FGO_EINVAL;
  (void)hipSetDevice(c->cfg.device);
  int rc = ensure_ready(c);
  if (rc) return rc;
  const DevPlan &P = c->plan;
  out[0] = P.n_hubs; out[1] = c->n_hub_vars; out[2] = P.n_hub_multi; out[3] = P.hub_deg; out[4] = (int64_t)c->hub_entry_cap;
  out[5] = P.n_dup_groups; out[6] = c->n_dup_members;
  out[7] = P.n_priors; out[8] = c->n_phantom; out[9] = P.imu_ncolor;
  out[10] = c->gtsam_mode && linearize_gtsam_maskable(P) ? 1 : 0;
  out[11] = c->last_phase_rebuilt;
  return FGO_OK;
} FGO_CATCH_INT(c)

// tests: what the last fgo_isam2_update on this context ran (see include/fgo.h)
int fgo_debug_isam_last(fgo_ctx *c, int *info5, int *level_lo, int *level_hi, int *level_ntask, int *level_fwd, int *level_fwtab, int level_cap, int *task_level, unsigned char *task_dirty,
                        unsigned char *task_run, int task_cap, int *var_task, unsigned char *var_chg, double *var_delta, int64_t var_cap) try {
  if (!c || level_cap < 0 || task_cap < 0 || var_cap < 0) return FGO_EINVAL;
  (void)hipSetDevice(c->cfg.device);
  if (c->structure_dirty || c->isam.col_task.empty() || !c->inc.valid || c->isam.n <= 0)
    return fail(c, FGO_ESTATE, "fgo_debug_isam_last: no fgo_isam2_update has run on the current structure");
  const int nl = c->sched.n_levels, ntask = (int)c->S.task_ptr.size() - 1, nb = c->plan.nb;
  const int64_t N = c->isam.n;
  if (info5) { info5[0] = (int)c->isam.last.sweep; info5[1] = c->isam.last.cut ? 1 : 0; info5[2] = nl; info5[3] = ntask; info5[4] = c->sched.bchain_low; }
  const bool ranged = c->isam.last.sweep == IsamState::Sweep::ranged;
  for (int l = 0; l < std::min(level_cap, nl); ++l) {
    if (level_lo) level_lo[l] = ranged ? c->isam.lvl_lo[(size_t)l] : c->sched.level_ptr[l];
    if (level_hi) level_hi[l] = ranged ? c->isam.lvl_hi[(size_t)l] : c->sched.level_ptr[l + 1] - 1;
    if (level_ntask) level_ntask[l] = c->sched.level_ptr[l + 1] - c->sched.level_ptr[l];
  }
  if ((level_fwd || level_fwtab) && level_cap > 0) {    // the launcher's own record of the sweep's forward-role workgroups (nothing is launched)
    LaunchCensus cz;
    DevPlan plan = c->plan;
    PartialSweep ps{};
    if (c->isam.last.sweep != IsamState::Sweep::full) plan.task_dirty = c->isam.d_task_dirty.p;
    if (ranged) ps = c->isam.partial_sweep(c->S);
    launch_factor(plan, c->sched, c->d_H[c->cur].p, c->d_L.p, c->d_scal.p + 3, c->d_fail.p, c->stream, c->d_b[c->cur].p, c->d_x.p, PHASE_ALL,
                  ranged ? &ps : nullptr, nullptr, &cz);
    for (int l = 0; l < std::min(level_cap, nl); ++l) {
      if (level_fwd) level_fwd[l] = cz.level_fwd[(size_t)l];
      if (level_fwtab) level_fwtab[l] = cz.level_fwtab[(size_t)l];
    }
  }
  const int nt = std::min(task_cap, ntask);
  if (task_level) for (int t = 0; t < nt; ++t) task_level[t] = c->isam.task_level[(size_t)t];
  if (task_dirty) {                                     // (a full sweep runs every task)
    std::fill(task_dirty, task_dirty + nt, (unsigned char)(c->isam.last.sweep == IsamState::Sweep::full ? 1 : 0));
    if (c->isam.last.sweep != IsamState::Sweep::full) for (int t : c->isam.last.set.tasks) if (t < nt) task_dirty[t] = 1;
  }
  std::vector<unsigned char> chg;
  if (c->isam.last.cut && (task_run || var_chg)) {
    std::vector<unsigned char> run((size_t)ntask);
    chg.resize((size_t)nb);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(run.data(), c->isam.wild.d_bwd_run.p, (size_t)ntask, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(chg.data(), c->isam.wild.d_chg.p, (size_t)nb, hipMemcpyDeviceToHost));
    // (the levels of the backward chain are always solved and have no run flag)
    if (task_run) for (int t = 0; t < nt; ++t) task_run[t] = c->isam.task_level[(size_t)t] >= c->sched.bchain_low ? 1 : run[(size_t)t];
  } else if (task_run) std::fill(task_run, task_run + nt, (unsigned char)1);
  const int64_t nv = std::min<int64_t>(var_cap, N);
  for (int64_t v = 0; v < nv; ++v) {                    // variables in the order they were added (phantom slots: beyond isam.n)
    const int k = c->inc.pose_col[(size_t)v];
    if (var_task) var_task[v] = k >= 0 ? c->isam.col_task[(size_t)k] : -1;
    if (var_chg) var_chg[v] = (k >= 0 && !chg.empty()) ? chg[(size_t)k] : 0;
  }
  if (var_delta && nv > 0) HIPCHK(c, hipMemcpy(var_delta, c->isam.d_delta.p, sizeof(double) * 6 * (size_t)nv, hipMemcpyDeviceToHost));
  return (int)std::min<int64_t>(N, INT32_MAX);
} FGO_CATCH_INT(c)

int fgo_bench_phase(fgo_ctx *c, int phase, int reps, double *ms_out) try {
  if (!c || reps < 1 || !ms_out || phase < 0 || phase > 2) return FGO_EINVAL;
  if (c->shard_world > 1) return fail(c, FGO_ESTATE, "fgo_bench_phase: not available in distributed mode");
  (void)hipSetDevice(c->cfg.device);
  int rc = ensure_ready(c);
  if (rc) return rc;
  if (!c->lin_valid) { rc = linearize_current(c, true); if (rc) return rc; }
  hipStream_t s = c->stream;
  claim_L(c);
  if (phase >= 1) {   // make sure lambda and (for the solve) a valid factor are in place
    HIPCHK(c, stage_lambda(c, 1e-5 * std::max(1.0, c->h_scal[2])));
    ctx_factor(c, c->cur, true);
  }
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipEventRecord(c->ev[0], s));
  for (int r = 0; r < reps; ++r) {
    if (phase == 0) ctx_linearize(c, c->cur, c->d_scal.p + 0);
    else if (phase == 1) ctx_factor(c, c->cur, true);
    else ctx_solve(c, c->cur, true);   // what a trial runs: backward sweep only
  }
  HIPCHK(c, hipEventRecord(c->ev[1], s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
  *ms_out = (double)ms / reps;
  return FGO_OK;
} FGO_CATCH_INT(c)

}  // extern "C"
