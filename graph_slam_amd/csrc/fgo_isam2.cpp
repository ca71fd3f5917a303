// ISAM2 semantics on the batch machinery (fgo_isam2_*).
#include "fgo_ctx.hpp"

using namespace fgo;

namespace {

using Sweep = IsamState::Sweep;

// Which forms an update runs (choose_forms); every later step reads this.
struct Forms {
  bool have_tables;    // the structure carries the partial-sweep tables: this update leaves L, y and the flags behind for the next
  bool partial;        // ... and L / y are the previous update's: only the tasks above the affected variables run again
  bool look;           // which variables the relinearisation moves came to the host with the previous update's last synchronisation
  bool maskable;       // the masked linearisation kernel serves this graph
  bool masked;         // ... and H / b of the previous update are in place: only the affected variables are gathered again
  bool prev_solution;  // the previous update left its solution behind (wildfire)
};

// Switches the context to the incremental, generic form and builds what is stale.  ISAM2 keeps theta / delta for EVERY variable
// and factors H as linearised: a structure built with the landmarks eliminated (fgo_optimize_gtsam ran first, or
// FGO_ISAM_INCREMENTAL=0) cannot serve it -> generic form from here on, until fgo_isam2_reset.  A call that fails (build error,
// g2o-semantics graph) leaves the context as it found it.  was_dirty: a structure phase ran.
int enter(fgo_ctx *c, bool &was_dirty) {
  // a context that is updated incrementally builds its structure with room to grow (phantom variable slots + factor
  // capacity), so that the per-record updates of the reference's drivers do not pay the structure phase every time
  const bool incr_off = std::getenv("FGO_ISAM_INCREMENTAL") && std::atoi(std::getenv("FGO_ISAM_INCREMENTAL")) == 0;
  const bool incr_was = c->isam_incremental;            // (captured BEFORE the switch below: the failure path restores it)
  if (!incr_off) c->isam_incremental = true;
  const bool ba_was_disabled = c->ba_disable;
  ba_off(c);
  was_dirty = c->structure_dirty;
  int rc = ensure_ready(c);
  if (rc == FGO_OK && !c->gtsam_mode) rc = fail(c, FGO_EINVAL, "g2o-semantics graph: ISAM2 semantics need a GTSAM-semantics graph");
  if (rc) {
    if (!ba_was_disabled) { c->ba_disable = false; c->structure_dirty = true; }   // (the next build decides again)
    if (c->isam_incremental != incr_was) { c->isam_incremental = incr_was; c->structure_dirty = true; }   // (a structure built with the reserve is not the batch one)
  }
  return rc;
}

// theta / delta sized to the structure's NX slots (covered variables keep theirs) and covering all N variables of the graph
int fit_state(fgo_ctx *c, int64_t NX, int64_t N) {
  IsamState &I = c->isam;
  hipStream_t s = c->stream;
  if (I.d_theta.n != (size_t)NX * 8) {
    DevBuf<double> th, de;
    HIPCHK(c, th.alloc((size_t)NX * 8));
    HIPCHK(c, de.alloc((size_t)NX * 6));
    HIPCHK(c, hipMemsetAsync(th.p, 0, sizeof(double) * (size_t)NX * 8, s));
    HIPCHK(c, hipMemsetAsync(de.p, 0, sizeof(double) * (size_t)NX * 6, s));
    if (I.n > 0) {
      HIPCHK(c, hipMemcpyAsync(th.p, I.d_theta.p, sizeof(double) * (size_t)I.n * 8, hipMemcpyDeviceToDevice, s));
      HIPCHK(c, hipMemcpyAsync(de.p, I.d_delta.p, sizeof(double) * (size_t)I.n * 6, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));
    I.d_theta.swap(th);
    I.d_delta.swap(de);
  }
  if (I.n < N) {                                        // newTheta: new variables enter at their initial value, delta = 0
    HIPCHK(c, hipMemcpyAsync(I.d_theta.p + (size_t)I.n * 8, c->d_poses[c->cur].p + (size_t)I.n * 8,
                             sizeof(double) * (size_t)(N - I.n) * 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(c, hipMemsetAsync(I.d_delta.p + (size_t)I.n * 6, 0, sizeof(double) * (size_t)(N - I.n) * 6, s));
    I.n = N;
  }
  return FGO_OK;
}

// Reads what the previous update carried over, and consumes it: this update sets it again when it succeeds (finish).
// ---- partial re-factorisation.  ISAM2 re-eliminates only the cliques on the paths from the affected variables to the
// root of the Bayes tree; here: only the TASKS of the elimination tree on those paths are run again (k_* kernels skip
// the others), every other column keeps its blocks of L and its entry of the forward solution y from the previous
// step (isam_dirty.cpp).
// FGO_ISAM_PARTIAL=0 switches it off (A/B measurements).  Measured, one new pose per update on a settled graph (1xMI355X,
// tools/isam_build_breakdown.py): 2 000 poses 1.30 vs 1.35 ms, 20 000 poses 2.13 vs 2.37 ms, 100 000 poses 3.30 vs 5.01 ms
// device per update -- ~25-30 of 200 / 1 750 / 8 600 tasks are re-run; what remains is one latency-bound pivot chain per level
// of the path, which is why the gain grows with the graph.
Forms choose_forms(fgo_ctx *c, double relin_threshold) {
  IsamState &I = c->isam;
  const char *pe = std::getenv("FGO_ISAM_PARTIAL");
  const bool partial_on = !(pe && std::atoi(pe) == 0);
  static const bool look_on = tune("isam_lookahead", 1) != 0;
  static const bool mask_on = tune("isam_masked", 1) != 0;
  Forms f{};
  f.have_tables = !I.col_task.empty() && c->inc.valid && I.d_y.p != nullptr;
  f.partial = partial_on && f.have_tables && c->L_holds == LHolds::isam_step;
  // which variables k_isam2_relin moves is known since the END of the previous update (same delta, same test: k_isam2_estimate)
  // unless the threshold or the structure changed in between -- then the flags come back here, at the price of a synchronisation
  f.look = look_on && f.partial && (I.carry & IsamState::CARRY_LOOK) && I.look_thr == relin_threshold && I.look_nx == c->plan.n_poses;
  f.maskable = mask_on && f.have_tables && I.d_chi_var.p != nullptr && linearize_gtsam_maskable(c->plan);
  f.masked = f.maskable && f.partial && (I.carry & IsamState::CARRY_H);
  f.prev_solution = (I.carry & IsamState::CARRY_SOLUTION) != 0;
  I.invalidate_carry();
  return f;
}

// theta <- theta (+) delta where delta crossed the threshold (count: scal[5]); without look-ahead flags the flags of what moved
// start their way to the host (ev[5])
int enqueue_relin(fgo_ctx *c, const Forms &f, double relin_threshold) {
  IsamState &I = c->isam;
  const bool fetch = f.partial && !f.look;
  launch_isam2_relin(c->plan, I.d_theta.p, I.d_delta.p, relin_threshold, c->d_scal.p + 5, c->stream, fetch ? I.d_moved.p : nullptr);
  if (fetch) {
    HIPCHK(c, hipMemcpyAsync(I.flags.moved, I.d_moved.p, (size_t)c->plan.n_poses, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
  }
  return FGO_OK;
}

// H / b of the side buffers and chi2 (scal[4]) at theta.  The masked form gathers only the factors of flags.affected again, so it
// comes after the host walk; the full form does not read the flags.  Ends the "linearise" interval (ev[1]).
int enqueue_linearize(fgo_ctx *c, const Forms &f) {
  const int w = c->cur ^ 1;                             // the side buffers: the current ones stay valid for the values
  unsigned char *mask = f.masked ? c->isam.d_lin_mask.p : nullptr;
  if (mask) HIPCHK(c, hipMemcpyAsync(mask, c->isam.flags.affected, (size_t)c->plan.n_poses, hipMemcpyHostToDevice, c->stream));
  if (f.maskable) launch_linearize_gtsam_masked(c->plan, c->isam.d_theta.p, c->d_H[w].p, c->d_b[w].p, c->d_scal.p + 4, c->stream, mask, c->isam.d_chi_var.p);
  else launch_linearize_gtsam(c->plan, c->isam.d_theta.p, c->d_H[w].p, c->d_b[w].p, c->d_scal.p + 4, c->stream);
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  return FGO_OK;
}

// The host walk of a partial update (isam_dirty.cpp): flags.affected / task_dirty / col_dirty and last.set of this update, the
// number of dirty tasks (-2: too many, full sweep), and where the sweep stays partial the dirty flags on their way to the device
// and plan.task_dirty set.  `seen`: what the previous update already knew.
int affected_tasks(fgo_ctx *c, const Forms &f, const IsamAdded &seen, DevPlan &plan, int64_t &n_dirty_tasks) {
  IsamState &I = c->isam;
  const IsamFlags &F = I.flags;
  const IsamGraph G{(int64_t)c->ids.size(), c->ei, c->ej, c->imu_ids, c->prior_v, c->inc.he_ptr, c->inc.he, c->inc.imu_inc_ptr, c->inc.imu_inc,
                    c->inc.pose_col, c->S.parent, I.col_task, c->S.task_ptr, c->S.task_cols};
  isam_mark_added(F, G, seen, I.last.set);              // (overlaps the copy of `moved`)
  if (!f.look) HIPCHK(c, hipEventSynchronize(c->ev[5]));
  static const double full_frac = tune("isam_full_frac", 0.3);
  n_dirty_tasks = isam_dirty_tasks(F, f.look ? F.moved_next : F.moved, G, I.last.set, full_frac);
  if (n_dirty_tasks >= 0) {
    HIPCHK(c, hipMemcpyAsync(I.d_task_dirty.p, F.task_dirty, c->S.task_ptr.size() - 1, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(I.d_col_dirty.p, F.col_dirty, (size_t)c->plan.nb, hipMemcpyHostToDevice, c->stream));
    // (pinned staging: no synchronisation needed; the buffers are not touched again before the stream is drained in finish)
    plan.task_dirty = I.d_task_dirty.p;
  }
  return FGO_OK;
}

// The factor sweep with the forward solve fused in -- full, masked by plan.task_dirty, or ranged over the levels' dirty tasks --
// and y kept for the next update.  Ends the "factor" interval (ev[2]).
int enqueue_sweep(fgo_ctx *c, const Forms &f, const DevPlan &plan) {
  IsamState &I = c->isam;
  hipStream_t s = c->stream;
  const int w = c->cur ^ 1;
  claim_L(c);
  if (plan.task_dirty) launch_mix_rhs(plan, c->d_b[w].p, I.d_y.p, c->d_x.p, I.d_col_dirty.p, s);
  PartialSweep ps{};
  const bool ranged = plan.task_dirty && I.tk_ok && !I.task_level.empty();
  if (ranged) {                                         // per level: the tasks that cover its dirty ones
    std::fill(I.lvl_lo.begin(), I.lvl_lo.end(), INT32_MAX);
    std::fill(I.lvl_hi.begin(), I.lvl_hi.end(), -1);
    for (int t : I.last.set.tasks) { const size_t l = (size_t)I.task_level[(size_t)t]; I.lvl_lo[l] = std::min(I.lvl_lo[l], t); I.lvl_hi[l] = std::max(I.lvl_hi[l], t); }
    if (std::getenv("FGO_ISAM_DEBUG")) {
      std::fprintf(stderr, "[isam] ranged sweep: %zu dirty tasks;", I.last.set.tasks.size());
      for (int l = 0; l < c->sched.n_levels; ++l) std::fprintf(stderr, " %d/%d", I.lvl_hi[(size_t)l] < I.lvl_lo[(size_t)l] ? 0 : I.lvl_hi[(size_t)l] - I.lvl_lo[(size_t)l] + 1, c->sched.level_ptr[l + 1] - c->sched.level_ptr[l]);
      std::fprintf(stderr, "\n");
    }
    ps = I.partial_sweep(c->S);
  }
  I.last.sweep = !plan.task_dirty ? Sweep::full : ranged ? Sweep::ranged : Sweep::masked;
  launch_factor(plan, c->sched, c->d_H[w].p, c->d_L.p, c->d_scal.p + 3, c->d_fail.p, s, c->d_b[w].p, c->d_x.p, PHASE_ALL, ranged ? &ps : nullptr);
  if (f.have_tables) launch_copy_vec(c->d_x.p, I.d_y.p, (int64_t)c->plan.nb * 6, s);       // y for the next step
  HIPCHK(c, hipEventRecord(c->ev[2], s));
  return FGO_OK;
}

// The backward solve, cut by the wildfire threshold where that applies, and its solution kept for the next update's cut.
// wild_possible: a cut can apply on this structure at all.  Ends the "solve" interval (ev[3]).
int enqueue_solve(fgo_ctx *c, const Forms &f, const DevPlan &plan, bool &wild_possible) {
  IsamState &I = c->isam;
  hipStream_t s = c->stream;
  const int w = c->cur ^ 1;
  // wildfire option: below the backward chain only what was re-factored or reads a delta that moved by >= the threshold
  Wildfire wf{I.wild.d_bwd_run.p, I.wild.d_chg.p, I.d_task_dirty.p, I.wild.d_xprev.p, I.wild.thr};
  const bool wild = I.wild.thr > 0 && plan.task_dirty && f.prev_solution && I.wild.d_xprev.p != nullptr && c->sched.bchain_low >= 0;
  launch_solve(c->plan, c->sched, c->d_L.p, c->d_b[w].p, c->d_x.p, s, true, PHASE_ALL, wild ? &wf : nullptr);
  // (the copy of this solution is what the NEXT update's cut compares against: only kept where a cut can apply at all)
  wild_possible = I.wild.thr > 0 && f.have_tables && I.wild.d_xprev.p && c->sched.bchain_low >= 0;
  if (wild_possible) launch_copy_vec(c->d_x.p, I.wild.d_xprev.p, (int64_t)c->plan.nb * 6, s);
  I.last.cut = wild;
  if (std::getenv("FGO_ISAM_DEBUG"))
    std::fprintf(stderr, "[isam] wildfire: thr %g, partial %d, solution of the previous update kept %d, backward chain from level %d (%d panels) -> cut %d\n",
                 I.wild.thr, plan.task_dirty != nullptr, (int)f.prev_solution, c->sched.bchain_low, c->sched.bchain_n, (int)wild);
  HIPCHK(c, hipEventRecord(c->ev[3], s));
  return FGO_OK;
}

// First synchronisation: did the factorisation succeed.  Then the estimate, chi2 and the look-ahead flags of the next update,
// second synchronisation, what this update carries over, timers and stats.
int finish(fgo_ctx *c, const Forms &f, double relin_threshold, bool wild_possible, double tstart, fgo_stats &st, fgo_stats *stats) {
  IsamState &I = c->isam;
  hipStream_t s = c->stream;
  double *scal = c->d_scal.p;
  HIPCHK(c, hipMemcpyAsync(c->h_fail, c->d_fail.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(c->h_scal + 4, scal + 4, sizeof(double) * 2, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  st.chi2_initial = c->h_scal[4];                       // chi2 at the linearisation point
  st.reserved[1] = c->h_scal[5];                        // variables relinearised by this update
  if (*c->h_fail) {
    c->last = st;
    return fail(c, FGO_ENUM, "ISAM2 update: linear system not positive definite (IndeterminantLinearSystemException)");
  }
  if (f.have_tables) record_L(c, LHolds::isam_step);
  if (f.maskable) I.carry |= IsamState::CARRY_H;
  if (wild_possible) I.carry |= IsamState::CARRY_SOLUTION;
  I.E_seen = (int64_t)c->ei.size(); I.NI_seen = (int64_t)c->imu_payload.size(); I.NP_seen = (int64_t)c->prior_v.size();
  const bool look_next = f.have_tables && I.d_moved_next.p != nullptr && I.flags.moved_next != nullptr;
  launch_isam2_estimate(c->plan, I.d_theta.p, c->d_x.p, I.d_delta.p, c->d_poses[c->cur].p, s, look_next ? I.d_moved_next.p : nullptr, relin_threshold);
  launch_chi2_gtsam(c->plan, c->d_poses[c->cur].p, scal + 0, s);
  HIPCHK(c, hipEventRecord(c->ev[4], s));
  HIPCHK(c, hipMemcpyAsync(c->h_scal, scal, sizeof(double), hipMemcpyDeviceToHost, s));
  if (look_next) HIPCHK(c, hipMemcpyAsync(I.flags.moved_next, I.d_moved_next.p, (size_t)c->plan.n_poses, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  HIPCHK(c, hipGetLastError());
  if (look_next) { I.carry |= IsamState::CARRY_LOOK; I.look_thr = relin_threshold; I.look_nx = c->plan.n_poses; }
  float ms = 0;
  (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]); st.ms_linearize = ms;
  (void)hipEventElapsedTime(&ms, c->ev[1], c->ev[2]); st.ms_factor = ms;
  (void)hipEventElapsedTime(&ms, c->ev[2], c->ev[3]); st.ms_solve = ms;
  (void)hipEventElapsedTime(&ms, c->ev[3], c->ev[4]); st.ms_update = ms;
  (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[4]); st.reserved[0] = ms;
  c->chi_cur = c->h_scal[0];
  c->lin_valid = false;                                 // H / b of the current buffers no longer match the values
  c->dev_poses_newer = true;
  st.chi2_final = c->h_scal[0]; st.lambda_final = 0;
  st.t_total = now_s() - tstart;
  c->last = st;
  if (stats) *stats = st;
  return 1;
}

}  // namespace

extern "C" {

// ISAM2::update + calculateEstimate on the batch machinery (kernels_gtsam.hip: k_isam2_relin / k_isam2_estimate): the steps above,
// in stream order.  Two synchronisations (both in finish), and one event wait where the look-ahead flags are not available.
int fgo_isam2_update(fgo_ctx *c, double relin_threshold, fgo_stats *stats) try {
  if (!c || !(relin_threshold >= 0)) return FGO_EINVAL;
  (void)hipSetDevice(c->cfg.device);
  const double tstart = now_s();
  if (c->shard_world > 1) return fail(c, FGO_ESTATE, "fgo_isam2_update is not available in distributed mode");
  bool was_dirty = false, wild_possible = false;
  int rc = enter(c, was_dirty);
  if (rc) return rc;
  IsamState &I = c->isam;
  const IsamAdded seen{I.n, I.E_seen, I.NI_seen, I.NP_seen};
  if ((rc = fit_state(c, c->plan.n_poses, (int64_t)c->ids.size()))) return rc;   // (n_poses: incl. the phantom slots of the incremental mode)
  fgo_stats st = c->last;
  if (!was_dirty) { st.structure_rebuilt = 0; st.t_symbolic = 0; st.t_upload = 0; }     // (else: set by build() / refresh_factors())
  st.iterations = st.trials = 1; st.terminated = 0;
  st.ms_factor = st.ms_solve = st.ms_update = st.ms_linearize = 0; st.reserved[0] = 0;
  HIPCHK(c, stage_lambda(c, 0.0));                      // Gauss-Newton: no damping (ISAM2GaussNewtonParams)
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  const Forms f = choose_forms(c, relin_threshold);
  DevPlan plan = c->plan;
  int64_t n_dirty_tasks = -1;
  if ((rc = enqueue_relin(c, f, relin_threshold))) return rc;
  // the full linearisation does not depend on the flags: it runs while the host walks the tree; the masked one needs the walk's mask
  if (!f.masked && (rc = enqueue_linearize(c, f))) return rc;
  if (f.partial && (rc = affected_tasks(c, f, seen, plan, n_dirty_tasks))) return rc;
  if (f.masked && (rc = enqueue_linearize(c, f))) return rc;
  if ((rc = enqueue_sweep(c, f, plan))) return rc;
  st.reserved[3] = (double)n_dirty_tasks;               // tasks re-run by this step (-1: full sweep, -2: full sweep because most of the tree was affected)
  if ((rc = enqueue_solve(c, f, plan, wild_possible))) return rc;
  st.reserved[4] = I.last.cut ? 1.0 : 0.0;              // this update cut its back-substitution (wildfire)
  return finish(c, f, relin_threshold, wild_possible, tstart, st, stats);
} FGO_CATCH_INT(c)

int fgo_isam2_reserve(fgo_ctx *c, int reserve_variables, int window) try {
  if (!c || reserve_variables < 0 || window < 0) return FGO_EINVAL;
  c->isam_reserve = reserve_variables;
  if (window > 0) c->isam_window = window;
  if (c->inc.valid) { c->inc.valid = false; c->structure_dirty = true; }      // the next use rebuilds with the new reserve
  return FGO_OK;
} FGO_CATCH_INT(c)

// growth reserve of g2o-semantics contexts (same machinery, same parameters as fgo_isam2_reserve)
int fgo_set_growth(fgo_ctx *c, int reserve_variables, int window) try {
  if (!c || reserve_variables < 0 || window < 0) return FGO_EINVAL;
  const bool on = reserve_variables > 0;
  if (on != c->grow_incremental || (on && (c->isam_reserve != reserve_variables || (window > 0 && c->isam_window != window)))) {
    if (c->inc.valid || on) { c->inc.valid = false; c->structure_dirty = true; }   // the next use rebuilds with / without the reserve
  }
  c->grow_incremental = on;
  c->grow_auto = on ? 1 : 0;
  if (on) { c->isam_reserve = reserve_variables; if (window > 0) c->isam_window = window; }
  return FGO_OK;
} FGO_CATCH_INT(c)

int fgo_isam2_set_wildfire(fgo_ctx *c, double threshold) try {
  if (!c || !(threshold >= 0)) return FGO_EINVAL;
  c->isam.wild.thr = threshold;
  c->isam.invalidate_carry(IsamState::CARRY_SOLUTION);                               // (the next update solves everything and leaves its solution behind)
  return FGO_OK;
} FGO_CATCH_INT(c)

int fgo_isam2_reset(fgo_ctx *c) try {
  if (!c) return FGO_EINVAL;
  (void)hipSetDevice(c->cfg.device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  IsamState &I = c->isam;
  I.d_theta.release(); I.d_delta.release();
  I.n = 0;
  I.invalidate_carry();
  drop_isam_step(c); I.E_seen = I.NI_seen = I.NP_seen = 0;
  // the growth reserve belongs to the incremental driving mode: a context that leaves it (delete isam2) goes back to a
  // structure without phantom slots at its next use; the next fgo_isam2_update lays a fresh reserve down
  c->isam_incremental = false;
  if (c->n_phantom > 0 || c->inc.valid) { c->inc.valid = false; c->structure_dirty = true; }
  // ... and so does the generic (not landmark-eliminated) form fgo_isam2_update had switched the context to
  if (c->ba_disable) { c->ba_disable = false; c->structure_dirty = true; }
  return FGO_OK;
} FGO_CATCH_INT(c)

int fgo_isam2_get_state(fgo_ctx *c, int64_t id, double theta7[7], double delta6[6]) try {
  if (!c || (!theta7 && !delta6)) return FGO_EINVAL;
  (void)hipSetDevice(c->cfg.device);
  auto it = c->id2idx.find(id);
  if (it == c->id2idx.end()) return fail(c, FGO_EINVAL, "unknown variable id");
  if (it->second >= c->isam.n) return fail(c, FGO_ESTATE, "variable not yet seen by fgo_isam2_update");
  if (theta7) HIPCHK(c, hipMemcpy(theta7, c->isam.d_theta.p + (size_t)it->second * 8, 7 * sizeof(double), hipMemcpyDeviceToHost));
  if (delta6) HIPCHK(c, hipMemcpy(delta6, c->isam.d_delta.p + (size_t)it->second * 6, 6 * sizeof(double), hipMemcpyDeviceToHost));
  return FGO_OK;
} FGO_CATCH_INT(c)

}  // extern "C"
