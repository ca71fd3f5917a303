// Structure phase of libfgo, build(): the phases in order -- semantics and variable indices (here), unique pairs and block graph
// (structure_pairs.cpp), ordering and symbolic factorisation (here; ordering.cpp, symbolic.cpp), host tables (structure_tables.cpp,
// structure_ba.cpp), device upload and DevPlan (structure_upload.cpp).  The in-place extension of the incremental mode
// (refresh_factors) and what it shares with the build: structure_grow.cpp.  What a phase hands on: structure_build.hpp.
#include "structure_build.hpp"
#include <memory>

namespace fgo {

// ---- semantics of the context (g2o / GTSAM), growth reserve of the incremental mode, landmarks to eliminate, free-variable indices
static int classify(fgo_ctx *c, VarIndex &V, BuildTimer &tm) {
  const int64_t N = V.N = (int64_t)c->ids.size(), E = V.E = (int64_t)c->ei.size();
  // one semantics per context: g2o ([t;q] tangent, VertexSE3 oplus) or GTSAM ([w;v] tangent, Expmap retraction)
  int64_t n_gtsam = 0;
  for (int64_t e = 0; e < E; ++e) n_gtsam += c->torder[e] != FGO_TANGENT_G2O;   // torder doubles as the factor kind
  bool non_pose = false;
  for (int64_t v = 0; v < N; ++v) non_pose |= c->var_kind[v] != 0;
  if (non_pose && n_gtsam != E) return fail(c, FGO_EINVAL, "plane / point / vector variables need a GTSAM-semantics graph");
  for (int64_t e = 0; e < E; ++e)
    if (c->torder[e] == 3 && !c->cam_set) return fail(c, FGO_EINVAL, "reprojection factors need fgo_set_calib_ds2 first");
  if ((n_gtsam != 0 && n_gtsam != E) || (n_gtsam == 0 && E > 0 && !c->prior_v.empty()))
    return fail(c, FGO_EINVAL, "a context holds either g2o-semantics edges or GTSAM-semantics factors, not both");
  c->gtsam_mode = n_gtsam > 0 || !c->prior_v.empty() || non_pose || !c->imu_payload.empty();
  if (!c->imu_payload.empty() && n_gtsam != E) return fail(c, FGO_EINVAL, "IMU factors need a GTSAM-semantics graph");
  if (c->dev_poses_newer) { int rc = download_poses(c); if (rc) return rc; }
  destroy_graphs(c);
  prepare_device_kernels();
  { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->cfg.device) == hipSuccess && cus > 0) c->sched.cus = cus; }
  // incremental mode: R phantom variables behind the real ones (free, no factors, identity diagonal)
  static const int env_reserve = std::getenv("FGO_ISAM_RESERVE") ? std::atoi(std::getenv("FGO_ISAM_RESERVE")) : 384;
  static const int env_window = std::getenv("FGO_ISAM_WINDOW") ? std::atoi(std::getenv("FGO_ISAM_WINDOW")) : 64;
  const int isam_reserve = c->isam_reserve >= 0 ? c->isam_reserve : env_reserve;
  // (g2o-semantics growth: a new key frame reaches back 1 + m_lookback_nodes <= 8 vertices, g2o/g2o_parameter.cpp:15 -- a band of
  //  16 holds it; the GTSAM drivers' IMU / plane / landmark factors get 64.  cfg 2 with band 64: +7.7 % block updates, with 16: +0.5 %)
  V.isam_window = c->isam_window > 0 ? c->isam_window : (c->gtsam_mode ? env_window : std::min(env_window, 16));
  // g2o-semantics graphs: the reference adds key frames between optimizeGraph() calls (g2o/test_g2o_graph.cpp:80-83); the
  // second time a structure has to be rebuilt because the graph GREW, growth mode switches itself on
  if (!c->gtsam_mode && c->grow_auto && c->built_N >= 0 && N > c->built_N && !(std::getenv("FGO_GROW") && std::atoi(std::getenv("FGO_GROW")) == 0))
    c->grow_incremental = true;
  const bool growing = c->gtsam_mode ? c->isam_incremental : c->grow_incremental;
  const int64_t R = V.R = (growing && c->shard_world == 1) ? isam_reserve : 0;
  const int64_t NX = V.NX = N + R;
  c->inc.valid = false;
  c->n_phantom = (int)R;
  V.NI = (int64_t)c->imu_payload.size();
  V.lm_index.assign((size_t)NX, -1);
  ba_select_landmarks(c, V);
  // free-variable (hessian) index per pose
  V.hidx = std::vector<int>((size_t)NX, -1);
  for (int64_t v = 0; v < NX; ++v) if ((v >= N || !c->fixed[v]) && V.lm_index[v] < 0) V.hidx[v] = V.nfree++;
  if (V.nfree == 0 && V.n_lm > 0) {                    // nothing but landmarks is free (pure triangulation): they stay columns
    std::fill(V.lm_index.begin(), V.lm_index.end(), -1);
    V.n_lm = 0;
    for (int64_t v = 0; v < NX; ++v) if (v >= N || !c->fixed[v]) V.hidx[v] = V.nfree++;
  }
  if (V.nfree == 0 || (E == 0 && c->prior_v.empty() && c->imu_payload.empty()))
    return fail(c, FGO_ESTATE, "nothing to optimise (no free vertex or no factor)");
  tm.prof = std::getenv("FGO_SYM_PROFILE") != nullptr;
  tm.tprev = now_s();
  return FGO_OK;
}

// ---- nested dissection, symbolic factorisation, schedule (ordering*.cpp, symbolic*.cpp)
static int order_and_symbolic(fgo_ctx *c, const VarIndex &V, const PairGraph &G, Ordering &O, BuildTimer &tm) {
  Symbolic &S = c->S;
  const char *wl = std::getenv("FGO_TASK_WORK");
  // light subtrees (one workgroup each, level 0): flat optimum 1250 .. 10000 on cfg 2 since the panel kernels exist
  const int64_t work_limit = wl ? std::atoll(wl) : 5000;
  const double cl_v = tune("chain_work", -1.0);
  // chains become panels (<= PANEL_MAX columns); with the LDS panel kernels the work bound no longer pays
  // (cfg 2: 60000 -> 31.6 it/s, unbounded -> 38.7 it/s)
  const int64_t chain_limit = cl_v >= 0 ? (int64_t)cl_v : (int64_t)1 << 60;
  O.world = c->shard_world; O.rank = c->shard_rank;
  // The bisection is greedy and the landscape of (levels, fill) noisy: on 100k-pose graphs the variants below differ by
  // 1-4 levels and 2-8 % iterations/s, and which one wins depends on the graph.  fgo_config.order_candidates (or
  // FGO_TUNE=nd_try=N) > 1 builds the first N of them and keeps the structure with the lowest PREDICTED sweep time -- a model
  // fitted on the measured sweeps (profiles/NOTES.md round 4): 76 us per level (every level is a chain of dependent launches
  // whatever it holds) + 0.051 ns per block update.  One candidate (the default) costs nothing extra.
  // Distributed mode: the cut into sub-trees per rank wants the better-balanced bisections of weight 8 (per-rank trial of
  // cfg 2 at 8 ranks, tools/dist_rank_timing.py: 2.21 ms against 2.55 with weight 5; one GPU: 148 against 151 it/s).
  struct Cand { double bal_w; int leaf; };
  static const Cand cands1[4] = {{5.0, 64}, {4.0, 64}, {8.0, 64}, {4.0, 96}}, candsN[4] = {{8.0, 64}, {5.0, 64}, {12.0, 64}, {8.0, 96}};
  const Cand *cands = O.world > 1 ? candsN : cands1;
  const int n_try = std::max(1, std::min(4, c->cfg.order_candidates > 0 ? c->cfg.order_candidates : (int)tune("nd_try", 1)));
  double best_cost = 0;
  int best = -1;
  for (int q = 0; q < n_try; ++q) {
    OrderingOptions oo;
    oo.leaf = c->cfg.nd_leaf > 0 ? c->cfg.nd_leaf : (int)tune("nd_leaf", cands[q].leaf);
    oo.bal_w = tune("nd_bal_w", cands[q].bal_w); oo.bal_t = tune("nd_bal_t", oo.bal_t);
    oo.dense_factor = tune("dense_factor", oo.dense_factor);
    // (time dissection ignores the balance weight: its candidates vary the balance window instead -- five 100k-pose seeds, predicted
    //  sweep + backward of the best of four against the first: -2 % on average, profiles/NOTES.md round 5)
    static const double tcand[4][2] = {{0.30, 0.0}, {0.30, 0.1}, {0.35, 0.0}, {0.25, 0.1}};
    oo.time_side = tune("nd_time_side", tcand[q][0]); oo.time_weight = tune("nd_time_weight", tcand[q][1]);
    // (recovered time labels: graphs whose variables are all poses -- a pose graph read from a file with arbitrary ids; ordering.cpp)
    oo.time_recover = true;
    for (int64_t v = 0; v < V.N && oo.time_recover; ++v) oo.time_recover = c->var_kind[(size_t)v] == 0;
    std::vector<int> pq;
    const double ta = now_s();
    nested_dissection(G.g, oo, pq);
    O.t_ord += now_s() - ta;
    if ((int)pq.size() != V.nfree) return fail(c, FGO_EINVAL, "internal: ordering lost vertices");
    if (n_try == 1) { O.perm.swap(pq); S.cus = c->sched.cus; build_symbolic(G.g, O.perm, work_limit, chain_limit, S, O.world); best = 0; break; }
    Symbolic Sq;
    Sq.cus = c->sched.cus;
    build_symbolic(G.g, pq, work_limit, chain_limit, Sq, O.world, true);      // (analysis only: the winner is built in full below)
    const double cost = 76.0 * (double)(Sq.level_ptr.size() - 1) + 0.051e-3 * (double)Sq.nops;      // us
    if (tm.prof) std::fprintf(stderr, "[fgo build]    ordering candidate %d (balance %.1f, leaf %d): %zu levels, %lld block updates, nnz(L) %lld -> predicted %.0f us\n", q,
                           oo.bal_w, oo.leaf, Sq.level_ptr.size() - 1, (long long)Sq.nops, (long long)Sq.nnzL, cost);
    if (best < 0 || cost < best_cost) { best = q; best_cost = cost; O.perm.swap(pq); }
  }
  if (n_try > 1) { S.cus = c->sched.cus; build_symbolic(G.g, O.perm, work_limit, chain_limit, S, O.world); }
  tm.lap("ordering + build_symbolic");
  O.nb = V.nfree;
  O.dist = O.world > 1;
  O.top_col0 = O.dist ? S.dom_col0[O.world] : O.nb;
  O.top_blk0 = O.dist ? S.colptr[O.top_col0] : S.nnzL;
  return FGO_OK;
}

// ---- incremental-mode bookkeeping, statistics
static void finish(fgo_ctx *c, const VarIndex &V, const Ordering &O, const BaTables &BA, double t0, double t1) {
  Symbolic &S = c->S;
  const int64_t hblocks = c->plan.n_hblocks;
  fgo_stats &st = c->last;
  std::memset(&st, 0, sizeof(st));
  st.structure_rebuilt = 1;
  c->last_phase_rebuilt = 1;
  st.t_symbolic = t1 - t0;
  st.t_upload = now_s() - t1;
  st.n_free = O.nb - (int)V.R + V.n_lm; st.n_edges = V.E;         // the phantom slots of the incremental mode are not the caller's variables
  st.nnz_H_blocks = (int64_t)hblocks; st.nnz_L_blocks = S.nnzL; st.n_update_ops = S.nops;
  st.n_levels = c->sched.n_levels; st.n_tasks = (int)S.task_ptr.size() - 1;
  // algorithmic HBM bytes: factor = read H once + write L once; solve = read L twice;
  // linearise = edge payload (232 B) + two 64-B pose gathers per edge, once per half-edge, + H/b written once
  // (the forward solve is fused into the factor sweep: it re-reads L once there; the solve phase is the backward sweep)
  st.bytes_factor = 288.0 * (double)hblocks + 2.0 * 288.0 * (double)S.nnzL + 2.0 * 48.0 * O.nb;
  st.bytes_solve = 288.0 * (double)S.nnzL + 2.0 * 48.0 * O.nb;
  st.bytes_linearize = (double)V.E * (8 + 56 + 168) + (double)V.E * 2 * 56 + 288.0 * (double)hblocks + 48.0 * O.nb;
  if (V.n_lm > 0) {
    // landmark elimination: pixel + weight (24 B), camera pose (64 B), landmark (32 B) per observation and side, the coupling
    // block W written once (144 B); per trial W read, Y written and read once more by the reduction (3 x 144 B) plus the
    // 3x3 blocks; the back-substitution reads Y again
    const double no = (double)BA.obs_uvw.size() / 3.0;
    st.bytes_linearize += no * (2.0 * (24 + 64 + 32) + 144) + 72.0 * V.n_lm;
    st.bytes_factor += no * 3.0 * 144 + 144.0 * V.n_lm;
    st.bytes_solve += no * 144 + 96.0 * V.n_lm;
  }
  if (c->cfg.verbose)
    std::fprintf(stderr, "[fgo] build: N=%lld E=%lld free=%d nnzL=%lld ops=%lld levels=%d tasks=%d symbolic %.3fs (ordering %.3fs) upload %.3fs\n",
                 (long long)V.N, (long long)V.E, O.nb, (long long)S.nnzL, (long long)S.nops, st.n_levels, st.n_tasks, st.t_symbolic, O.t_ord, st.t_upload);
  // host copies of the big lists are no longer needed.  Unmapping a few hundred MB takes tens of milliseconds (cfg 2: 31 ms
  // here + 30 ms for this object's own tables, a seventh of a fresh context's first optimize()): a detached thread does it.
  {
    struct Lists { IntList a, b, c, d; };
    Lists *gone = new Lists;
    gone->a.swap(S.op_a); gone->b.swap(S.op_b); gone->c.swap(S.g2_a); gone->d.swap(S.g2_b);
    release_detached(gone);
  }
}

// The phases of a structure build, in order.
static int build_phases(fgo_ctx *c) {
  // (the phases' host tables are released by a detached thread once everything is on the device, see finish())
  struct Tables { VarIndex V; PairGraph G; Ordering O; HostTables T; BaTables BA; };
  struct Release { void operator()(Tables *p) const noexcept { release_detached(p); } };
  std::unique_ptr<Tables, Release> holder(new Tables);
  Tables &d = *holder;
  BuildTimer tm;
  const double t0 = now_s();
  int rc;
  if ((rc = classify(c, d.V, tm)) != FGO_OK) return rc;
  if ((rc = pairs_and_graph(c, d.V, d.G, tm)) != FGO_OK) return rc;
  if ((rc = order_and_symbolic(c, d.V, d.G, d.O, tm)) != FGO_OK) return rc;
  if ((rc = host_tables(c, d.V, d.G, d.O, d.T, d.BA.lm_mine, tm)) != FGO_OK) return rc;
  if ((rc = ba_tables(c, d.V, d.G, d.O, d.T, d.BA, tm)) != FGO_OK) return rc;
  const double t1 = now_s();
  if ((rc = upload_structure(c, d.V, d.G, d.O, d.T, d.BA, tm)) != FGO_OK) return rc;
  finish(c, d.V, d.O, d.BA, t0, t1);
  // the poses go up HERE, while the host tables are still alive: their release (a detached thread unmapping ~1.5 GB) holds the
  // address-space lock, and the first thing after a build -- a fresh staging vector for the poses, its page faults, the pinning of the
  // copy -- used to wait 45-70 ms behind it (cfg 2; measured round 5)
  if (c->host_poses_newer && (rc = upload_poses(c)) != FGO_OK) return rc;
  if (std::getenv("FGO_SYM_PROFILE")) std::fprintf(stderr, "[fgo build]    phases done after %.1f ms (symbolic %.1f + upload %.1f)\n", 1e3 * (now_s() - t0), 1e3 * c->last.t_symbolic, 1e3 * c->last.t_upload);
  return FGO_OK;
}

// Structure build: ordering, symbolic factorisation, device upload.  Replaces BlockSolver::buildStructure +
// the CSparse symbolic decomposition g2o redoes on iteration 0 of every optimize() call; here it is cached
// until vertices or edges are added.
int build(fgo_ctx *c) {
  const double t0 = now_s();
  const int rc = build_phases(c);
  if (std::getenv("FGO_SYM_PROFILE")) std::fprintf(stderr, "[fgo build]    build() %.1f ms in all (incl. releasing its host tables)\n", 1e3 * (now_s() - t0));
  return rc;
}

}  // namespace fgo
