/* fgo.h — C-ABI of the MI355X-native batch factor-graph optimiser (libfgo.so).
 *
 * This is the drop-in boundary for the optimiser back-end that rising-turtle/graph_slam delegates
 * to g2o / GTSAM.  Every entry point names the reference call site it replaces
 * (paths relative to the reference tree).  Plain C: opaque context, pointers and sizes, no C++ or
 * torch types.  Every function returns 0 on success or a negative FGO_E* code and never throws;
 * fgo_last_error() gives the message.  One context per caller thread (the reference's wrappers
 * are single-threaded too: g2o/g2o_graph.cpp, gtsam/gtsam_graph.cpp).  Arrays passed in are
 * copied; the context owns all device (HBM) memory.  All arithmetic is IEEE f64.
 *
 * Conventions: pose = t[3] + unit quaternion q[4] in (x,y,z,w) order (Eigen coeff order);
 * X = (R(q), t) maps local -> world.  Information matrices are passed as the 21 upper-triangular
 * entries, row-major (O00 O01 .. O05 O11 ..), the VRO record order (gtsam/gtsam_graph.cpp:1574-1590).
 */
#ifndef FGO_H
#define FGO_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libfgo.so is built with -fvisibility=hidden: the declarations below are the whole export list. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define FGO_OK 0
#define FGO_EINVAL (-1)   /* bad argument / unknown id                                   */
#define FGO_ENODEV (-2)   /* no HIP device, or the HIP runtime reported an error          */
#define FGO_ENOMEM (-3)
#define FGO_ESTATE (-4)   /* nothing to optimise (g2o's optimize() == -1)                */
#define FGO_ENUM (-5)     /* numerical failure: factorisation not positive definite       */

/* tangent / information ordering of an SE3 edge */
#define FGO_TANGENT_G2O 0    /* [t; q]   g2o EdgeSE3        (g2o/g2o_graph.cpp:125-132)      */
#define FGO_TANGENT_GTSAM 1  /* [w; v]   gtsam BetweenFactor (gtsam/gtsam_graph.cpp:689-692) */

typedef struct fgo_ctx fgo_ctx;

typedef struct {
  int device;          /* HIP device ordinal (default 0)                                   */
  int verbose;         /* 0 silent (reference: setVerbose(false), g2o_graph.cpp:70)        */
  int ordering;        /* 0 = nested dissection + local minimum degree (default)           */
  int nd_leaf;         /* nested-dissection leaf size in poses (0 = default 64)            */
  int order_candidates;/* 0 / 1: one ordering (default).  2 .. 4: that many orderings (balance weight / leaf size variants) are built
                          and the one with the lowest predicted sweep time (levels x 76 us + block updates x 0.051 ns) is kept:
                          +2 .. 4 % iterations/s on 100k-pose graphs for 2 .. 4 x the structure phase -- for long runs      */
  int reserved[11];
} fgo_config;

/* Result of one fgo_optimize() call == one g2o SparseOptimizer::optimize(n) call. */
typedef struct {
  int iterations;      /* LM iterations performed (what optimize() returns)                */
  int trials;          /* linear solves, accepted + rejected                               */
  int terminated;      /* algorithm returned 'Terminate' (10 failed trials / rho == 0)     */
  int structure_rebuilt;
  double chi2_initial, chi2_final, lambda_final;
  /* wall-clock (host) seconds */
  double t_symbolic, t_upload, t_total;
  /* device milliseconds from hipEvents on the context's stream */
  double ms_linearize, ms_factor, ms_solve, ms_update;
  /* structure */
  int64_t n_free, n_edges, nnz_H_blocks, nnz_L_blocks, n_update_ops;
  int n_levels, n_tasks;
  /* algorithmic HBM bytes of ONE pass of each phase: factor = H read + L written + L re-read by the
     forward solve fused into the factor sweep; solve = the backward sweep (L read once) */
  double bytes_factor, bytes_linearize, bytes_solve;
  double reserved[8];
} fgo_stats;

/* ---- lifecycle: replaces CGraphG2O::createOptimizer (g2o/g2o_graph.cpp:65-77) and the
 *      NonlinearFactorGraph/Values allocation in CGraphGT::CGraphGT (gtsam/gtsam_graph.cpp:75-91) */
fgo_ctx *fgo_create(const fgo_config *cfg);          /* NULL cfg = defaults; NULL on failure */
void fgo_destroy(fgo_ctx *ctx);                      /* ~CGraphG2O: g2o_graph.cpp:50-56       */
const char *fgo_last_error(const fgo_ctx *ctx);      /* ctx may be NULL (creation errors)     */
const char *fgo_version(void);
int fgo_device_count(void);                          /* HIP devices visible, <0 on error      */

/* ---- variables: VertexSE3 creation, g2o/g2o_graph.cpp:88-91 (fixed first vertex), :115-119;
 *      Values::insert / update of Pose3, gtsam/gtsam_graph.cpp:331,655-669 */
int fgo_add_pose(fgo_ctx *ctx, int64_t id, const double t[3], const double q_xyzw[4], int fixed);
int fgo_set_pose(fgo_ctx *ctx, int64_t id, const double t[3], const double q_xyzw[4]);
int fgo_set_fixed(fgo_ctx *ctx, int64_t id, int fixed);       /* OptimizableGraph::Vertex::setFixed ("FIX id" of a .g2o file) */
int fgo_get_pose(fgo_ctx *ctx, int64_t id, double out7[7]);   /* VertexSE3::estimate(), :297,327 */
int fgo_has_pose(const fgo_ctx *ctx, int64_t id);             /* mp_optimizer->vertex(id) != 0, :98-99 */
int64_t fgo_num_poses(const fgo_ctx *ctx);
int64_t fgo_num_edges(const fgo_ctx *ctx);
/* bulk forms (poses7 = n x 7, ids may be NULL for 0..n-1 continuing from the current count) */
int fgo_add_poses(fgo_ctx *ctx, int64_t n, const int64_t *ids, const double *poses7,
                  const unsigned char *fixed);
int fgo_get_poses(fgo_ctx *ctx, int64_t n, const int64_t *ids, double *poses7);

/* ---- factors: EdgeSE3 + setMeasurement + setInformation, g2o/g2o_graph.cpp:125-132;
 *      BetweenFactor<Pose3> + Gaussian::Information, gtsam/gtsam_graph.cpp:689-692 */
int fgo_add_edge_se3(fgo_ctx *ctx, int64_t id_i, int64_t id_j, const double t[3],
                     const double q_xyzw[4], const double info_ut21[21], int tangent_order);
int fgo_add_edges_se3(fgo_ctx *ctx, int64_t n, const int64_t *id_i, const int64_t *id_j,
                      const double *meas7, const double *info_ut21, int tangent_order);

/* ---- GTSAM-semantics factors.  A context is either a g2o-semantics graph (FGO_TANGENT_G2O edges, solved by
 *      fgo_optimize) or a GTSAM-semantics graph (FGO_TANGENT_GTSAM edges + priors, solved by fgo_optimize_gtsam);
 *      mixing the two in one context is an error (their Jacobians refer to different retractions).
 *      PriorFactor<Pose3>(X(id), mean, noise): gtsam/gtsam_graph.cpp:338-341 (Diagonal::Sigmas(1e-7 x 6) ->
 *      info = diag(1/sigma^2)); information passed as 21 upper-triangular entries in [omega; v] order. */
int fgo_add_prior_pose(fgo_ctx *ctx, int64_t id, const double t[3], const double q_xyzw[4], const double info_ut21[21]);
/* Plane landmarks: Values::insert(L(id), OrientedPlane3(a,b,c,d)) — gtsam/gtsam_graph.cpp:1198-1202 — and
 *      OrientedPlane3Factor(z, noiseModel::Gaussian::Covariance(S), X(pose), L(plane)) — gtsam/gtsam_graph.cpp:1265.
 *      z = measured plane (a,b,c,d) in the pose frame; cov_ut6 = upper triangle of the 3x3 covariance S, row-major.
 *      Any variable's current value is read back with fgo_get_pose (7 slots: plane = nx ny nz d, point = x y z). */
int fgo_add_plane(fgo_ctx *ctx, int64_t id, const double abcd[4]);
int fgo_add_plane_factor(fgo_ctx *ctx, int64_t pose_id, int64_t plane_id, const double z_abcd[4], const double cov_ut6[6]);
/* Bundle adjustment: Values::insert(Q(id), Point3) + PriorFactor<Point3>(Isotropic::Sigma(3, sigma)) —
 *      gtsam/gtsam_graph.cpp:379,387-394; Cal3DS2(fx,fy,s,u0,v0,k1,k2[,p1,p2]) — :373; GenericProjectionFactor<Pose3,
 *      Point3, Cal3DS2>(z, Isotropic::Sigma(2, sigma), X, Q, K, false, false, body_P_sensor) — :405-409.
 *      body_P_sensor7 = t(3) q_xyzw(4), NULL = identity. */
int fgo_add_point3(fgo_ctx *ctx, int64_t id, const double xyz[3]);
int fgo_add_prior_point3(fgo_ctx *ctx, int64_t id, const double xyz[3], double sigma);
int fgo_set_calib_ds2(fgo_ctx *ctx, double fx, double fy, double s, double u0, double v0, double k1, double k2, double p1,
                      double p2, const double body_P_sensor7[7]);
int fgo_add_reproj(fgo_ctx *ctx, int64_t pose_id, int64_t point_id, const double uv[2], double sigma);
/* bulk forms: n points (+ PriorFactor<Point3> when prior_sigma > 0) / n projection factors */
int fgo_add_points3(fgo_ctx *ctx, int64_t n, const int64_t *ids, const double *xyz, double prior_sigma);
int fgo_add_reprojs(fgo_ctx *ctx, int64_t n, const int64_t *pose_ids, const int64_t *point_ids, const double *uv, double sigma);
/* Batched two-view bundle adjustment: CGraphGT::bundleAdjust (gtsam/gtsam_graph.cpp:500-610) for n_pairs independent
 * visual-odometry records in ONE launch, one wave per pair (the reference's offline tools call it record after record:
 * gtsam/test/convert_vo2ba.cpp:210-243, :300, convert_vo2ba_2.cpp:177).  Pair p owns the matches
 * [match_ptr[p], match_ptr[p+1]) of xyz_i (the feature in camera i, M x 3), uv_i / uv_j (its pixel in either image, M x 2):
 *      pose i   starts at identity, PriorFactor<Pose3>(identity, sigma pose_prior_sigma)          :537
 *      pose j   starts at pose_j0[p] (t(3) q_xyzw(4), unit quaternion; NULL = identity, as the reference starts), free
 *      point k  starts at xyz_i[k], PriorFactor<Point3>(xyz_i[k], sigma point_sigma)              :574
 *      two GenericProjectionFactor<Pose3, Point3, Cal3DS2>(sigma pixel_sigma) per match           :539
 *      calib9 = fx fy s u0 v0 k1 k2 p1 p2 and body_P_sensor7 as fgo_set_calib_ds2 takes them (NULL = identity);
 *      cheirality as in a context (throwCheirality = false).
 * LevenbergMarquardtOptimizer::optimize() with the controller of fgo_optimize_gtsam (lambda0 1e-5, factor 10, upper bound
 * 1e5, identity damping on poses and points, minModelFidelity 1e-3, relative / absolute tolerance 1e-5); then the system is
 * linearised undamped at the final estimate: cov36_out = Marginals::marginalCovariance of pose j (6x6 row-major, tangent
 * [omega; v]), info_ut21_out = its inverse, symmetric by construction, as the 21 upper-triangular entries
 * fgo_add_edge_se3(..., FGO_TANGENT_GTSAM) takes.  error_* = 0.5 sum |whitened r|^2, priors included.
 * Stateless, host arrays in and out, like fgo_preint_batch.  FGO_EINVAL (before any HIP call): negative or decreasing
 * match_ptr, more than INT_MAX / 3 matches in one pair, a NULL required pointer, a sigma <= 0, min_matches < 3, a zero quaternion in body_P_sensor7; FGO_ENODEV without a
 * HIP device (no CPU fallback).  n_pairs == 0: FGO_OK.  A numerical failure of one pair is that pair's status: the call still
 * returns FGO_OK and no other pair is affected (a pair's result does not depend on what else is in the batch). */
typedef struct {
  double pose_prior_sigma;   /* 1e-7   gtsam_graph.cpp:537 */
  double point_sigma;        /* 0.014  :574 */
  double pixel_sigma;        /* 1.0    :539 */
  int max_iters;             /* <= 0: 100 (GTSAM default) */
  int min_matches;           /* 5: the reference returns false for matches.size() <= 4 (:513); values < 3 are FGO_EINVAL */
} fgo_two_view_params;
void fgo_two_view_params_default(fgo_two_view_params *p);
#define FGO_TV_OK 0
#define FGO_TV_TOO_FEW 1     /* fewer than min_matches: pose_j_out = start, cov / info zero */
#define FGO_TV_NUM 2         /* a non-finite residual, or a pivot of the undamped reduced system <= 0 or non-finite:
                                the pose is returned as LM left it, cov / info zero */
typedef struct { int status, iterations, trials; double error_initial, error_final, lambda_final; } fgo_two_view_result;
int fgo_two_view_ba_batch(int device, int64_t n_pairs, const int64_t *match_ptr /* n_pairs + 1 */,
                          const double *xyz_i /* M x 3 */, const double *uv_i /* M x 2 */, const double *uv_j /* M x 2 */,
                          const double *pose_j0 /* n_pairs x 7, NULL = identity */,
                          const double calib9[9], const double body_P_sensor7[7] /* NULL = identity */,
                          const fgo_two_view_params *params /* NULL = defaults */,
                          double *pose_j_out /* n x 7 */, double *pose_i_out /* n x 7, may be NULL */,
                          double *cov36_out /* n x 36, may be NULL */, double *info_ut21_out /* n x 21, may be NULL */,
                          fgo_two_view_result *result /* n */);
/* Plane check of visual-odometry records, batched: what gtsam/test_plane_check_vo.cpp does record after record
 * (computePlaneNodeDis :328-379, computePlaneDis :383-445; gtsam/test/delete_vo_by_plane_check.cpp consumes its log and sets the
 * information of the rejected records to the 10000 sentinel, :189), for n_records independent records in ONE launch, one wave
 * per record.  Record r has the relative pose Tij = pose_ij7[r] (t(3) q_xyzw(4), the pose of frame j in frame i: Pose3(final_trafo),
 * :165-166; the quaternion is normalised on entry) and the covariance Sij: either info_ut21[r]^-1 (:167; the 21 upper-triangular
 * entries in tangent [omega; v] that fgo_two_view_ba_batch writes, inverted on the device by a 6x6 Cholesky factorisation) or
 * cov36[r] as given (6x6 row-major, only its upper triangle is read; it has to be positive semi-definite, which is not tested,
 * and the sentinel does not apply).  Exactly one of the two is passed, the other is NULL.  The record owns the planes
 * [pi_ptr[r], pi_ptr[r+1]) seen in frame i and [pj_ptr[r], pj_ptr[r+1]) seen in frame j.  A plane is (a, b, c, d): the normal is
 * normalised on entry and d left untouched, as fgo_add_plane_factor does; cov16 is CPlane::m_CP (4x4 row-major), of which the
 * upper triangle of the 3x3 normal block S_n and entry (3, 3) S_d are read.  The tangent covariance of a plane is
 * S_P = diag(B^T S_n B, S_d), B = Unit3::basis(n) (:395-406).
 *   plane i     PE = Pi.transform(Tij): n' = R^T n, d' = n.t + d, with the Jacobians D_pose (3x6) and D_plane (3x3) of
 *               OrientedPlane3::transform;  S_PE = D_pose Sij D_pose^T + D_plane S_Pi D_plane^T (:409).
 *               pred_abcd_out = PE, pred_cov9_out = S_PE (row-major, in the tangent of PE),
 *               sdj_out = S_di + n^T S_t n + g^T S_ni g, g = (I - n n^T) t, S_t = Sij[3:6, 3:6]  (CGraphGT::computeSdj,
 *               gtsam/gtsam_graph.cpp:725-748, with CP(3, 3) standing in for m_E_Sdi)
 *   matching    planes i are taken in order; plane i takes the FIRST j, in order, with |n'.n_j| >= cos_min and
 *               |d' - d_j| <= d_max (:338-362); several i may take the same j.  match_out[i] = the index of that j within the
 *               record's own j-list, or -1
 *   pair        e = PE.errorVector(Pj) = [B(n')^T n_j; d' - d_j], raw = e.e, S_e = H1 S_PE H1^T + H2 S_Pj H2^T,
 *               d2 = e^T S_e^-1 e by a 3x3 Cholesky factorisation;  H2 = diag(B(n')^T B(n_j), -1), H1 = diag(Hp, 1) with Hp the
 *               derivative of B(n')^T n_j along n' -> retract(n', v), taken through the basis rule with the axis choice held
 *               fixed (GTSAM 4.0's Unit3::errorVector).  A pair whose S_e is not positive definite is counted in n_bad, gets
 *               d2_out = raw_out = +inf and takes no part in the maximum.  Unmatched planes: d2_out = raw_out = 0
 *   record      err = the largest d2 over the matched planes i, by strict > in order of i from 0 (a tie stays with the earlier
 *               i), err_raw = that pair's raw, best_i / best_j = that pair (indices within the record's lists), -1 when
 *               no pair raised err above 0;  n_matched = planes i that took a j (the bad ones included)
 * A record whose status is not FGO_PC_OK has err = err_raw = 0, nothing matched (match_out = -1) and every other per-plane
 * output zero.  Stateless, host arrays in and out, like fgo_two_view_ba_batch.  FGO_EINVAL (before any HIP call): a NULL
 * required pointer, both or neither of info_ut21 / cov36, a negative or decreasing ptr array (or more than INT_MAX planes in one
 * list), a zero quaternion or a zero normal, cos_min outside [-1, 1], d_max < 0; FGO_ENODEV without a HIP device (no CPU
 * fallback).  n_records == 0: FGO_OK.  A record's result never depends on what else is in the batch. */
typedef struct {
  double cos_min;        /* cos(10 deg)   test_plane_check_vo.cpp:330,355 */
  double d_max;          /* 0.2           :355 */
  double failed_info00;  /* 10000: information (0,0) == this marks a failed VO record (:171); <= 0 disables the test */
} fgo_plane_check_params;
void fgo_plane_check_params_default(fgo_plane_check_params *p);      /* NULL tolerated */
#define FGO_PC_OK 0
#define FGO_PC_SKIPPED 1   /* failed-VO sentinel: err = err_raw = 0, nothing matched (:171-176) */
#define FGO_PC_NUM 2       /* the record's information is not positive definite (a pivot <= 0 or non-finite): err = err_raw = 0 */
typedef struct { int status, n_matched, n_bad, best_i, best_j, reserved; double err, err_raw; } fgo_plane_check_result;
int fgo_plane_check_vro_batch(int device, int64_t n_records,
                              const double *pose_ij7 /* n x 7 */,
                              const double *info_ut21 /* n x 21, or NULL */, const double *cov36 /* n x 36, or NULL */,
                              const int64_t *pi_ptr /* n + 1 */, const double *pi_abcd /* Mi x 4 */, const double *pi_cov16 /* Mi x 16 */,
                              const int64_t *pj_ptr /* n + 1 */, const double *pj_abcd /* Mj x 4 */, const double *pj_cov16 /* Mj x 16 */,
                              const fgo_plane_check_params *params /* NULL = defaults */,
                              fgo_plane_check_result *result /* n */,
                              int64_t *match_out /* Mi */, double *d2_out /* Mi */, double *raw_out /* Mi */,
                              double *pred_abcd_out /* Mi x 4 */, double *pred_cov9_out /* Mi x 9 */,
                              double *sdj_out /* Mi */);   /* each of the six may be NULL */
/* Plane extraction from depth frames, batched: the step that PRODUCES the planes the call above and fgo_add_plane_factor /
 * fgo_gate_plane_factors / fgo_associate_planes consume -- what the reference obtains frame after frame, on the CPU, from
 * CPlaneNode::extractPlanes(i_img, d_img, &sr4k) (gtsam/test_plane_check_vo.cpp:181,188,213; gtsam/test_ba_imu_graph.cpp:137,274,297;
 * gtsam/test/test_plane_propagate.cpp:144,307) -- for n_frames independent frames in ONE launch, one workgroup per frame.  The plane
 * package's own arithmetic is not part of the reference tree, so the semantics below are THIS PROJECT'S DEFINITION, pinned to the
 * numpy restatement tests/plane_extract_reference.py and not to the plane package.  depth is n x H x W depth words, row-major.
 *   points      pixel (u, v) with depth word w has z = w z_scale and is VALID iff z_min < z < z_max;
 *               p = ((u - cx) z / fx, (v - cy) z / fy, z)  (CamModel::convertUVZ2XYZ; lens distortion is out of scope)
 *   rounds      r = 0 .. max_planes - 1.  The CANDIDATES of round r are the valid pixels not yet given to a plane, in pixel order
 *               (v W + u), M their number.  M < max(3, min_pixels): the search stops (the round is not run).
 *   sampling    the sampler of fgo_vro_ransac_batch with the round folded into the counter: hypothesis h of round r draws
 *               u_k = mix(seed + ((r hypotheses + h) 3 + k + 1) 0x9E3779B97F4A7C15), k = 0, 1, 2, and from them three distinct
 *               candidates a, b, c exactly as there.  A hypothesis depends on (seed, r, h, M) only.
 *   hypothesis  m = (p_b - p_a) x (p_c - p_a); invalid (count -1) if |m| < min_area.  n = m / |m|, d = -n.p_a, both negated when
 *               d < 0: n.p + d = 0 with the camera on the positive side.  count = the number of candidates with |n.p + d| <= max_dist.
 *               Winner: the largest count, ties to the lowest h.  No valid hypothesis, or the winner's count < min_pixels: the
 *               search stops.
 *   refinement  the set starts as the winner's inliers; up to refine_rounds times: total-least-squares fit on the set (centroid c,
 *               the 3x3 scatter of the centred points in a second pass, the eigenvector of its smallest eigenvalue by a fixed
 *               number of cyclic Jacobi sweeps, d = -n.c, the same orientation rule), the new set = the round's candidates within
 *               max_dist of that fit; stop early when the set did not change.  A set below min_pixels: the search stops and this
 *               plane is not kept.  Otherwise the set leaves the candidates and the next round begins.
 *   final pass  every valid pixel goes to the kept plane with the smallest |n.p + d| (ties to the lower index) if that distance is
 *               <= max_dist, else its label is -1.  A plane left with fewer than min_pixels is dropped: its pixels become -1 and the
 *               later planes move up.  Each remaining plane is fitted once more on its final set by the same fit: that is abcd_out;
 *               n_pixels, rmse (of n.p + d) and centroid are over that set.  The labels are not recomputed after the final fit.
 *               Without this pass the first plane of a corner keeps the neighbouring walls' pixels within max_dist of it, and the
 *               covariance below is too small by one to two orders of magnitude.
 *   covariance  B = Unit3::basis(n), J_k = [p_k^T B, 1] (1x3), sigma_k^2 = n^T Sigma(p_k) n with Sigma(p) the pixel-plus-depth model
 *               of fgo_vro_ransac_batch: sigma_px^2 ((n_x z / fx)^2 + (n_y z / fy)^2) + sigma_z(z)^2 (n.r)^2, r = p / z.  The fit
 *               is unweighted, so its first-order covariance is the sandwich C = A^-1 M A^-1, A = sum J_k^T J_k (inverted by a
 *               3x3 Cholesky), M = sum sigma_k^2 J_k^T J_k; C is exactly symmetric.  cov_ut6_out = the upper triangle of C in the
 *               tangent [dn(2); dd]: what fgo_add_plane_factor, fgo_gate_plane_factors and fgo_associate_planes take.
 *               cov16_out = E C E^T, E = [[B, 0], [0, 1]] (4x4 row-major): CPlane::m_CP as fgo_plane_check_vro_batch reads it (its
 *               B^T S_n B and S_d return the diagonal blocks of C).  C is the covariance of the DEPTH NOISE, not of the
 *               segmentation: near intersections a residual bias of the sequential search remains.
 *   status      A not positive definite, or a non-finite value in a plane: the frame is FGO_PX_NUM with n_planes = 0, zero outputs
 *               and labels of -2 / -1 only.  FGO_PX_OK otherwise; zero planes is OK.  rounds_run = the rounds whose hypotheses
 *               were scored.  Per plane: best_hypothesis / best_count / n_valid_hyp of the round that found it, fits = the fits
 *               of that round's refinement.  The slots past n_planes are zero.
 *   diagnosis   hyp_count_out[f][r][h] = the count, -1 for an invalid hypothesis, -2 for every h of a round that was not run.
 * Every sum over pixels is a per-lane sum in pixel order followed by a fixed butterfly, the waves merged in wave order, no atomics:
 * results are bit-identical from call to call and do not depend on the rest of the batch.  Stateless, host arrays in and out, like
 * fgo_vro_ransac_batch; the call holds 30 bytes of scratch per pixel of the batch on the device (FGO_ENOMEM: split the batch).
 * FGO_EINVAL (before any HIP call): a NULL required pointer, a negative n_frames, width or height < 1 or width height > 2^24,
 * fx / fy / z_scale / max_dist / min_area / sigma_px <= 0, z_min >= z_max, hypotheses outside [1, 65536], max_planes outside
 * [1, FGO_PX_MAX_PLANES], refine_rounds outside [0, 10], min_pixels < 3, a sigma_z coefficient < 0 or all three zero;
 * FGO_ENODEV without a HIP device (no CPU fallback).  n_frames == 0: FGO_OK. */
#define FGO_PX_MAX_PLANES 8
typedef struct {
  double fx, fy, cx, cy;   /* 250.5773, 250.5773, 90, 70  (gtsam_graph.cpp:544) */
  double z_scale;          /* 0.001: metres per depth word (CamModel::m_z_scale) */
  double z_min, z_max;     /* 0.1, 5.0 */
  int hypotheses;          /* 512, in [1, 65536]: per round */
  uint64_t seed;           /* 0 */
  double max_dist;         /* 0.05 m (our choice: about 3.5 sigma_z) */
  double min_area;         /* 1e-3 m^2 */
  int min_pixels;          /* 1500, >= 3 */
  int max_planes;          /* 4, in [1, FGO_PX_MAX_PLANES] */
  int refine_rounds;       /* 3, in [0, 10] */
  double sigma_px;         /* 1.0 */
  double sigma_z[3];       /* {0.014, 0, 0}: sigma_z(z) = s0 + s1 z + s2 z^2, as fgo_vro_params */
} fgo_plane_extract_params;
void fgo_plane_extract_params_default(fgo_plane_extract_params *p);      /* NULL tolerated */
#define FGO_PX_OK 0
#define FGO_PX_NUM 2       /* A is not positive definite or a plane holds a non-finite value: no planes, zero outputs */
typedef struct { int status, n_planes, n_valid_pixels, rounds_run; } fgo_plane_extract_result;
typedef struct { int n_pixels, best_hypothesis, best_count, n_valid_hyp, fits, reserved; double rmse, centroid[3]; } fgo_plane_extract_plane;
int fgo_plane_extract_batch(int device, int64_t n_frames, int width, int height,
                            const uint16_t *depth /* n x H x W, row-major */,
                            const fgo_plane_extract_params *params /* NULL = defaults */,
                            fgo_plane_extract_result *result /* n */,
                            double *abcd_out /* n x max_planes x 4 */, double *cov16_out /* n x max_planes x 16 */,
                            double *cov_ut6_out /* n x max_planes x 6, may be NULL */,
                            fgo_plane_extract_plane *plane_out /* n x max_planes, may be NULL */,
                            int8_t *label_out /* n x H x W, may be NULL: -2 no depth, -1 no plane, k */,
                            int32_t *hyp_count_out /* n x max_planes x hypotheses, may be NULL: for tests and diagnosis */);
/* development: the kernel time of the last fgo_plane_extract_batch call by HIP events, ms */
double fgo_debug_plane_extract_kernel_ms(void);
/* Plane propagation between depth frames, batched: what the reference does frame after frame, on the CPU, in
 * CGraphGT::predictPlaneNode part 1 with computeSdj, inThisPlane, intensityTol and regionGrow (gtsam/gtsam_graph.cpp:725-1041; called at
 * gtsam/test_vro_imu_graph.cpp:241,595 and gtsam/test_ba_imu_graph.cpp:253-365) when visual odometry failed and only the IMU's pose
 * is left -- for n_pairs independent pairs of frames in ONE launch, one workgroup per pair.  The frames (depth words, intensity
 * bytes, the label image and the planes of fgo_plane_extract_batch or of this call) are given once, n_frames x H x W row-major and
 * n_frames x FGO_PX_MAX_PLANES planes, of which frame f uses the first n_planes[f]; pair p carries the planes of frame frame_i[p]
 * into frame frame_j[p].  All arithmetic is in double: the reference's float pixel coordinates (ujf, vjf, du, dv) are NOT reproduced.
 * T = pose_ij7[p] (t(3) q_xyzw(4), the pose of frame j in frame i, the quaternion normalised on entry), S its covariance in
 * [omega; v]: cov36[p] as given or info_ut21[p] inverted by the 6x6 Cholesky of fgo_plane_check_vro_batch, exactly one of the two;
 * only S_t = S[3:6, 3:6] is read (:889).  The planes l = 0 .. n_planes[frame_i] - 1 are taken in order; ONE flag image of frame j is
 * shared by all of them (:897): a pixel is free, CLAIMED by a plane, or REJECTED.
 *   prediction  (computeSdj) n normalised on entry, n_j = R^T n, d_j = n.t + d, S_dj = S_di + n^T S_t n + g^T S_ni g, g = (I - n n^T) t,
 *               S_ni = cov16[0:3, 0:3], S_di = cov16[3][3] standing in for m_E_Sdi: the pred_abcd_out and sdj_out of
 *               fgo_plane_check_vro_batch.  The predicted plane is not re-oriented.
 *   in plane    (inThisPlane) with e = fma(n_j.x, x, fma(n_j.y, y, fma(n_j.z, z, d_j))): e^2 <= S_dj or e^2 <= d_floor^2
 *   seeds       (:941-1017) every pixel of frame i with label == l is back-projected with frame i's depth (the points of
 *               fgo_plane_extract_batch), carried over, p_j = R^T (p_i - t), and projected, u = fx x / z + cx, v = fy y / z + cy.  A
 *               point with z <= 0, or with u or v non-finite or of magnitude >= 2^30, seeds nothing (this rule is ours).  The nine
 *               candidates are ((int)(u + du), (int)(v + dv)), du, dv in {-0.5, 0, 0.5}, truncated toward zero as C does: a
 *               projection less than a pixel left of or above the image still seeds column or row 0, as in the reference.  A
 *               candidate inside the image whose flag is free takes frame j's depth z: not z_min < z < z_max -> REJECTED; else
 *               CLAIMED by l if its back-projection is in the plane and REJECTED if not.  The outcome depends on the pixel and
 *               the plane alone, so the seed set does not depend on the order of the pixels.  n_seed = the pixels claimed.
 *   keep        (:1024-1025) the plane goes on iff n_seed > (int)(keep_ratio n_prev), n_prev = its pixels in frame i, the product in
 *               double.  A plane that fails keeps its claimed pixels in the flag image (the reference never clears them) and gives
 *               no output plane.
 *   growth      (regionGrow, kept planes only) the reference's queue computes a unique fixed point, and the result is DEFINED as it:
 *               the smallest set E that holds the plane's seeds and is closed under: p in E, q a 4-neighbour of p with
 *               |I(p) - I(q)| <= intensity_tol; then q is in E if q is claimed (by this plane, an earlier one or a dropped one: it
 *               conducts and does not join), or if q is free and in the plane by frame j's depth (it joins plane l).  No depth-range
 *               test here (:800-802): a pixel without a return back-projects to the origin.  REJECTED pixels neither join nor
 *               conduct; a free pixel that fails stays free for later planes (the == of :822 is a no-op, and that is kept).
 *               n_pixels = n_seed + the pixels that joined.
 *   refit       (:1031; computeCOVSparse is not in the reference tree, so this is ours) the fit, orientation (d >= 0), rmse, centroid
 *               and sandwich covariance of fgo_plane_extract_batch on the plane's final pixel set, with frame j's back-projections
 *               (not the carried-over points the reference collects) and without the reference's down-sampling by 4.  Output slot k
 *               is the k-th kept plane; plane_out[k].source = l, whose landmark id the caller carries over.
 *   record      num_added = sum of n_pixels over the kept planes + sum of n_seed over the dropped ones (:1040); search_rest = 0 if
 *               num_added > (int)(rest_ratio W H), 2 if num_added == 0, 1 otherwise (:1047-1077: nothing to do / extract from the
 *               whole frame / extract from the free pixels).  label_out: k = the kept plane of slot k, -1 free, -2 free and the depth
 *               outside (z_min, z_max), -3 REJECTED, -4 claimed by a dropped prediction; with -1 / -2 / k it reads like the label image
 *               of fgo_plane_extract_batch and can be the `label` of the next pair.  pred_out[l], per PREVIOUS plane: abcd = (n_j, d_j),
 *               sdj, n_prev, n_seed, kept.  The slots past the last plane are zero.
 *   status      FGO_PP_NUM: the information is not positive definite, some S_dj is negative or not finite, or a refit is not positive
 *               definite or not finite: every output of the pair is zero, its labels are -1 / -2 only and search_rest = 2.
 * Every sum over pixels follows fgo_plane_extract_batch's rule, no atomics: two calls are bit-identical and a pair's result never
 * depends on the rest of the batch.  Stateless, host arrays in and out; the call holds 24 bytes of scratch per pixel of every
 * pair on the device, and one more when width height > 65536 (FGO_ENOMEM: split the batch).  FGO_EINVAL (before any HIP call): a
 * NULL required pointer, both or neither of info_ut21 / cov36, a negative count, width or height < 1 or width height > 2^24, a frame
 * index outside [0, n_frames), n_planes outside [0, FGO_PX_MAX_PLANES], a zero quaternion, a zero normal among the first n_planes of a
 * frame, fx / fy / z_scale / sigma_px <= 0, z_min >= z_max, a sigma_z coefficient < 0 or all three zero, d_floor < 0,
 * intensity_tol < 0, keep_ratio or rest_ratio outside [0, 1]; FGO_ENODEV without a HIP device (no CPU fallback).  n_pairs == 0: FGO_OK. */
typedef struct {
  double fx, fy, cx, cy;   /* 250.5773, 250.5773, 90, 70 */
  double z_scale;          /* 0.001 */
  double z_min, z_max;     /* 0.1, 5.0  (:992) */
  double sigma_px;         /* 1.0 */
  double sigma_z[3];       /* {0.014, 0, 0} */
  double d_floor;          /* 0.014 m: e^2 <= d_floor^2 is in the plane whatever S_dj  (:753) */
  int intensity_tol;       /* 5  (:768) */
  double keep_ratio;       /* 0.7  (:1024) */
  double rest_ratio;       /* 0.5  (:1046) */
} fgo_plane_propagate_params;
void fgo_plane_propagate_params_default(fgo_plane_propagate_params *p);      /* NULL tolerated */
#define FGO_PP_OK 0
#define FGO_PP_NUM 2
typedef struct { int status, n_planes, num_added, search_rest; } fgo_plane_propagate_result;
typedef struct { int n_pixels, n_seed, source, reserved; double rmse, centroid[3]; } fgo_plane_propagate_plane;
typedef struct { double abcd[4], sdj; int n_prev, n_seed, kept, reserved; } fgo_plane_propagate_pred;
int fgo_plane_propagate_batch(int device, int64_t n_frames, int width, int height,
                              const uint16_t *depth /* n_frames x H x W */, const uint8_t *intensity /* n_frames x H x W */,
                              const int8_t *label /* n_frames x H x W */, const int32_t *n_planes /* n_frames */,
                              const double *abcd /* n_frames x FGO_PX_MAX_PLANES x 4 */,
                              const double *cov16 /* n_frames x FGO_PX_MAX_PLANES x 16 */,
                              int64_t n_pairs, const int64_t *frame_i /* n_pairs */, const int64_t *frame_j /* n_pairs */,
                              const double *pose_ij7 /* n_pairs x 7 */,
                              const double *info_ut21 /* n_pairs x 21, or NULL */, const double *cov36 /* n_pairs x 36, or NULL */,
                              const fgo_plane_propagate_params *params /* NULL = defaults */,
                              fgo_plane_propagate_result *result /* n_pairs */,
                              double *abcd_out /* n_pairs x FGO_PX_MAX_PLANES x 4 */, double *cov16_out /* n_pairs x FGO_PX_MAX_PLANES x 16 */,
                              double *cov_ut6_out /* n_pairs x FGO_PX_MAX_PLANES x 6, may be NULL */,
                              fgo_plane_propagate_plane *plane_out /* n_pairs x FGO_PX_MAX_PLANES, may be NULL */,
                              fgo_plane_propagate_pred *pred_out /* n_pairs x FGO_PX_MAX_PLANES, may be NULL */,
                              int8_t *label_out /* n_pairs x H x W, may be NULL */);
/* development: the kernel time of the last fgo_plane_propagate_batch call by HIP events, ms */
double fgo_debug_plane_propagate_kernel_ms(void);
/* utils::chi2(dof, alpha) = boost::math::quantile(chi_squared(dof), alpha) (gtsam/chi2.h:17-26): the x with P(dof / 2, x / 2) = p, P the
 * regularised lower incomplete gamma function (series below x = a + 1, continued fraction above), inverted by a safeguarded Newton
 * iteration from the Wilson-Hilferty start.  Host only.  dof < 1: 0 (as the reference returns); p <= 0: 0; p >= 1: +inf; p NaN: NaN. */
double fgo_chi2_quantile(int dof, double p);
/* ---- IMU: velocity / bias variables, their priors, preintegration and the CombinedImuFactor.
 *      Values::insert(V(id), Vector3) / insert(B(id), imuBias::ConstantBias) + PriorFactor<Vector3>(Isotropic::Sigma(3,
 *      1e-3)) / PriorFactor<ConstantBias>(Isotropic::Sigma(6, 1e-3)) — gtsam/gtsam_graph.cpp:346-367.
 *      bias = [acc(3); gyro(3)].  fgo_preint mirrors PreintegratedCombinedMeasurements (on-manifold form; the
 *      reference's preintegration type is a GTSAM build flag, gtsam/imu_base.h:73 — see DESIGN.md):
 *      fgo_preint_reset + fgo_preint_integrate(acc, gyro, dt) replace resetIntegrationAndSetBias + the
 *      integrateMeasurement loop of CImuBase::predictNext (gtsam/imu_base.cpp:72-87; host-side, per factor);
 *      fgo_imu_params_vn100 = CImuVn100::getIMUParams + MakeSharedD(9.71) (gtsam/imu_vn100.cpp:24-67,
 *      gtsam/imu_base.cpp:258-263); fgo_add_imu_combined = CombinedImuFactor(X(i-1), V(i-1), X(i), V(i), B(i-1), B(i),
 *      preint) added to the graph (gtsam/test_ba_imu_graph.cpp:239-244). */
typedef struct {
  double dt;
  double dR[4];                /* preintegrated rotation, quaternion x y z w */
  double dp[3], dv[3];
  double J_R_bg[9], J_p_ba[9], J_p_bg[9], J_v_ba[9], J_v_bg[9];   /* row-major 3x3 bias Jacobians */
  double bhat[6];              /* bias the measurements were corrected with: acc(3), gyro(3) */
  double cov[225];             /* preintMeasCov, row-major 15x15, order theta p v bias_acc bias_gyro */
} fgo_preint;
typedef struct {
  double acc_cov, gyro_cov, integ_cov, bias_acc_cov, bias_gyro_cov, bias_acc_omega_int;   /* isotropic variances */
  double gravity[3];           /* n_gravity (navigation frame) */
} fgo_imu_params;
void fgo_imu_params_vn100(fgo_imu_params *p);
void fgo_preint_reset(fgo_preint *m, const double bias_hat6[6]);
void fgo_preint_integrate(fgo_preint *m, const fgo_imu_params *p, const double acc[3], const double gyro[3], double dt);
/* PreintegratedCombinedMeasurements::predict(state_i, bias_i): pose_j (7) and velocity_j (3) */
void fgo_preint_predict(const fgo_preint *m, const double gravity[3], const double pose_i7[7], const double vel_i[3],
                        const double bias_i6[6], double pose_j7[7], double vel_j[3]);
/* Batched preintegration on the GPU (the factors are independent; the reference runs the
 * integrateMeasurement loop of CImuBase::predictNext serially on the CPU, gtsam/imu_base.cpp:72-87).  Factor f integrates
 * the samples [sample_ptr[f], sample_ptr[f+1]) of acc / gyro (3 doubles per sample) with step dt, starting from
 * fgo_preint_reset(bias_hat6 + 6 f) (zero bias if NULL).  Same arithmetic as fgo_preint_integrate.  Host arrays in and
 * out; FGO_ENODEV without a HIP device (no CPU fallback -- use fgo_preint_integrate for that). */
int fgo_preint_batch(int device, int64_t n, const int64_t *sample_ptr, const double *acc, const double *gyro, double dt,
                     const double *bias_hat6, const fgo_imu_params *params, fgo_preint *out);
int fgo_add_vec3(fgo_ctx *ctx, int64_t id, const double xyz[3]);
int fgo_add_bias(fgo_ctx *ctx, int64_t id, const double bias6[6]);
int fgo_add_prior_vec3(fgo_ctx *ctx, int64_t id, const double xyz[3], double sigma);
int fgo_add_prior_bias(fgo_ctx *ctx, int64_t id, const double bias6[6], double sigma);
int fgo_set_gravity(fgo_ctx *ctx, const double n_gravity[3]);     /* default (0, 0, 9.71) */
int fgo_add_imu_combined(fgo_ctx *ctx, const int64_t ids6[6] /* Xi Vi Xj Vj Bi Bj */, const fgo_preint *preint);
/* the 15x15 information matrix (row-major, order theta p v ba bg) fgo_add_imu_combined gives the factor:
 * preintMeasCov^-1 by Cholesky, symmetrised -- noiseModel::Gaussian::Covariance(pim.preintMeasCov()) in GTSAM terms.
 * Host-only; FGO_ENUM if the covariance is not positive definite. */
int fgo_preint_information(const fgo_preint *preint, double info225[225]);
/* IMU check of visual-odometry records, batched: the chi-square test the chi2_for_vro switch turns on in the reference's drivers
 * (gtsam/test_vro_imu_graph.cpp:679-778; g_chi2_test :52, :496; the switch is read in test_ba_imu_graph.cpp:575 and
 * test_plane_check_vo.cpp:467 as well) -- the rotation of a record against the rotation the IMU preintegrated between the same
 * two key frames -- for n_records independent records in ONE launch, one wave per record.  Record r has the relative pose
 * pose_ij7[r] (t(3) q_xyzw(4) in the camera frame, as fgo_plane_check_vro_batch takes it; only the quaternion is read, and it is
 * normalised on entry) with the covariance Sij: info_ut21[r]^-1 (6x6 Cholesky on the device, tangent [omega; v]) or cov36[r] (6x6
 * row-major, only the upper triangle of its leading 3x3 block is read); exactly one of the two is passed.  It is tested against
 * preint[preint_index[r]] (what fgo_preint_batch / fgo_preint_integrate produce; several records may name the same one) at the
 * bias bias_i6[r] (acc(3), gyro(3); NULL = every preintegration's own bhat).  imu_q_cam4 is the rotation R_uc of *mp_u2c (x y z w,
 * normalised on entry, NULL = identity): the omega rows of the adjoint hold nothing but R, so its translation does not enter.
 *   dR_imu = dR Exp(J_R_bg (bg_i - bhat_g))   the rotation of pre_p.transform_pose_to(cur_state.pose()) (:708-710), corrected as
 *                                             fgo_preint_predict corrects it
 *   dR_vro = R_uc R(q_ij) R_uc^T              (:692-698)
 *   dRw = dR_imu^T dR_vro, dw = Logmap(dRw), angle = |dw|, D = the inverse right Jacobian at dw;
 *   J_imu = -D dRw^T (Rot3::between's H1 through Logmap's Jacobian, :714-717), J_vro = D (the term the reference has commented out)
 *   calibrated   S = J_imu Sth J_imu^T + J_vro (R_uc Sij[0:3, 0:3] R_uc^T) J_vro^T with Sth = preintMeasCov[0:3, 0:3];
 *                d2 = dw^T S^-1 dw by a 3x3 Cholesky: chi-square with 3 degrees of freedom for a consistent record.
 *                cov_dw9_out = S (row-major, exactly symmetric), dw_out = dw
 *   reference    Lth = (preintMeasCov^-1)[0:3, 0:3], d2_ref = dw^T (J_imu Lth J_imu^T) dw (:724-743): an information-weighted norm
 *                that leaves the record's own uncertainty out and is not chi-square distributed; the 15x15 inverse is
 *                not formed: the covariance is factored with the theta block last, Lth is the inverse Gram matrix of the factor's
 *                trailing 3x3 triangle
 *   reject       bit 0: d2 > d2_gate;  bit 1: d2_ref > d2_ref_gate (:753)
 * preintMeasCov is read as (C + C^T) / 2.  A record whose status is not FGO_IC_OK has every output zero; a preintegration of no
 * samples (covariance 0) is FGO_IC_NUM.  Stateless, host arrays in and out, like fgo_plane_check_vro_batch.  FGO_EINVAL (before any
 * HIP call): a negative n_records, a NULL required pointer, both or neither of info_ut21 / cov36, n_preint < 1 with n_records > 0,
 * an index outside [0, n_preint), a zero quaternion (record or extrinsic), a gate <= 0; FGO_ENODEV without a HIP device (no CPU
 * fallback).  n_records == 0: FGO_OK.  A numerical failure of one record is that record's status; a record's result never depends
 * on what else is in the batch, on its place in it, or on the call. */
typedef struct {
  double d2_gate;        /* fgo_chi2_quantile(3, 0.95) = 7.814727903251179: the CI the reference computes (:683) */
  double d2_ref_gate;    /* 40000  (:753) */
  double failed_info00;  /* 10000: information (0,0) == this marks a failed VO record; <= 0 disables the test */
} fgo_imu_check_params;
void fgo_imu_check_params_default(fgo_imu_check_params *p);          /* NULL tolerated */
#define FGO_IC_OK 0
#define FGO_IC_SKIPPED 1   /* failed-VO sentinel (info_ut21 mode only) */
#define FGO_IC_NUM 2       /* the record's information, preintMeasCov or S is not positive definite (a pivot <= 0 or non-finite) */
typedef struct { int status, reject; double d2, d2_ref, angle; } fgo_imu_check_result;
int fgo_imu_check_vro_batch(int device, int64_t n_records,
                            const double *pose_ij7 /* n x 7 */,
                            const double *info_ut21 /* n x 21, or NULL */, const double *cov36 /* n x 36, or NULL */,
                            int64_t n_preint, const fgo_preint *preint, const int64_t *preint_index /* n, each in [0, n_preint) */,
                            const double *bias_i6 /* n x 6, or NULL */, const double imu_q_cam4[4] /* NULL = identity */,
                            const fgo_imu_check_params *params /* NULL = defaults */,
                            fgo_imu_check_result *result /* n */,
                            double *dw_out /* n x 3, may be NULL */, double *cov_dw9_out /* n x 9, may be NULL */);
/* RANSAC registration of visual-odometry records, batched: the step that PRODUCES the record the three calls above consume -- a
 * RANSAC search over matched 3-D features (m_ransac_iterations = 5000, gtsam/test/convert_vo2ba.cpp:448), a closed-form rigid fit
 * on the inliers (getTransformFromMatches, gtsam/gtsam_graph.cpp:492), the covariance of that fit (CGraphGT::computeCovVRO,
 * :256-277) and the void record when it fails (makeItVoid, convert_vo2ba.cpp:424-436) -- for n_pairs independent pairs in ONE
 * launch, one workgroup per pair.  The VRO library's own arithmetic (matchNodePairVRO, getTransformFromMatches,
 * CCameraNode::computeCov) is not part of the reference tree, so the semantics below are THIS PROJECT'S DEFINITION, pinned to the
 * numpy restatement tests/vro_ransac_reference.py and not to the VRO library.
 * Pair p owns the matches [match_ptr[p], match_ptr[p+1]); xyz_i[k] / xyz_j[k] are the same feature in camera i / camera j.  The
 * result is T = (R, t) with p_i = R p_j + t, the pose of frame j in frame i (pose_j0 of fgo_two_view_ba_batch, pose_ij7 of the two
 * checks), stored t(3) q_xyzw(4) with w >= 0.
 *   sampling    hypothesis h draws three distinct matches a, b, c of the pair's M from counter-based integers (mod 2^64):
 *               u_k = mix(seed + (3 h + k + 1) 0x9E3779B97F4A7C15), k = 0, 1, 2, mix the splitmix64 finaliser
 *               (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31);
 *               a = u0 % M;  b = u1 % (M - 1), b += (b >= a);  c = u2 % (M - 2), c += (c >= min(a, b)), c += (c >= max(a, b)).
 *               A hypothesis depends on (seed, h, M) only.
 *   hypothesis  in either frame the triad e1 = (p_b - p_a) / |p_b - p_a|, e3 = e1 x (p_c - p_a) normalised, e2 = e3 x e1, F = [e1 e2 e3];
 *               R = F_i F_j^T, t = mean_i - R mean_j over the three points.  Invalid (count -1) if |p_b - p_a| < min_side or
 *               |(p_b - p_a) x (p_c - p_a)| < min_side^2 in either frame, or a side length (ab, ac, bc) differs between the frames
 *               by more than rigid_tol.  Otherwise count = the number of the pair's matches with |p_i - (R p_j + t)|^2 <= max_dist^2.
 *               Winner: the largest count, ties to the lowest h.  n_valid = the number of valid hypotheses.
 *   refinement  the set starts as the winner's inliers; refine_rounds times: least-squares fit on the set (centroids, 3x3
 *               cross-covariance of the centred points, the rotation maximising tr(R^T C): Horn's quaternion form, the 4x4
 *               eigenproblem by a fixed number of cyclic Jacobi sweeps), the new set = the inliers of that fit; stop early when
 *               the set did not change.  rounds = the fits made.  Outputs: the pose of the last round (the winner's own with
 *               refine_rounds = 0) and its inliers; rmse over them.
 *   information Fisher information of the pose at the final fit over the final inliers, tangent [omega; v], perturbation T Exp(xi):
 *               r_k = p_i - (R p_j + t), J_k = [-R [p_j]x, R], Sigma(p) = G diag(sigma_px^2, sigma_px^2, sigma_z(z)^2) G^T with
 *               G = [[z / fx, 0, x / z], [0, z / fy, y / z], [0, 0, 1]], S_k = Sigma(p_i) + R Sigma(p_j) R^T,
 *               info = sum_k J_k^T S_k^-1 J_k (a 3x3 Cholesky per match); info_ut21_out = its upper triangle as
 *               fgo_add_edge_se3(..., FGO_TANGENT_GTSAM) and the two checks take it; cov36_out = its inverse by a 6x6 Cholesky,
 *               exactly symmetric.
 *   failed      any status != FGO_VRO_OK gives makeItVoid's record: pose identity, information 10000 on the diagonal, covariance
 *               zero, inlier mask zero, n_inliers = 0, rmse = 0; best_hypothesis / best_count (-1 / -1 when no hypothesis is
 *               valid), n_valid and rounds as found.  The two checks report such a record as skipped.
 * Every sum over matches is a per-lane sum in match order followed by a fixed butterfly: results are bit-identical from call to call
 * and do not depend on the rest of the batch.  Stateless, host arrays in and out, like fgo_two_view_ba_batch.  FGO_EINVAL (before
 * any HIP call): a NULL required pointer, a negative n_pairs, a negative or decreasing match_ptr, more than INT_MAX / 3 matches in
 * one pair, hypotheses outside [1, 2^20], max_dist / min_side / fx / fy / sigma_px <= 0, rigid_tol < 0, refine_rounds outside
 * [0, 10], min_inliers < 3, a sigma_z coefficient < 0 or all three zero; FGO_ENODEV without a HIP device (no CPU fallback).
 * n_pairs == 0: FGO_OK.  A numerical failure of one pair is that pair's status only. */
typedef struct {
  int hypotheses;        /* 5000  m_ransac_iterations (convert_vo2ba.cpp:448) */
  uint64_t seed;         /* 0 */
  double max_dist;       /* 0.03 m (our choice: VRO's value is not in the reference) */
  double min_side;       /* 0.05 m */
  double rigid_tol;      /* 0.03 m */
  int refine_rounds;     /* 3, 0 .. 10 */
  int min_inliers;       /* 8  (convert_vo2ba.cpp:228) */
  double fx, fy;         /* 250.5773  (gtsam_graph.cpp:544) */
  double sigma_px;       /* 1.0 */
  double sigma_z[3];     /* {0.014, 0, 0}: sigma_z(z) = s0 + s1 z + s2 z^2  (0.014: gtsam_graph.cpp:379) */
} fgo_vro_params;
void fgo_vro_params_default(fgo_vro_params *p);            /* NULL tolerated */
#define FGO_VRO_OK 0
#define FGO_VRO_TOO_FEW 1   /* fewer than 3 matches, no valid hypothesis, or fewer than min_inliers inliers after any round */
#define FGO_VRO_NUM 2       /* non-finite input reached the fit, z <= 0 on an inlier, or the information is not positive definite */
typedef struct { int status, n_inliers, best_hypothesis, best_count, n_valid, rounds; double rmse; } fgo_vro_result;
int fgo_vro_ransac_batch(int device, int64_t n_pairs, const int64_t *match_ptr /* n + 1 */,
                         const double *xyz_i /* M x 3 */, const double *xyz_j /* M x 3 */,
                         const fgo_vro_params *params /* NULL = defaults */,
                         double *pose_ij7_out /* n x 7 */, double *info_ut21_out /* n x 21, may be NULL */,
                         double *cov36_out /* n x 36, may be NULL */, uint8_t *inlier_out /* M, may be NULL */,
                         int32_t *hyp_count_out /* n x hypotheses, may be NULL: for tests and diagnosis */,
                         fgo_vro_result *result /* n */);
/* development: waves per pair of the next fgo_vro_ransac_batch calls (1 or 4; 0 = the default), returns the value in force; and
 * the kernel time of the last call by HIP events, ms */
int fgo_debug_vro_waves(int waves);
double fgo_debug_vro_kernel_ms(void);
/* development: the largest grid of the next launches of the capped-grid kernels (map fusion, cleaning, normals and rendering, the
 * cell index, vocabulary training and place query), which stride over whatever the grid does not cover: 1 .. 2^20; 0 = the default,
 * 2^20; any other value changes nothing.  Returns the value in force.  Results do not depend on it; tests lower it to run every
 * stride loop past its grid at small shapes. */
int fgo_debug_grid_cap(int cap);

/* Descriptor matching of key-frame pairs, batched: the step that PRODUCES the matched 3-D features the calls above start from --
 * CCameraNode::matchNodePair before its RANSAC (g2o/g2o_graph.cpp:174,210-211, gtsam/gtsam_graph.cpp:1730-1731) and the pose-guided
 * matchNodePairBA(ni, Tji, pcam) of CGraphGT::vroAdjust (gtsam/gtsam_graph.cpp:450-498, gtsam/test/convert_vo2ba.cpp:206) -- for
 * n_pairs independent pairs in ONE launch, one workgroup per pair.  The reference fixes 128-byte SIFT descriptors, m_nn_distance_ratio
 * = 0.5 and m_min_matches = 12 (gtsam/test_gt_graph.cpp:165-172); the matching arithmetic itself (matchNodePair, matchNodePairBA,
 * the FLANN search) is not part of the reference tree, so the semantics below are THIS PROJECT'S DEFINITION, pinned to the numpy
 * restatement tests/feature_match_reference.py and not to the VRO library.
 * Frame f owns the features [feat_ptr[f], feat_ptr[f+1]) of desc (SIFT as OpenCV stores it, integers 0 .. 255), xyz (camera frame)
 * and uv (undistorted pixels).  Pair p matches the features of frame_j[p] (the queries, local index a) against those of frame_i[p]
 * (the trains, local index b).  pose_ij7 (t q_xyzw, p_i = R p_j + t, as fgo_vro_ransac_batch writes it) guides a pair: NULL = no
 * pair is guided; with guided == NULL every pair is, otherwise the pairs with guided[p] != 0.
 *   usable      a feature whose three coordinates are finite with z > 0; any other never matches (reason 1) and is no candidate.
 *   distance    d(a, b) = sum_k (desc_a[k] - desc_b[k])^2, an integer <= 128 * 255^2 = 8 323 200, computed exactly.
 *   candidates  unguided: every usable (a, b).  Guided: also gate(a, b): with p = R^T (xyz_b - t), the train in frame j, p.z > 0 and
 *               (fx p.x / p.z + cx - u_a)^2 + (fy p.y / p.z + cy - v_a)^2 <= radius_px^2 and, if max_dist_3d > 0,
 *               |p - xyz_a|^2 <= max_dist_3d^2.  The gate belongs to the PAIR (a, b): the cross-check runs over the same set.
 *   best        b1 = the candidate with the smallest d, ties to the lowest b; d1 = d(a, b1); d2 = the smallest d over the
 *               candidates other than b1 (a tie at the minimum gives d2 = d1).  No candidate: reason 2, best = d1 = d2 = -1.
 *               Exactly one candidate: d2 = -1 and the ratio test passes.
 *   ratio       (if ratio_test) kept iff (double) d1 < r2 * (double) d2 with r2 = ratio * ratio formed once in f64; else reason 3.
 *   cap         d1 <= max_desc_dist2, else reason 4.
 *   cross       (if cross_check) kept iff a is the candidate query with the smallest d(., b1), ties to the lowest a; else reason 5.
 *               Without it several queries may keep the same train.
 * The first test that fails gives the reason; reason 0 is a match.  The matches of a pair are its kept queries in ascending a.
 * Per query, indexed q_ptr[p] + a with q_ptr the prefix sum of the pairs' query counts (Q = q_ptr[n_pairs]): best_out (b1), d1_out,
 * d2_out, reason_out.  Packed by the host after the download, capacity Q rows, the first match_ptr_out[n_pairs] filled:
 * idx_i_out / idx_j_out (GLOBAL feature indices) and the gathers xyz_i_out, xyz_j_out, uv_i_out, uv_j_out -- with match_ptr_out
 * exactly what fgo_vro_ransac_batch and fgo_two_view_ba_batch take.  dist_out (for tests and diagnosis, like hyp_count_out): the
 * full matrix of every pair one after the other, N_j x N_i int32, row a, column b, -1 where (a, b) is no candidate.
 * result: n_query / n_train = the usable features of frame j / frame i, n_matches, n_ratio / n_cross = the queries the ratio test /
 * the cross-check rejected (reasons 3 / 5); status FGO_FM_TOO_FEW when n_matches < min_matches -- the matches are written all the
 * same, the caller applies the reference's 4 (gtsam_graph.cpp:463) / 8 / 20 (convert_vo2ba.cpp:210,231) thresholds itself.
 * The arithmetic is integer, the column minima are integer atomic minima: results are bit-identical from call to call and a pair's
 * result does not depend on the rest of the batch.  Stateless, host arrays in and out, like fgo_vro_ransac_batch.  FGO_EINVAL
 * (before any HIP call): a NULL required pointer, a negative n_frames or n_pairs, a negative or decreasing feat_ptr, more than
 * FGO_FM_MAX_FEATURES features in a frame, a frame index outside [0, n_frames), a zero quaternion on a guided pair, ratio outside
 * (0, 1], radius_px / fx / fy <= 0, max_dist_3d < 0, max_desc_dist2 < 0, min_matches < 0; FGO_ENODEV without a HIP device (no CPU
 * fallback).  n_pairs == 0: FGO_OK. */
#define FGO_FM_DIM 128
#define FGO_FM_MAX_FEATURES 4096
typedef struct {
  double ratio;          /* 0.5  m_nn_distance_ratio (test_gt_graph.cpp:165-172); compared squared, on squared distances */
  int ratio_test;        /* 1 */
  int cross_check;       /* 1 */
  int32_t max_desc_dist2;/* INT32_MAX: off */
  int min_matches;       /* 12  m_min_matches */
  double radius_px;      /* 10.0 (our choice) */
  double max_dist_3d;    /* 0: off */
  double fx, fy, cx, cy; /* 250.5773, 250.5773, 90, 70: the SR4000 pinhole */
} fgo_match_params;
void fgo_match_params_default(fgo_match_params *p);        /* NULL tolerated */
#define FGO_FM_OK 0
#define FGO_FM_TOO_FEW 1    /* n_matches < min_matches */
typedef struct { int status, n_query, n_train, n_matches, n_ratio, n_cross; } fgo_match_result;
int fgo_match_features_batch(int device, int64_t n_frames, const int64_t *feat_ptr /* n_frames + 1 */,
                             const uint8_t *desc /* F x 128 */, const double *xyz /* F x 3 */, const double *uv /* F x 2 */,
                             int64_t n_pairs, const int64_t *frame_i, const int64_t *frame_j,
                             const double *pose_ij7 /* n x 7, or NULL */, const uint8_t *guided /* n, or NULL */,
                             const fgo_match_params *params /* NULL = defaults */,
                             fgo_match_result *result /* n */, int64_t *q_ptr_out /* n + 1, may be NULL */,
                             int32_t *best_out /* Q, may be NULL */, int32_t *d1_out /* Q, may be NULL */,
                             int32_t *d2_out /* Q, may be NULL */, uint8_t *reason_out /* Q, may be NULL */,
                             int64_t *match_ptr_out /* n + 1 */, int64_t *idx_i_out /* Q */, int64_t *idx_j_out /* Q */,
                             double *xyz_i_out /* Q x 3, may be NULL */, double *xyz_j_out /* Q x 3, may be NULL */,
                             double *uv_i_out /* Q x 2, may be NULL */, double *uv_j_out /* Q x 2, may be NULL */,
                             int32_t *dist_out /* sum N_j N_i, may be NULL: for tests and diagnosis */);
/* development: the kernel time of the last fgo_match_features_batch call by HIP events, ms */
double fgo_debug_match_kernel_ms(void);

/* Voxel-grid map fusion of depth frames, batched: the step that turns the optimised trajectory into the run's product, the map --
 * mapping/mapping_PCD.cpp:86-167, mapping_PCD_rs.cpp:127-252, mapping_PLY*.cpp, map_video*.cpp: every key frame is back-projected
 * (generatePointCloud), range-filtered (passThroughZ), carried into the world by Pw2c = Pw2j * Pu2c (mapping_PCD.cpp:140-144),
 * appended to the map and thinned with pcl::VoxelGrid at voxel_grid_size = 0.02 (mapping_PCD_rs.cpp:59-66,220-229), frame after frame
 * on the CPU -- for ALL n_frames in ONE call.  PCL is not part of the reference tree, so the semantics below are THIS PROJECT'S
 * DEFINITION, pinned to the numpy restatement tests/map_fuse_reference.py.  Where they differ from the reference: its grid is aligned
 * to the cloud's bounding box and its arithmetic is in float, ours is world-aligned (voxel i covers [i, i + 1) leaves from the
 * world's origin) with integer sums; it re-filters the accumulated map after each frame (an unweighted centroid of centroids), ours
 * is ONE centroid per voxel over all points of all frames; lens distortion and the median filter of mapping_PLY_rs.cpp:172
 * are out of scope; the clustering and floor removal of pcd_filter.cpp are fgo_map_clean below (min_points only drops thin voxels);
 * the caller chooses the frames (trajectory_skip).
 *   pose        frame f has pose_w7[f] = t_w(3) q_xyzw(4), as fgo_get_poses gives it; extrinsic7 (t_e, q_e) is Pu2c, NULL = identity.
 *               A quaternion is normalised on entry: each component divided by sqrt(((qx qx + qy qy) + qz qz) + qw qw).  With the
 *               normalised (x, y, z, w):  R00 = 1 - 2 (y y + z z)  R01 = 2 (x y - z w)      R02 = 2 (x z + y w)
 *                                         R10 = 2 (x y + z w)      R11 = 1 - 2 (x x + z z)  R12 = 2 (y z - x w)
 *                                         R20 = 2 (x z - y w)      R21 = 2 (y z + x w)      R22 = 1 - 2 (x x + y y)
 *               each product and sum rounded on its own.  With an extrinsic R = R_w R_e, R_ij = (Rw_i0 Re_0j + Rw_i1 Re_1j) + Rw_i2 Re_2j,
 *               and t_i = ((Rw_i0 te_0 + Rw_i1 te_1) + Rw_i2 te_2) + tw_i.  This runs on the host, without fused multiply-adds;
 *               rt_out[f] = R row-major, then t: exactly what the kernel used.
 *   sampling    the pixels (u, v) = (su + a skip, sv + b skip), a, b >= 0, u < eu, v < ev; rect = {su, sv, eu, ev}, all zero = the whole
 *               image.  n_sampled counts them over all frames.
 *   point       z = w z_scale for the depth word w; the point is valid iff z_min < z < z_max (the project's rule, not PCL's closed
 *               interval).  p = (((u - cx) z) / fx, ((v - cy) z) / fy, z); x_k = ((R_k0 p_0 + R_k1 p_1) + R_k2 p_2) + t_k.  EVERY
 *               product, quotient and sum is rounded to double on its own: the kernel does not contract them.
 *   quantum     Q_k = llrint(x_k 2^20), ties to even: the quantum is 2^-20 m = 0.95 um.  L = llrint(leaf 2^20): the EFFECTIVE leaf is
 *               L 2^-20 (0.02 m -> 20972 quanta = 0.0200005 m).  i_k = floor(Q_k / L), floor division of the QUANTISED coordinate: a
 *               point at -1e-6 has Q = -1 and is in voxel -1, a point at -1e-7 rounds to Q = 0 and is in voxel 0.  r_k = Q_k - i_k L
 *               lies in [0, L).  A valid point with a non-finite x_k or some |i_k| >= 2^20 is OUT OF RANGE: counted in
 *               n_out_of_range, not in n_valid, not stored.
 *   key         ((i_z + 2^20) << 42) | ((i_y + 2^20) << 21) | (i_x + 2^20)
 *   voxel       n = its number of points, S_k = sum r_k, C_c = sum colour_c: integer sums, whatever the order of arrival.
 *   output      the voxels with n >= min_points in ascending key (the others are counted in n_dropped):
 *               xyz_k = ((double)(i_k L) + (double)S_k / (double)n) 2^-20, colour_c = (2 C_c + n) / (2 n) in integer division (the mean
 *               rounded half up), count = n, key.  frame_points_out[f] = the valid points of frame f; n_valid their sum.
 * result: status FGO_MAP_OK; FGO_MAP_TRUNCATED when n_voxels > max_voxels: n_voxels is the true number and the first max_voxels rows
 * in key order are written; FGO_MAP_FULL when the hash table filled up: no voxel is written, n_voxels = n_dropped = 0 (the counts of
 * points, frame_points_out and rt_out are written), and the call still returns FGO_OK.  table_log2 = T, the table has 2^T slots of
 * 64 bytes: automatic (0) is the smallest T >= 4 with 2^T >= 2 n_sampled, which cannot fill; a caller who knows the map is small
 * sets it lower.  Two calls give bit-identical outputs, and so does any permutation of the frames (frame_points_out and rt_out
 * permuted alike).  Stateless, host arrays in and out, like fgo_plane_extract_batch; only min(n_voxels, max_voxels) rows are copied
 * back.  FGO_EINVAL (before any HIP call): result NULL, n_frames < 0, max_voxels < 0, width or height < 1 or their product > 2^24,
 * n_frames x sampled pixels >= 2^31, channels not 0, 1 or 3, fx, fy, z_scale <= 0 or not finite, cx or cy not finite,
 * z_min >= z_max, skip < 1, a rect that is empty or not inside the image, leaf outside [2^-20, 1024], min_points < 1, table_log2
 * outside {0} u [4, 32]; and for n_frames > 0: depth or
 * pose_w7 NULL, xyz_out NULL with max_voxels > 0, color NULL with channels > 0 or not NULL with channels == 0, a zero (or
 * non-finite) quaternion.  n_frames == 0: FGO_OK and a zero result.  FGO_ENODEV without a HIP device (no CPU fallback).  FGO_ENOMEM:
 * the table does not fit: split the batch or set table_log2. */
typedef struct {
  double fx, fy, cx, cy;   /* 250.5773, 250.5773, 90, 70: the SR4000 pinhole */
  double z_scale;          /* 0.001 */
  double z_min, z_max;     /* 0.1, 5.0 (mapping_PCD_rs keeps 0 .. 1.2) */
  int skip;                /* 2: downsample_skip, >= 1 */
  int rect[4];             /* su, sv, eu, ev; all zero = the whole image; eu, ev exclusive */
  double leaf;             /* 0.02 m: voxel_grid_size */
  int min_points;          /* 1 */
  int table_log2;          /* 0 = automatic; else in [4, 32] */
} fgo_map_params;
void fgo_map_params_default(fgo_map_params *p);            /* NULL tolerated */
#define FGO_MAP_OK 0
#define FGO_MAP_TRUNCATED 1  /* n_voxels > max_voxels: the first max_voxels in key order are written */
#define FGO_MAP_FULL 2       /* the hash table is full: no outputs, n_voxels = 0 */
typedef struct { int status, table_log2; int64_t n_sampled, n_valid, n_out_of_range, n_voxels, n_dropped; } fgo_map_result;
int fgo_map_fuse_batch(int device, int64_t n_frames, int width, int height,
                       const uint16_t *depth /* n x H x W */, const uint8_t *color /* n x H x W x channels, NULL iff channels == 0 */,
                       int channels /* 0, 1 or 3 */, const double *pose_w7 /* n x 7: t(3) q_xyzw(4), as fgo_get_poses gives them */,
                       const double *extrinsic7 /* Pu2c, NULL = identity */, const fgo_map_params *params /* NULL = defaults */,
                       int64_t max_voxels, fgo_map_result *result /* 1 */,
                       double *xyz_out /* max_voxels x 3 */, uint8_t *color_out /* max_voxels x channels, may be NULL */,
                       int32_t *count_out /* may be NULL */, int64_t *key_out /* may be NULL */,
                       int64_t *frame_points_out /* n, may be NULL */, double *rt_out /* n x 12, may be NULL */);
/* development: the device time of the last fgo_map_fuse_batch call by HIP events (table init, insert, pack; sort, finalise), ms */
double fgo_debug_map_fuse_kernel_ms(void);

/* Cluster filtering and floor removal of the fused map: the program that ends the reference's run, mapping/pcd_filter.cpp:44-66,95-99
 * (clusterFilter(0.03, ...) = pcl::EuclideanClusterExtraction with setMinClusterSize(200): the points whose cluster has at least 200
 * members stay, the flying pixels go) and :107-172 (remove_floor_pt: the floor is the most populated bin of a histogram of z at
 * res = 0.1, everything up to 0.1 above it is dropped and the floor becomes the zero of z), in ONE call on the device.  The call
 * takes ANY cloud of n_points rows, not only fgo_map_fuse_batch's xyz_out; colour and count are not arguments, the caller gathers
 * them through index_out.  PCL is not part of the reference tree, so the semantics below are THIS PROJECT'S DEFINITION, pinned to the
 * numpy restatement tests/map_clean_reference.py.  Everything that decides an outcome is integer arithmetic.  Where they differ
 * from the reference: it works in float, ours on the 2^-20 m quantum; its clamp of max_z to min_z + 2 (:124) feeds only n_bins, which
 * is printed and never used, so it bins EVERY point (:130-135) -- ours looks for the floor in the lowest floor_span only, which is
 * what that clamp was evidently for; its up axis is z, ours is a parameter (the camera's y points down).
 *   quantum     Q_k = llrint(x_k 2^20), ties to even, as in map fusion.  T = llrint(tolerance 2^20).  The cell of a point is
 *               c_k = floor(Q_k / T), floor division of the QUANTISED coordinate (Q = -1 is in cell -1), and its key
 *               ((c_z + 2^20) << 42) | ((c_y + 2^20) << 21) | (c_x + 2^20).  A point is OUT OF RANGE if a coordinate is not finite,
 *               if |x_k 2^20| >= 2^62 or if some |c_k| >= 2^20: reason 1, label -1, counted in n_out_of_range, and it takes no
 *               further part.  n_cells counts the occupied cells.
 *   link        two in-range points are linked iff dQ_x^2 + dQ_y^2 + dQ_z^2 <= T^2 in 64-bit integers: PCL's closed radius.
 *               Coincident points are linked.  The link is symmetric and exact; linked points lie in the same or in adjacent
 *               cells (27 cells); tolerance in [2^-20, 256] keeps every intermediate below 2^63.
 *   clusters    the connected components of the link graph, numbered 0, 1, ... in ascending order of their SMALLEST member's input
 *               index, the small ones too.  label_out[p] is that number, cluster_size_out[c] the size of cluster c, n_clusters
 *               their number.  A cluster is kept iff min_cluster_size <= size and (max_cluster_size == 0 or size <=
 *               max_cluster_size), both bounds included as in PCL; n_clusters_kept counts those.  The points of the others get
 *               reason 2; n_after_clusters points survive this stage.
 *   floor       only with remove_floor and n_after_clusters > 0 (else floor_bin = -1, floor_bin_points = 0, floor_height = 0), over
 *               the points that survived the cluster stage.  h_p = up_sign Q_up_axis(p), h_min their minimum.  R = llrint(floor_res
 *               2^20), S = llrint(floor_span 2^20), C = llrint(floor_clearance 2^20).  bin(p) = (h_p - h_min + R div 2) div R, and
 *               a point is counted only if h_p - h_min <= S.  floor_bin is the LOWEST index among the most populated bins (the
 *               reference's std::map walk with > does the same), floor_bin_points its count.  F = h_min + floor_bin R,
 *               floor_height = (double)F 2^-20.  A point is kept iff h_p > F + C, strictly; otherwise reason 3, counted in
 *               n_floor_removed.  The up-axis coordinate of a kept point's row of xyz_out is x - up_sign floor_height, one
 *               subtraction rounded once; the other two coordinates are copied bit for bit (all three without the floor stage).
 *   output      kept points have reason 0 and appear in ASCENDING INPUT INDEX: index_out their indices, xyz_out their rows,
 *               n_kept their number.  n_kept + n_floor_removed = n_after_clusters.
 * Two calls give bit-identical outputs.  Under a permutation of the input the kept SET, the partition and every count are the
 * same; labels and index_out map through the permutation.  Stateless, host arrays in and out; only the n_clusters sizes and the
 * n_kept rows are copied back.  FGO_EINVAL (before any HIP call): result NULL, n_points < 0 or >= 2^30, xyz NULL with n_points > 0,
 * tolerance outside [2^-20, 256] or not finite, min_cluster_size < 1, max_cluster_size < 0 or in [1, min_cluster_size), up_axis not
 * 0, 1 or 2, up_sign not +1 or -1, remove_floor not 0 or 1; and with remove_floor: floor_res outside [2^-20, 1024], floor_span < 0,
 * floor_span / floor_res > 4096, floor_clearance < 0, any of the three not finite.  n_points == 0: FGO_OK and a zero result with
 * floor_bin = -1.  FGO_ENODEV without a HIP device (no CPU fallback).  FGO_ENOMEM: the call needs about 170 bytes of device memory
 * per point. */
typedef struct {
  double tolerance;        /* 0.03 m   clusterFilter(0.03, ...)                       */
  int min_cluster_size;    /* 200      setMinClusterSize; 1 keeps every cluster        */
  int max_cluster_size;    /* 0 = no upper bound (PCL's default)                       */
  int remove_floor;        /* 1                                                        */
  int up_axis, up_sign;    /* 2, +1    height h = up_sign * coordinate[up_axis]        */
  double floor_res;        /* 0.1 m    res                                             */
  double floor_span;       /* 2.0 m    the floor is looked for in the lowest span      */
  double floor_clearance;  /* 0.1 m    keep h > floor + clearance                      */
} fgo_map_clean_params;
void fgo_map_clean_params_default(fgo_map_clean_params *p);   /* NULL tolerated */
typedef struct {
  int64_t n_points, n_out_of_range, n_cells, n_clusters, n_clusters_kept, n_after_clusters, n_floor_removed, n_kept;
  int64_t floor_bin /* -1: no floor stage */, floor_bin_points;
  double floor_height;
} fgo_map_clean_result;
int fgo_map_clean(int device, int64_t n_points, const double *xyz /* n x 3 */, const fgo_map_clean_params *params /* NULL = defaults */,
                  fgo_map_clean_result *result /* 1 */, int32_t *label_out /* n, may be NULL */, uint8_t *reason_out /* n, may be NULL */,
                  int32_t *cluster_size_out /* n (n_clusters written), may be NULL */,
                  int64_t *index_out /* n (n_kept written), may be NULL */, double *xyz_out /* n x 3 (n_kept rows), may be NULL */);
/* development: the device time of the last fgo_map_clean call by HIP events (quantise to compact), ms */
double fgo_debug_map_clean_kernel_ms(void);

/* k-nearest-neighbour surface normals of the map: the first half of mapping/pcd2mesh.cpp:52-67 (pcl::NormalEstimation with a kd-tree
 * and setKSearch(20): a surface normal and a curvature for every point; concatenateFields is the caller's, see write_ply in the
 * Python package), in ONE call on the device.  The greedy triangulation of the second half is a sequential front-growing algorithm
 * and out of scope.  The call takes ANY cloud of n_points rows; with neighbour_out it is a k-nearest-neighbour query of the cloud
 * on its own.  PCL is not part of the reference tree, so the semantics below are THIS PROJECT'S DEFINITION, pinned to the numpy
 * restatement tests/map_normals_reference.py.  Where they differ from PCL: distances are integers on the 2^-20 m quantum and ties
 * have a stated order; the neighbours lie within max_radius (PCL's k-search has no bound); the covariance is the exact integer
 * scatter, converted once.
 *   quantum     Q_k = llrint(x_k 2^20), ties to even, the product rounded on its own, as in map fusion and cleaning.  A point is
 *               IN RANGE iff every coordinate is finite and every |Q_k| < 2^34 (16384 m).  Any other point has status 1, is counted
 *               in n_out_of_range, is nobody's neighbour and has none: n_neighbours 0, its rows of neighbour_out and dist2_out
 *               all -1, of scatter_out 0.  The range does not depend on cell.  n_cells counts the occupied search cells
 *               (c_k = floor(Q_k / llrint(cell 2^20))): the only output that depends on cell.
 *   neighbours  the neighbours of the in-range point p are the first min(k, .) in-range points q, p ITSELF INCLUDED (as in PCL),
 *               in ascending order of the pair (d2, input index of q), where d2 = dQ_x^2 + dQ_y^2 + dQ_z^2, dQ = Q(q) - Q(p), in
 *               64-bit integers, among the points with d2 <= Rq^2, Rq = llrint(max_radius 2^20): the radius is closed, ties in d2
 *               go to the smaller input index.  n_neighbours_out[p] = m is their number; neighbour_out[p] and dist2_out[p] hold
 *               them in that order, the tail padded with -1.  With max_radius <= 16 and k <= 64 every integer here stays below 2^63.
 *   scatter     S1 = sum dQ, S2 = sum dQ dQ^T over the m neighbours, M = m S2 - S1 S1^T: exact in int64, whatever the order of
 *               summation.  scatter_out[p] is its upper triangle xx xy xz yy yz zz (for status 2 and 3 too).
 *   status      0 valid; 1 out of range; 2 few: m < 3 (whatever M is); 3 degenerate: m >= 3 and M is the zero matrix, that is, all
 *               neighbours coincide.  For 1, 2 and 3 the normal, the curvature and the eigenvalues are NaN.  n_valid, n_few and
 *               n_degenerate count status 0, 2 and 3.
 *   fit         for status 0: A_ij = (double)M_ij / ((double)(m m) 2^40), each entry converted once, then divided once: the
 *               covariance of the neighbours in m^2.  eigenvalues_out = l0 <= l1 <= l2 of A by 8 sweeps of the cyclic Jacobi
 *               rotation (pairs 01, 02, 12) every plane fit of this library uses; normal_out = the eigenvector e of l0 divided by
 *               sqrt((e_x e_x + e_y e_y) + e_z e_z); curvature_out = l0 / ((l0 + l1) + l2).  Sign: d_k = viewpoint_k -
 *               (double)Q_k 2^-20, s = (n_x d_x + n_y d_y) + n_z d_z; the normal is negated if s < 0, and if s == 0 exactly, if its
 *               first non-zero component is negative: n.(viewpoint - p) >= 0 always.  Every product, quotient and sum is rounded
 *               to double on its own: the kernel does not contract them.  Rounding may leave l0 a few ulps of l2 below zero.
 * Two calls give bit-identical outputs.  Every output but n_cells is bit-identical for every admissible cell: cell only tunes
 * the search.  Under a permutation of the input every output maps through the permutation exactly, provided that no point has a
 * tie in d2 at the place where its list ends.  Stateless, host arrays in and out.  FGO_EINVAL (before any HIP call): result NULL,
 * n_points < 0 or >= 2^30, xyz NULL with n_points > 0, normal_out, curvature_out, n_neighbours_out or status_out NULL with
 * n_points > 0, k outside [3, 64], max_radius outside [2^-20, 16] or not finite, cell outside [2^-6, 16] or not finite (so that
 * floor(Q / T_cell) fits the 21-bit cell fields), max_radius / cell > 16 (the search visits at most 17 rings of cells), a
 * viewpoint coordinate not finite.  n_points == 0: FGO_OK and a zero result.  FGO_ENODEV without a HIP device (no CPU fallback).
 * FGO_ENOMEM: the call needs about 200 bytes of device memory per point, and 12 k + 48 more with all optional outputs. */
typedef struct {
  int k;                 /* 20     setKSearch(20), pcd2mesh.cpp:59; the point itself is one of the k, as in PCL */
  double max_radius;     /* 0.16 m neighbours lie within this closed radius; PCL has no such bound (stated difference) */
  double cell;           /* 0.04 m side of the search cells: tuning only, NO output but n_cells depends on it */
  double viewpoint[3];   /* 0,0,0  PCL's default viewpoint: normals are turned towards it */
} fgo_map_normals_params;
void fgo_map_normals_params_default(fgo_map_normals_params *p);   /* NULL tolerated */
typedef struct { int64_t n_points, n_out_of_range, n_cells, n_valid, n_few, n_degenerate; } fgo_map_normals_result;
int fgo_map_normals(int device, int64_t n_points, const double *xyz /* n x 3 */, const fgo_map_normals_params *params /* NULL = defaults */,
                    fgo_map_normals_result *result /* 1 */,
                    double *normal_out /* n x 3 */, double *curvature_out /* n */, double *eigenvalues_out /* n x 3, may be NULL */,
                    int32_t *n_neighbours_out /* n */, uint8_t *status_out /* n */,
                    int32_t *neighbour_out /* n x k, may be NULL */, int64_t *dist2_out /* n x k, may be NULL */,
                    int64_t *scatter_out /* n x 6, may be NULL */);
/* development: the device time of the last fgo_map_normals call by HIP events (quantise to fit), ms */
double fgo_debug_map_normals_kernel_ms(void);

/* Z-buffer rendering of the map from trajectory poses, batched: what mapping/map_video.cpp, map_video_rs.cpp and map_video_sr.cpp do
 * with a VTK viewer -- for every pose of the trajectory a camera is placed relative to the sensor (eye (0, -2, -5), looking at
 * (0, 0, 5), up (0, -0.98, 0.199) in the camera frame, map_video.cpp:119-127,187), the accumulated map is drawn from there, and an
 * arc is flown round it at the end (:210-238) -- for ALL n_views in ONE call; and the map's self-check: the map drawn from a key
 * frame's own camera, with that frame's intrinsics, predicts the frame's depth image, and depth_meas is compared with it pixel by
 * pixel.  The call takes ANY cloud of n_points rows.  PCL and VTK are not part of the reference tree, so the semantics below are
 * THIS PROJECT'S DEFINITION, pinned to the numpy restatement tests/map_render_reference.py: a point is a square of pixels, a pixel
 * keeps the nearest point, everything after the projection is integer.  Lines, axes, the window, lens distortion, anti-aliasing,
 * shading and video encoding are out of scope.
 *   view        (R1, t1) = the rt of fgo_map_fuse_batch for pose_w7[v] and extrinsic7 (NULL = identity), bit for bit.  view_offset7
 *               (t_o, q_o; NULL = identity: then (R, t) = (R1, t1)) is a further pose composed on the right -- it carries the chase
 *               camera: with Ro the matrix of the normalised q_o as in the fusion, R_ij = (R1_i0 Ro_0j + R1_i1 Ro_1j) + R1_i2 Ro_2j
 *               and t_i = ((R1_i0 to_0 + R1_i1 to_1) + R1_i2 to_2) + t1_i.  This runs on the host, every operation rounded on its own,
 *               without fused multiply-adds; rt_out[v] = R row-major, then t: exactly what the kernel used.  The camera frame is x
 *               right, y down, z forward.
 *   point       a point with a non-finite coordinate is skipped and counted ONCE (not per view) in n_nonfinite.  d_k = x_k - t_k;
 *               p_k = (R_0k d_0 + R_1k d_1) + R_2k d_2 (R^T d); z = p_2; the point is VALID in the view iff z_min < z < z_max (the
 *               open interval of the project).  zq = llrint(z 2^20), ties to even.  uf = ((fx p_0) / z) + cx, vf = ((fy p_1) / z) + cy;
 *               the point is OFF-IMAGE (valid, not drawn) unless -2^30 < uf < 2^30 and -2^30 < vf < 2^30, compared in double (a NaN is
 *               off-image).  The centre is (u0, v0) = (floor(uf + 0.5), floor(vf + 0.5)).  The half-width is h = min(max_half,
 *               splat + s), with s = 0 unless radius > 0, then s = floor((fx radius) / z) (taken as max_half where it is larger, an
 *               infinite quotient included): a sphere of that radius at that depth.  The footprint is the square
 *               [u0 - h, u0 + h] x [v0 - h, v0 + h] clipped to the image.  EVERY product, quotient and sum is rounded to double
 *               on its own: the kernels do not contract them.
 *   pixel       its word is the MINIMUM over all points whose footprint covers it of ((uint64)zq << 32) | (uint32)index: the nearest
 *               point wins, ties on zq go to the smaller input index; an uncovered pixel is all ones.  zq_out = zq or -1, index_out =
 *               index or -1, color_out = the winner's colour or background[0 .. channels).
 *   depth check with depth_meas (NULL: the five counts are zero): zm = w z_scale for the measured word w, valid iff z_min < zm <
 *               z_max; mq = llrint(zm 2^20), tq = llrint(agree_tol 2^20).  Where a pixel is both measured and covered: it AGREES iff
 *               |mq - zq| <= tq; the measurement is CLOSER iff mq < zq - tq (something stands in front of the map); it goes THROUGH
 *               iff mq > zq + tq (the measurement sees through the map: a free-space violation, the signature of a wrong pose).
 *   counts      per view, int64: n_valid = valid points, n_drawn = valid points whose clipped footprint is not empty, n_pixels =
 *               covered pixels, n_meas = valid measured pixels, n_both = measured and covered, n_agree + n_closer + n_through = n_both.
 * result: n_points, n_nonfinite, form = FGO_MAP_RENDER_TILES or _GLOBAL, the kernel form that ran (no output depends on it), and
 * tile_rows = max(1, 8192 / width), the rows of a strip of the tiles form (0 in the global form).  An image wider than 8192 pixels
 * runs in the global form.  Two calls give bit-identical outputs; zq_out, color_out (where the pixel's minimum is unique) and every
 * count are invariant under a permutation of the points.  Each output array may be NULL: it is then neither allocated on the device
 * nor copied back.  Stateless, host arrays in and out, like fgo_map_fuse_batch.  FGO_EINVAL (before any HIP call): result NULL,
 * n_points or n_views < 0, n_points >= 2^31, width or height < 1 or their product > 2^24, n_views x width x height >= 2^31, channels
 * not 0, 1 or 3, fx, fy or z_scale <= 0 or not finite, cx or cy not finite, z_min < 0, z_max > 2047 (so that zq < 2^31), z_min >=
 * z_max, splat outside [0, 32], max_half outside [splat, 32], radius or agree_tol negative, not finite or > 2047, color_out not NULL
 * with channels == 0, pose_w7 NULL with n_views > 0, and with n_points > 0 xyz NULL, color NULL with channels > 0 or not NULL with
 * channels == 0; a zero (or non-finite) quaternion in pose_w7, extrinsic7 or view_offset7.  n_views == 0: FGO_OK and a zero result.
 * n_points == 0: every view is all background, with zero counts.  FGO_ENODEV without a HIP device (no CPU fallback).  FGO_ENOMEM:
 * the cloud, the requested outputs (4 + 4 + channels bytes per pixel and view) or, in the global form, the z-buffer do not fit. */
typedef struct {
  double fx, fy, cx, cy;   /* 250.5773, 250.5773, 90, 70: the SR4000 pinhole of fgo_map_params */
  double z_scale;          /* 0.001: metres per word of depth_meas */
  double z_min, z_max;     /* 0.1, 50: 0 <= z_min < z_max <= 2047 */
  int splat;               /* 0: half-width of every footprint in pixels, in [0, 32] */
  double radius;           /* 0.0 m: a point is a sphere of this radius (the map's leaf fills the holes); 0 = off */
  int max_half;            /* 8: the largest half-width, in [splat, 32] */
  double agree_tol;        /* 0.05 m */
  uint8_t background[3];   /* 0, 0, 26 */
} fgo_map_render_params;
void fgo_map_render_params_default(fgo_map_render_params *p);   /* NULL tolerated */
#define FGO_MAP_RENDER_TILES 0   /* a strip of a view per workgroup in an LDS z-buffer */
#define FGO_MAP_RENDER_GLOBAL 1  /* a device-wide z-buffer, one lane per (view, point) */
typedef struct { int64_t n_valid, n_drawn, n_pixels, n_meas, n_both, n_agree, n_closer, n_through; } fgo_map_render_view;
typedef struct { int64_t n_points, n_nonfinite; int form, tile_rows; } fgo_map_render_result;
int fgo_map_render_batch(int device, int64_t n_points, const double *xyz /* n x 3 */,
                         const uint8_t *color /* n x channels, NULL iff channels == 0 */, int channels /* 0, 1 or 3 */,
                         int64_t n_views, const double *pose_w7 /* V x 7: t(3) q_xyzw(4), as fgo_get_poses gives them */,
                         const double *extrinsic7 /* Pu2c, NULL = identity */, const double *view_offset7 /* NULL = identity */,
                         int width, int height, const fgo_map_render_params *params /* NULL = defaults */,
                         const uint16_t *depth_meas /* V x H x W, may be NULL */, fgo_map_render_result *result /* 1 */,
                         fgo_map_render_view *view_out /* V, may be NULL */, int32_t *zq_out /* V x H x W, may be NULL */,
                         int32_t *index_out /* V x H x W, may be NULL */, uint8_t *color_out /* V x H x W x channels, may be NULL */,
                         double *rt_out /* V x 12, may be NULL */);
/* development: the device time of the last fgo_map_render_batch call by HIP events (all kernels of the call), ms */
double fgo_debug_map_render_kernel_ms(void);

/* LevenbergMarquardtOptimizer(graph, values).optimize() with GTSAM 4.0's default parameters —
 *      CGraphGT::optimizeGraphBatch, gtsam/gtsam_graph.cpp:1784-1788.  max_iters <= 0 selects the default 100.
 *      Returns the number of iterations performed or a negative code. */
int fgo_optimize_gtsam(fgo_ctx *ctx, int max_iters, fgo_stats *stats /* may be NULL */);
/* ISAM2 semantics — CGraphGT::optimizeGraphIncremental, gtsam/gtsam_graph.cpp:1768-1776:
 *      isam2->update(new factors, new values);  values = isam2->calculateEstimate();
 *      with ISAM2Params{relinearizeThreshold (reference: 0.1), relinearizeSkip = 1} (:93-99) and the Gauss-Newton
 *      (undamped) step of ISAM2's default optimisation parameters.  "New" = everything added through fgo_add_* since the
 *      previous call.  The context keeps ISAM2's linearisation point theta and linear solution delta per variable; one
 *      call = { theta_v <- theta_v (+) delta_v, delta_v <- 0 for every variable with max|delta_v| >= threshold; linearise
 *      all factors at theta; solve H delta = b; values <- theta (+) delta }, i.e. what ISAM2's partial re-elimination
 *      computes with wildfireThreshold -> 0, evaluated as one full device sweep (the resident factorisation is rebuilt
 *      rather than edited; the structure phase reruns only when factors or variables were added).
 *      Returns 1, or a negative code (FGO_ENUM: system not positive definite; values, theta and delta are then as the
 *      relinearisation step left them).  stats->reserved[1] = number of variables relinearised; stats->reserved[3] = tasks of
 *      the elimination tree this update re-factored (-1: full sweep, -2: full sweep because most of the tree was affected);
 *      stats->reserved[4] = 1 if the back-substitution was cut by the wildfire threshold (fgo_isam2_set_wildfire), else 0.
 *      A structure built with landmarks eliminated (fgo_optimize_gtsam on a bundle-adjustment graph) cannot serve ISAM2:
 *      the first successful update switches the context to the generic form (one rebuild) until fgo_isam2_reset; a call
 *      that fails leaves that choice as it was. */
int fgo_isam2_update(fgo_ctx *ctx, double relinearize_threshold, fgo_stats *stats /* may be NULL */);
/* Growth reserve of the incremental mode.  A context that is driven through fgo_isam2_update builds its structure for
 * the graph PLUS `reserve_variables` phantom variables, each coupled to the `window` variables added before it: later
 * variables claim the phantom slots and later factors whose variable pairs lie inside that band (odometry, look-back,
 * IMU, plane and landmark factors of the newest key frames: gtsam/test_vro_imu_graph.cpp:159-350) are appended to the
 * device arrays in place -- no ordering, no symbolic factorisation, no re-upload; stats->structure_rebuilt stays 0 and
 * stats->t_symbolic is the host time of the in-place extension.  A factor outside the band (a far loop closure) or an
 * exhausted reserve triggers one ordinary rebuild (with a fresh reserve).  Defaults 384 / 64; reserve 0 disables. */
int fgo_isam2_reserve(fgo_ctx *ctx, int reserve_variables, int window);
/* The same growth reserve for g2o-semantics contexts: CGraphG2O::addNode adds key frames -- each matched against its
 * predecessor and the m_lookback_nodes before it (g2o/g2o_graph.cpp:159-239) -- between optimizeGraph() calls that come
 * every m_optimize_step key frames (g2o/test_g2o_graph.cpp:80-83).  g2o rebuilds its structure at every such call; here a
 * structure built in growth mode takes the new vertices into its reserve slots and the new edges (pairs inside the band
 * `window`) into its device arrays in place: fgo_optimize's stats->structure_rebuilt stays 0 and stats->t_symbolic is the
 * host time of the extension.  Growth mode switches itself on the first time a built structure has to be REBUILT because
 * vertices were added; fgo_set_growth(ctx, R, W) with R > 0 switches it on beforehand (W = 0: default band 16 >= 1 + m_lookback_nodes),
 * fgo_set_growth(ctx, 0, 0) switches it (and the automatic rule) off.  An edge outside the band (a far loop closure), a fixed new
 * vertex or an exhausted reserve costs one ordinary rebuild (with a fresh reserve).  The estimate does not depend on the mode
 * beyond rounding (another elimination order). */
int fgo_set_growth(fgo_ctx *ctx, int reserve_variables, int window);
/* ISAM2Params::wildfireThreshold analogue (gtsam/gtsam_graph.cpp:93-99 leaves GTSAM's default, 1e-3, in place).  0 (the
 * default here) = exact back-substitution of every variable at every update.  threshold > 0: below the top levels of the
 * elimination tree -- the re-factored root paths, always solved -- a task is solved again only if it was re-factored or an entry
 * of delta it depends on changed by >= threshold since the previous update; the others keep their delta.  Like GTSAM's, the
 * cut follows THIS elimination order, so the two approximations agree to the order of the threshold, not digit by digit.
 * The cut applies to an update only when (i) the update ran as a PARTIAL re-factorisation (stats->reserved[3] >= 0), (ii) the
 * schedule has a backward chain -- at least two panel levels at the top of the tree, single GPU -- and (iii) the previous
 * update left its solution behind; otherwise the call still returns FGO_OK and the back-substitution stays exact:
 * stats->reserved[4] of fgo_isam2_update says which of the two happened. */
int fgo_isam2_set_wildfire(fgo_ctx *ctx, double threshold);
/* delete mp_isam2; new ISAM2(params): forget theta and delta (the values stay).  Also leaves the incremental mode: the
 * growth reserve is dropped at the next use of the context and laid down again by the next fgo_isam2_update.  Batch
 * entry points (fgo_optimize_gtsam, marginals) called BETWEEN fgo_isam2_update calls keep the reserve (no structure
 * ping-pong in the reference's per-record flow); its cost is `reserve` identity columns coupled in a `window`-wide band. */
int fgo_isam2_reset(fgo_ctx *ctx);
/* ISAM2::getLinearizationPoint().at(key), ISAM2::getDelta()[key] (either output may be NULL) */
int fgo_isam2_get_state(fgo_ctx *ctx, int64_t id, double theta7[7], double delta6[6]);
/* NonlinearFactorGraph::error(values) = 0.5 * sum ||whitened r||^2 — CGraphGT::error, gtsam/gtsam_graph.cpp:173-176 */
double fgo_error(fgo_ctx *ctx);
/* Marginals(graph, values, Marginals::CHOLESKY).marginalCovariance(key) — gtsam/gtsam_graph.cpp:598-601: the 6x6
 *      (row-major, tangent order of the graph's semantics; 3-dof variables use the top-left 3x3) diagonal block of
 *      (J' Omega J)^-1 at the current estimate.  Works for both semantics. */
int fgo_marginal_cov(fgo_ctx *ctx, int64_t id, double *cov36);
/* Several blocks from ONE factorisation (the reference asks for many per Marginals object: gtsam/gtsam_graph.cpp:598-601,
 * :1357 + the commented-out association test :1429-1476): cov36 = n x 36 doubles.  The undamped factor stays resident in
 * HBM until the estimate or the structure changes, so consecutive calls do not re-factor either. */
int fgo_marginal_cov_many(fgo_ctx *ctx, int64_t n, const int64_t *ids, double *cov36);
/* SparseOptimizer::computeMarginals / Marginals for the whole map: the H^-1 diagonal blocks of EVERY free variable from one
 * selected inversion of the resident undamped factor (H^-1 on the block pattern of L, one reverse sweep over the factor's
 * level schedule).  Same semantics as fgo_marginal_cov; ids_out (n) / cov36_out (n x 36) in the order the variables were
 * added.  Returns the count n (ids_out / cov36_out may be NULL with cap 0 to query it), FGO_EINVAL if cap < n.  On a
 * bundle-adjustment graph the landmarks are included (the context switches to the generic form, like a landmark's
 * fgo_marginal_cov). */
int64_t fgo_marginal_cov_all(fgo_ctx *ctx, int64_t cap, int64_t *ids_out, double *cov36_out);
/* Cov(x_a, x_b) 6x6 row-major (rows: a's tangent, cols: b's); a == b is the marginal.  Pairs on the factor's pattern
 * (every pair sharing a factor is) come from the selected inverse; other pairs by column solves, grouped by b.
 * Marginals::jointMarginalCovariance is assembled from these blocks. */
int fgo_marginal_cov_pairs(fgo_ctx *ctx, int64_t n, const int64_t *id_a, const int64_t *id_b, double *cov36);
/* timings of the last selected inversion: [0] host seconds of the pair tables, [1] their bytes, [2] device ms of the undamped
 * factorisation, [3] of the prep kernel, [4] of the reverse sweep, [5] pair-table entries, [6] pairs of the last
 * fgo_marginal_cov_pairs call that were off the factor's pattern (served by column solves) */
int fgo_debug_selinv_stats(const fgo_ctx *ctx, double out[7]);
/* what a selected inversion of the built structure launches, from the host's column patterns, task tables and level schedule
 * (nothing is launched; FGO_ESTATE before the structure is built).  The reverse sweep runs a level as 16-wave workgroups (G = 160
 * lane groups per column) or 4-wave ones (G = 40): [0..5] for the 16-wave form, [6..11] for the 4-wave form: launches, workgroups
 * (= tasks), columns, largest m (off-diagonal blocks of a column), columns with m > G (the target loop wraps), most columns in
 * one task.  [12] block columns nb, [13] columns with m == 0, [14] workgroups of the prep kernel, [15] compute units of the device
 * (a level with fewer tasks than FGO_TUNE sinv_wide, by default this count, takes the 16-wave form). */
int fgo_debug_selinv_census(const fgo_ctx *ctx, int64_t out[16]);
/* ---- validating an edge BEFORE it enters the graph, inspecting edges afterwards.  The reference asks "is this constraint
 *      consistent with the map, given how uncertain the map is?" in several places and approximates the answer each time, because
 *      a Marginals object costs it a batch factorisation: the chi2_for_vro switch gates a visual-odometry edge with
 *      utils::chi2(N, 0.95) against an ad-hoc rotation-only information matrix (gtsam/test_vro_imu_graph.cpp:679-778); plane
 *      association builds a Marginals object and then has the J Sigma J' test commented out in favour of fixed thresholds
 *      (gtsam/gtsam_graph.cpp:1357-1470); a commented-out robust kernel is the only defence against a bad loop closure
 *      (g2o/g2o_graph.cpp:130).  Here the exact test is one call (fgo_gate_edges_se3 for pose-pose edges, fgo_gate_plane_factors /
 *      fgo_associate_planes below for plane observations).  For a candidate between a and b with measurement Z and
 *      information Omega (positive definite), at the current estimate: e, Ja, Jb as the linearisation computes them for a real
 *      edge of the context's semantics; chi2 = e' Omega e; P = [Ja Jb] Sigma_{ab,ab} [Ja Jb]' with Sigma = (J' Omega J)^-1 of
 *      the graph (the blocks fgo_marginal_cov_pairs returns; a fixed endpoint contributes zero blocks, both fixed: P = 0);
 *      d2 = e' (P + Omega^-1)^-1 e, the squared Mahalanobis distance of the innovation: chi-square with 6 degrees of freedom
 *      for a correct candidate that is not in the graph yet, 0 <= d2 <= chi2.  Accept when d2 < utils::chi2(6, 0.95) = 12.59.
 * n candidate SE3 edges at the current estimate; nothing is added to the graph.  d2_out[n]; chi2_out[n] and
 *      pred_cov36_out[n x 36] (P, row-major) may be NULL.  tangent_order must be the context's own semantics.
 *      FGO_EINVAL: unknown id, non-pose variable, a == b, foreign tangent order; FGO_ENUM: an information matrix is not positive
 *      definite (fgo_last_error names the first such candidate); FGO_ESTATE in distributed mode. */
int fgo_gate_edges_se3(fgo_ctx *ctx, int64_t n, const int64_t *id_a, const int64_t *id_b, const double *meas7,
                       const double *info_ut21, int tangent_order,
                       double *d2_out, double *chi2_out, double *pred_cov36_out);
/* e' Omega e of the SE3 edges already in the graph, [first, first + n) in the order they were added (g2o: edge->chi2()); needs no
 *      factorisation.  Single-GPU entry point like the gate. */
int fgo_edge_chi2_se3(fgo_ctx *ctx, int64_t first, int64_t n, double *chi2_out);
/* ---- the same test for a plane observation (GTSAM-semantics contexts): plane association is the one site where the reference
 *      builds a Marginals object live (gtsam/gtsam_graph.cpp:1357, for every key frame that carries planes), and the test it then
 *      has commented out (:1429-1476) drops the pose/plane cross-covariance, which accepts too much.  A candidate is a pose x, a
 *      plane p that is already a variable, a measurement z = (a, b, c, d) in the pose frame and its 3x3 covariance S (upper
 *      triangle), both taken exactly as fgo_add_plane_factor takes them (the normal of z is normalised, d is not touched).  At the
 *      current estimate: e (3), Jx (3x6), Jp (3x3) as the linearisation computes them for a real OrientedPlane3Factor;
 *      chi2 = e' S^-1 e; P = Jx Sxx Jx' + Jx Sxp Jp' + Jp Sxp' Jx' + Jp Spp Jp' with the blocks of Sigma fgo_marginal_cov_pairs
 *      returns (of a plane's padded block only the leading 3x3 / 6x3 part is read; a fixed endpoint contributes zero blocks, both
 *      fixed: P = 0, no factorisation); d2 = e' (P + S)^-1 e, chi-square with 3 degrees of freedom for a correct association,
 *      0 <= d2 <= chi2; cos = n' . n_z, the cosine between the predicted and the measured normal.  Accept when
 *      d2 < utils::chi2(3, 0.95) = 7.815.  Nothing is added to the graph; the context is left as fgo_marginal_cov_pairs on the
 *      same id pairs leaves it.
 * n candidates.  d2_out[n]; chi2_out[n], cos_out[n], resid3_out[n x 3] (e) and pred_cov9_out[n x 9] (P, row-major) may be NULL.
 *      FGO_EINVAL: unknown id, pose_id not a pose, plane_id not a plane, zero normal, g2o-semantics context; FGO_ENUM: S (or
 *      P + S) is not positive definite (fgo_last_error names the first such candidate); FGO_ESTATE in distributed mode. */
int fgo_gate_plane_factors(fgo_ctx *ctx, int64_t n, const int64_t *pose_id, const int64_t *plane_id, const double *z_abcd,
                           const double *cov_ut6, double *d2_out, double *chi2_out, double *cos_out, double *resid3_out,
                           double *pred_cov9_out);
/* The association loop of gtsam/gtsam_graph.cpp:1367-1479 as one call: k observations (z_abcd k x 4, cov_ut6 k x 6) made from
 *      pose_id against the m distinct planes plane_ids; all k m candidates are evaluated on the device.  A candidate with
 *      cos < cos_min (the reference's COSA < COS10, :1409; -1 disables it) or whose S or P + S is not positive definite is
 *      excluded.  Per observation the smallest and the second smallest d2 are reduced on the device, going through plane_ids from
 *      its first entry to its last; a tie goes to the earlier entry.  match_out[k] = the plane of the smallest d2 if that is
 *      < d2_gate, else -1; best2_out[k x 2] = smallest, second smallest d2 (+inf when absent: the runner-up shows ambiguity);
 *      d2_matrix_out[k x m] (may be NULL) = every d2, +inf where the candidate was excluded.  Observations are matched independently
 *      of one another, as the reference does.  k = 0: nothing is written; m = 0: match -1, best2 +inf.  Errors as above, and
 *      FGO_EINVAL for a plane listed twice. */
int fgo_associate_planes(fgo_ctx *ctx, int64_t pose_id, int64_t k, const double *z_abcd, const double *cov_ut6, int64_t m,
                         const int64_t *plane_ids, double d2_gate, double cos_min, int64_t *match_out, double *best2_out,
                         double *d2_matrix_out);
/* the last gate call of either kind: [0] its candidates whose cross-covariance block was off the factor's pattern, [1] column
 *      groups solved for them, [2] device ms of the gate kernel (and the association's reduction), [3] device ms of those column
 *      solves */
int fgo_debug_gate_stats(const fgo_ctx *ctx, double out[4]);

/* ---- solve: ONE SparseOptimizer::optimize(max_iters) call as issued by
 *      CGraphG2O::optimizeGraph (g2o/g2o_graph.cpp:246-249).  Returns the number of LM iterations
 *      performed (>= 1), FGO_ESTATE if there is nothing to optimise, or another negative code. */
int fgo_optimize(fgo_ctx *ctx, int max_iters, fgo_stats *stats /* may be NULL */);
/* computeActiveErrors(); chi2()  — CGraphG2O::error, g2o/g2o_graph.cpp:254-258 (no 1/2).  NaN on error. */
double fgo_chi2(fgo_ctx *ctx);
/* per-iteration (chi2, lambda) of the last fgo_optimize call; returns the number written */
int fgo_trace(const fgo_ctx *ctx, double *chi2s, double *lambdas, int cap);

/* ---- building blocks exposed for parity tests and profiling (same device kernels the solve uses).
 * fgo_linearize: computeActiveErrors + buildSystem at the current estimate; optional outputs are the
 * dense (6*n_free)^2 row-major H and 6*n_free b in free-variable order = order in which the variables were added (small graphs
 * only: n_free <= 4096).  fgo_solve_step: one damped solve (H + lambda I) d = b, d returned in the same
 * order.  n_free counts the CALLER's free variables only (fgo_stats.n_free, *n_free_out): the phantom slots a context in
 * incremental mode keeps behind them (fgo_isam2_reserve) are internal and never appear in H_dense, b_dense or delta_out,
 * so buffers sized from the caller's own free-variable count are always large enough; landmarks a bundle-adjustment structure
 * eliminates analytically DO count (asking for the dense system switches the context to the generic form).  fgo_bench_phase: repeats one phase as an LM trial runs it (0 linearize, 1 factor sweep with
 * the forward solve fused in, 2 backward solve sweep) 'reps' times on the context's stream and returns the mean device ms
 * per repetition. */
int fgo_linearize(fgo_ctx *ctx, double *chi2_out, double *H_dense, double *b_dense, int64_t *n_free_out);
int fgo_solve_step(fgo_ctx *ctx, double lambda, double *delta_out);
int fgo_bench_phase(fgo_ctx *ctx, int phase, int reps, double *ms_out);
int fgo_get_stats(const fgo_ctx *ctx, fgo_stats *stats);       /* structure fields of the last build */

/* ---- synthetic pose graphs (SURVEY.md §8d "Manhattan-3D"); host-only, no device needed.
 * Lattice random walk, odometry + `lookback` look-back edges per pose as CGraphG2O::addNode builds
 * them (g2o/g2o_graph.cpp:196-205) + up to `n_loop` loop closures to earlier poses within 2 m.
 * Outputs must hold n_poses*7 / max_edges*{1,1,7,21} entries; returns the edge count (or <0). */
int64_t fgo_synth_manhattan3d(int64_t n_poses, int lookback, int n_loop, uint64_t seed, double sigma_t,
                              double sigma_q, double *poses_init7, double *poses_true7, int64_t *id_i,
                              int64_t *id_j, double *meas7, double *info_ut21, int64_t max_edges);

/* ---- multi-GPU: distributed factorisation by domain decomposition (north star: "the graph shards by
 * pose-block column across up to 8 GPUs with RCCL all-reduce ... on the off-diagonal Hessian contributions").
 * The reference's only solve site is single-threaded (g2o/g2o_graph.cpp:246-249).  Here every rank holds the whole graph
 * (host side) and calls the same entry points in the same order -- fgo_optimize* and fgo_chi2 become COLLECTIVE calls.
 * fgo_set_shard(rank, world) cuts the elimination tree into `world` groups of sub-trees ("domains": contiguous ranges of
 * block columns, one group per rank) plus their common ancestors (the "top": the upper nested-dissection separators).
 * A rank linearises only the factors of its domain, factors only its own block columns (with the forward solve fused),
 * and adds its updates into the top's blocks of L and entries of the right-hand side; ONE all-reduce per LM trial sums
 * those contributions -- exactly the Hessian blocks and updates that cross from a domain's columns into the separator
 * columns -- then every rank finishes the (small, latency-bound) top redundantly, back-substitutes through the top and
 * its own domain, updates its poses and re-linearises.  Scalars (chi2, the LM scale, lambda_0) are summed / maximised
 * over the ranks, so all ranks take identical accept / reject decisions.  At the end of an optimize call the ranks'
 * poses are gathered, so fgo_get_pose* answers with the whole estimate on every rank.
 * Transport: fgo_dist_init_rccl (RCCL on the context's stream: no host callback, no extra synchronisation), or a
 * host callback (fgo_set_allreduce: tests, torch.distributed) that must sum a device buffer over the ranks in place.
 * ISAM2 updates, marginal covariances and fgo_solve_step are single-GPU entry points (FGO_ESTATE when world > 1).
 * Errors: fgo_optimize* first agree on a status word, so a rank whose structure build failed (or that has nothing to
 * optimise) makes ALL ranks return an error instead of leaving them blocked in a collective; numerical failures inside
 * the LM loop are agreed through the scalar collective.  A HIP or transport error in the middle of a trial is fatal for
 * the communicator (the other ranks may block): destroy the contexts. */
typedef int (*fgo_allreduce_fn)(void *user, double *device_buffer, int64_t count);
int fgo_set_shard(fgo_ctx *ctx, int rank, int world);
int fgo_set_allreduce(fgo_ctx *ctx, fgo_allreduce_fn fn, void *user);
/* RCCL transport: rank 0 obtains a 128-byte id (ncclGetUniqueId), the host program broadcasts it to all ranks by any means,
 * every rank calls fgo_dist_init_rccl after fgo_set_shard (ncclCommInitRank; one GPU per rank).  librccl is loaded at
 * run time (FGO_RCCL_LIB overrides the name), so single-GPU deployments do not need it.  An id serves ONE communicator
 * (one rendezvous): a second context, or a context that is re-initialised, draws and broadcasts a new one. */
int fgo_dist_unique_id(void *id128);
int fgo_dist_init_rccl(fgo_ctx *ctx, const void *id128);
/* tests: the decomposition for a block graph (host only; group_out[v] = owning rank, `world` = top); one all-reduce of
 * host data through the context's transport */
int fgo_debug_partition(int n, int64_t n_pairs, const int *a, const int *b, int world, int *group_out);
int fgo_debug_allreduce(fgo_ctx *ctx, double *host_buffer, int64_t count);
/* contiguous shard [lo, hi) of n items for rank r of w (host-only helper, also used internally) */
int fgo_shard_range(int64_t n, int rank, int world, int64_t *lo, int64_t *hi);
/* profiling hook: the first `count` doubles of the device-side reduction scratch (FGO_TRI_PROF=1 makes single-panel
 * k_panel_tri launches leave shader-clock stamps of their phases there: tools/tri_prof.py) */
int fgo_debug_read_scratch(fgo_ctx *ctx, double *out, int64_t count);
/* debugging / tests: copy the current (partial or full) H blocks, b and chi2 to the host.
 * H: n_hblocks*36 doubles (fgo_stats.nnz_H_blocks), b: 6*n_free doubles.  FGO_ESTATE on a structure that carries the
 * growth reserve of the incremental mode. */
int fgo_debug_read_system(fgo_ctx *ctx, double *H, double *b, double *chi2);
/* tests: the REDUCED camera system of a structure whose Point3 landmarks are eliminated first (the Schur complement GTSAM's
 * multifrontal elimination forms for gtsam/gtsam_graph.cpp:370-448 graphs): S = H_cc - W (H_pp + lambda I)^-1 W^T,
 * g = b_c - W (H_pp + lambda I)^-1 b_p at the current estimate, dense row-major (6 n)^2 / 6 n with n = *n_out = the free
 * non-landmark variables in the order they were added (n <= 4096).  FGO_ESTATE if no landmarks are eliminated. */
int fgo_debug_read_reduced(fgo_ctx *ctx, double lambda, double *H_dense, double *b_dense, int64_t *n_out);
/* tests: one damped solve (H + lambda I) d = b as an LM trial runs it -- the forward solve fused into the factor sweep, then the
 * backward sweep alone -- where fgo_solve_step runs the stand-alone forward kernels.  d in the order of fgo_solve_step, same
 * refusals (FGO_ESTATE in distributed mode; phantom slots of the incremental mode are not reported). */
int fgo_debug_solve_fused(fgo_ctx *ctx, double lambda, double *delta_out);
/* tests: which kernel instantiations one factor + solve of the built structure launches, without launching anything (the launchers
 * are walked with their launches switched off).  fused != 0: as fgo_debug_solve_fused / an LM trial, 0: as fgo_solve_step.
 * launches / workgroups / items: per instantiation, the first form_cap of them (items: the targets -- gather form -- or groups --
 * column-group form -- of an accumulate launch, without the forward-solve workgroups that ride in it and without padding; for
 * every other instantiation its workgroups); fused == 2: the factor sweep as the last fgo_isam2_update ran it; level_riders / level_long: per schedule level
 * (fgo_stats.n_levels), rider items carried by the level's triangle and row launches / long-list targets of its accumulate launch;
 * chain2[0]: the backward chain is on, chain2[1]: its mode; names: the instantiations' names, one per line (NUL-terminated).
 * Any output may be NULL.  Returns the number of instantiations (>= 0) or an error (< 0). */
int fgo_debug_launch_census(fgo_ctx *ctx, int fused, int64_t *launches, int64_t *workgroups, int64_t *items, int form_cap, int *level_riders,
                            int *level_long, int level_cap, int *chain2, char *names, int names_cap);
/* tests: what the last fgo_isam2_update on this context ran.  info5: {sweep (0 full, 1 masked: dirty flags on full grids, 2 ranged),
 * back-substitution cut (0 / 1), schedule levels, tasks, first level of the backward chain (-1: none)}.  Per level (the first level_cap): the task range [lo, hi] the factor sweep
 * launched (hi < lo: none; the whole level unless the sweep was ranged), the level's task count, the forward-solve workgroups
 * that rode in its accumulate launch and whether they came from the level's work-item table (both as the launcher itself records them).  Per task (the first task_cap):
 * its level, whether it was re-factored, and -- after a cut back-substitution -- whether it was solved again (1 for every task
 * otherwise, and for the tasks of the backward chain, which are always solved).  Per variable, in the order the variables were
 * added, phantom slots left out (the first var_cap): its task (-1: fixed), whether the cut found its delta moved by >= the
 * wildfire threshold (0 when nothing was cut), and its delta (6 doubles).  Any output may be NULL.  fgo_debug_launch_census with
 * fused == 2 walks the factor sweep of the same update (FGO_ESTATE if it was a full sweep).  Returns the number of variables the
 * ISAM2 state covers (>= 0) or an error (< 0); FGO_ESTATE before the first update / after a change of structure. */
int fgo_debug_isam_last(fgo_ctx *ctx, int *info5, int *level_lo, int *level_hi, int *level_ntask, int *level_fwd, int *level_fwtab, int level_cap,
                        int *task_level,
                        unsigned char *task_dirty, unsigned char *task_run, int task_cap, int *var_task, unsigned char *var_chg,
                        double *var_delta, int64_t var_cap);
/* tests: what the next linearisation of this context launches, as counts copied from the context and its device plan (the structure
 * is brought up to date first, as by every other call; nothing is launched).  out[0..11]: hub entries (one workgroup each), distinct
 * hub variables, hubs of more than one slice (what k_hub_combine* runs on), the degree above which a variable is a hub, hub entries
 * the scratch buffers hold; duplicate groups and the factors in them; unary priors on the device; unclaimed phantom slots of the
 * growth reserve; colour slots of the IMU factors (64 + the factors with a colour of their own); whether the masked ISAM2 linearisation applies (GTSAM
 * semantics only); whether the last structure phase was a build (1) or an in-place extension (0). */
int fgo_debug_linearize_census(fgo_ctx *ctx, int64_t out[12]);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FGO_H */
