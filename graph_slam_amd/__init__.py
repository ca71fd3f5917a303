"""graph_slam_amd — MI355X-native batch factor-graph optimiser behind the graph_slam C++ surface.

The product is the C-ABI shared library ``libfgo.so`` (``include/fgo.h``): hand-written HIP kernels for
gfx950 + a C++ host.  This Python module is only a ctypes binding used by the tests and ``bench.py``.
There is NO CPU fallback: if the library is missing this import raises, and if no HIP device is
present ``Graph()`` raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FGO_LIB", os.path.join(_HERE, "libfgo.so"))      # (FGO_LIB: developer A/B of two builds on the same GPU box)

FGO_TANGENT_G2O = 0
FGO_TANGENT_GTSAM = 1


class FgoConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("verbose", C.c_int), ("ordering", C.c_int), ("nd_leaf", C.c_int), ("order_candidates", C.c_int),
                ("reserved", C.c_int * 11)]


class FgoStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("trials", C.c_int), ("terminated", C.c_int), ("structure_rebuilt", C.c_int),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double),
                ("t_symbolic", C.c_double), ("t_upload", C.c_double), ("t_total", C.c_double),
                ("ms_linearize", C.c_double), ("ms_factor", C.c_double), ("ms_solve", C.c_double), ("ms_update", C.c_double),
                ("n_free", C.c_int64), ("n_edges", C.c_int64), ("nnz_H_blocks", C.c_int64), ("nnz_L_blocks", C.c_int64),
                ("n_update_ops", C.c_int64), ("n_levels", C.c_int), ("n_tasks", C.c_int),
                ("bytes_factor", C.c_double), ("bytes_linearize", C.c_double), ("bytes_solve", C.c_double),
                ("reserved", C.c_double * 8)]

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if name == "reserved" else v
        return d


class TwoViewParams(C.Structure):
    """fgo_two_view_params"""
    _fields_ = [("pose_prior_sigma", C.c_double), ("point_sigma", C.c_double), ("pixel_sigma", C.c_double),
                ("max_iters", C.c_int), ("min_matches", C.c_int)]


class TwoViewResult(C.Structure):
    """fgo_two_view_result"""
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("trials", C.c_int),
                ("error_initial", C.c_double), ("error_final", C.c_double), ("lambda_final", C.c_double)]


FGO_TV_OK, FGO_TV_TOO_FEW, FGO_TV_NUM = 0, 1, 2


class PlaneCheckParams(C.Structure):
    """fgo_plane_check_params"""
    _fields_ = [("cos_min", C.c_double), ("d_max", C.c_double), ("failed_info00", C.c_double)]


class PlaneCheckResult(C.Structure):
    """fgo_plane_check_result"""
    _fields_ = [("status", C.c_int), ("n_matched", C.c_int), ("n_bad", C.c_int), ("best_i", C.c_int), ("best_j", C.c_int),
                ("reserved", C.c_int), ("err", C.c_double), ("err_raw", C.c_double)]


FGO_PC_OK, FGO_PC_SKIPPED, FGO_PC_NUM = 0, 1, 2


class ImuCheckParams(C.Structure):
    """fgo_imu_check_params"""
    _fields_ = [("d2_gate", C.c_double), ("d2_ref_gate", C.c_double), ("failed_info00", C.c_double)]


class ImuCheckResult(C.Structure):
    """fgo_imu_check_result"""
    _fields_ = [("status", C.c_int), ("reject", C.c_int), ("d2", C.c_double), ("d2_ref", C.c_double), ("angle", C.c_double)]


FGO_IC_OK, FGO_IC_SKIPPED, FGO_IC_NUM = 0, 1, 2


class VroParams(C.Structure):
    """fgo_vro_params"""
    _fields_ = [("hypotheses", C.c_int), ("seed", C.c_uint64), ("max_dist", C.c_double), ("min_side", C.c_double),
                ("rigid_tol", C.c_double), ("refine_rounds", C.c_int), ("min_inliers", C.c_int), ("fx", C.c_double), ("fy", C.c_double),
                ("sigma_px", C.c_double), ("sigma_z", C.c_double * 3)]


class VroResult(C.Structure):
    """fgo_vro_result"""
    _fields_ = [("status", C.c_int), ("n_inliers", C.c_int), ("best_hypothesis", C.c_int), ("best_count", C.c_int),
                ("n_valid", C.c_int), ("rounds", C.c_int), ("rmse", C.c_double)]


FGO_VRO_OK, FGO_VRO_TOO_FEW, FGO_VRO_NUM = 0, 1, 2


class PlaneExtractParams(C.Structure):
    """fgo_plane_extract_params"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("z_scale", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("hypotheses", C.c_int), ("seed", C.c_uint64), ("max_dist", C.c_double),
                ("min_area", C.c_double), ("min_pixels", C.c_int), ("max_planes", C.c_int), ("refine_rounds", C.c_int),
                ("sigma_px", C.c_double), ("sigma_z", C.c_double * 3)]


class PlaneExtractResult(C.Structure):
    """fgo_plane_extract_result"""
    _fields_ = [("status", C.c_int), ("n_planes", C.c_int), ("n_valid_pixels", C.c_int), ("rounds_run", C.c_int)]


class PlaneExtractPlane(C.Structure):
    """fgo_plane_extract_plane"""
    _fields_ = [("n_pixels", C.c_int), ("best_hypothesis", C.c_int), ("best_count", C.c_int), ("n_valid_hyp", C.c_int),
                ("fits", C.c_int), ("reserved", C.c_int), ("rmse", C.c_double), ("centroid", C.c_double * 3)]


FGO_PX_OK, FGO_PX_NUM = 0, 2
FGO_PX_MAX_PLANES = 8


class PlanePropagateParams(C.Structure):
    """fgo_plane_propagate_params"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("z_scale", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("sigma_px", C.c_double), ("sigma_z", C.c_double * 3),
                ("d_floor", C.c_double), ("intensity_tol", C.c_int), ("keep_ratio", C.c_double), ("rest_ratio", C.c_double)]


class PlanePropagateResult(C.Structure):
    """fgo_plane_propagate_result"""
    _fields_ = [("status", C.c_int), ("n_planes", C.c_int), ("num_added", C.c_int), ("search_rest", C.c_int)]


class PlanePropagatePlane(C.Structure):
    """fgo_plane_propagate_plane"""
    _fields_ = [("n_pixels", C.c_int), ("n_seed", C.c_int), ("source", C.c_int), ("reserved", C.c_int), ("rmse", C.c_double),
                ("centroid", C.c_double * 3)]


class PlanePropagatePred(C.Structure):
    """fgo_plane_propagate_pred"""
    _fields_ = [("abcd", C.c_double * 4), ("sdj", C.c_double), ("n_prev", C.c_int), ("n_seed", C.c_int), ("kept", C.c_int),
                ("reserved", C.c_int)]


FGO_PP_OK, FGO_PP_NUM = 0, 2


class MatchParams(C.Structure):
    """fgo_match_params"""
    _fields_ = [("ratio", C.c_double), ("ratio_test", C.c_int), ("cross_check", C.c_int), ("max_desc_dist2", C.c_int32),
                ("min_matches", C.c_int), ("radius_px", C.c_double), ("max_dist_3d", C.c_double), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double)]


class MatchResult(C.Structure):
    """fgo_match_result"""
    _fields_ = [("status", C.c_int), ("n_query", C.c_int), ("n_train", C.c_int), ("n_matches", C.c_int), ("n_ratio", C.c_int),
                ("n_cross", C.c_int)]


FGO_FM_OK, FGO_FM_TOO_FEW = 0, 1
FGO_FM_DIM, FGO_FM_MAX_FEATURES = 128, 4096


class MapParams(C.Structure):
    """fgo_map_params"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("z_scale", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("skip", C.c_int), ("rect", C.c_int * 4), ("leaf", C.c_double),
                ("min_points", C.c_int), ("table_log2", C.c_int)]


class MapResult(C.Structure):
    """fgo_map_result"""
    _fields_ = [("status", C.c_int), ("table_log2", C.c_int), ("n_sampled", C.c_int64), ("n_valid", C.c_int64),
                ("n_out_of_range", C.c_int64), ("n_voxels", C.c_int64), ("n_dropped", C.c_int64)]


FGO_MAP_OK, FGO_MAP_TRUNCATED, FGO_MAP_FULL = 0, 1, 2


class MapCleanParams(C.Structure):
    """fgo_map_clean_params"""
    _fields_ = [("tolerance", C.c_double), ("min_cluster_size", C.c_int), ("max_cluster_size", C.c_int), ("remove_floor", C.c_int),
                ("up_axis", C.c_int), ("up_sign", C.c_int), ("floor_res", C.c_double), ("floor_span", C.c_double),
                ("floor_clearance", C.c_double)]


class MapCleanResult(C.Structure):
    """fgo_map_clean_result"""
    _fields_ = [("n_points", C.c_int64), ("n_out_of_range", C.c_int64), ("n_cells", C.c_int64), ("n_clusters", C.c_int64),
                ("n_clusters_kept", C.c_int64), ("n_after_clusters", C.c_int64), ("n_floor_removed", C.c_int64), ("n_kept", C.c_int64),
                ("floor_bin", C.c_int64), ("floor_bin_points", C.c_int64), ("floor_height", C.c_double)]


class MapNormalsParams(C.Structure):
    """fgo_map_normals_params"""
    _fields_ = [("k", C.c_int), ("max_radius", C.c_double), ("cell", C.c_double), ("viewpoint", C.c_double * 3)]


class MapNormalsResult(C.Structure):
    """fgo_map_normals_result"""
    _fields_ = [("n_points", C.c_int64), ("n_out_of_range", C.c_int64), ("n_cells", C.c_int64), ("n_valid", C.c_int64),
                ("n_few", C.c_int64), ("n_degenerate", C.c_int64)]


class MapRenderParams(C.Structure):
    """fgo_map_render_params"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("z_scale", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("splat", C.c_int), ("radius", C.c_double), ("max_half", C.c_int),
                ("agree_tol", C.c_double), ("background", C.c_uint8 * 3)]


class MapRenderView(C.Structure):
    """fgo_map_render_view"""
    _fields_ = [(f, C.c_int64) for f in ("n_valid", "n_drawn", "n_pixels", "n_meas", "n_both", "n_agree", "n_closer", "n_through")]


class MapRenderResult(C.Structure):
    """fgo_map_render_result"""
    _fields_ = [("n_points", C.c_int64), ("n_nonfinite", C.c_int64), ("form", C.c_int), ("tile_rows", C.c_int)]


FGO_MAP_RENDER_TILES, FGO_MAP_RENDER_GLOBAL = 0, 1


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)     # fgo_allreduce_fn


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "graph_slam_amd: %s is missing — build it with `python -m graph_slam_amd.build` "
            "(hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    dp, ip, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int64)
    lib.fgo_create.restype = C.c_void_p
    lib.fgo_create.argtypes = [C.POINTER(FgoConfig)]
    lib.fgo_destroy.argtypes = [C.c_void_p]
    lib.fgo_last_error.restype = C.c_char_p
    lib.fgo_last_error.argtypes = [C.c_void_p]
    lib.fgo_version.restype = C.c_char_p
    lib.fgo_device_count.restype = C.c_int
    lib.fgo_add_pose.argtypes = [C.c_void_p, C.c_int64, dp, dp, C.c_int]
    lib.fgo_set_pose.argtypes = [C.c_void_p, C.c_int64, dp, dp]
    lib.fgo_get_pose.argtypes = [C.c_void_p, C.c_int64, dp]
    lib.fgo_has_pose.argtypes = [C.c_void_p, C.c_int64]
    lib.fgo_num_poses.restype = C.c_int64
    lib.fgo_num_poses.argtypes = [C.c_void_p]
    lib.fgo_num_edges.restype = C.c_int64
    lib.fgo_num_edges.argtypes = [C.c_void_p]
    lib.fgo_add_poses.argtypes = [C.c_void_p, C.c_int64, i64p, dp, C.POINTER(C.c_ubyte)]
    lib.fgo_get_poses.argtypes = [C.c_void_p, C.c_int64, i64p, dp]
    lib.fgo_add_edge_se3.argtypes = [C.c_void_p, C.c_int64, C.c_int64, dp, dp, dp, C.c_int]
    lib.fgo_add_edges_se3.argtypes = [C.c_void_p, C.c_int64, i64p, i64p, dp, dp, C.c_int]
    lib.fgo_optimize.argtypes = [C.c_void_p, C.c_int, C.POINTER(FgoStats)]
    lib.fgo_chi2.restype = C.c_double
    lib.fgo_chi2.argtypes = [C.c_void_p]
    lib.fgo_trace.argtypes = [C.c_void_p, dp, dp, C.c_int]
    lib.fgo_linearize.argtypes = [C.c_void_p, dp, dp, dp, i64p]
    lib.fgo_solve_step.argtypes = [C.c_void_p, C.c_double, dp]
    lib.fgo_bench_phase.argtypes = [C.c_void_p, C.c_int, C.c_int, dp]
    lib.fgo_get_stats.argtypes = [C.c_void_p, C.POINTER(FgoStats)]
    lib.fgo_synth_manhattan3d.restype = C.c_int64
    lib.fgo_synth_manhattan3d.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_uint64, C.c_double, C.c_double,
                                          dp, dp, i64p, i64p, dp, dp, C.c_int64]
    lib.fgo_shard_range.argtypes = [C.c_int64, C.c_int, C.c_int, i64p, i64p]
    lib.fgo_add_prior_pose.argtypes = [C.c_void_p, C.c_int64, dp, dp, dp]
    lib.fgo_optimize_gtsam.argtypes = [C.c_void_p, C.c_int, C.POINTER(FgoStats)]
    lib.fgo_error.restype = C.c_double
    lib.fgo_isam2_update.argtypes = [C.c_void_p, C.c_double, C.POINTER(FgoStats)]
    lib.fgo_isam2_reset.argtypes = [C.c_void_p]
    lib.fgo_isam2_get_state.argtypes = [C.c_void_p, C.c_int64, dp, dp]
    lib.fgo_error.argtypes = [C.c_void_p]
    lib.fgo_marginal_cov.argtypes = [C.c_void_p, C.c_int64, dp]
    lib.fgo_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.fgo_set_allreduce.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p]
    lib.fgo_isam2_reserve.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.fgo_set_growth.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.fgo_isam2_set_wildfire.argtypes = [C.c_void_p, C.c_double]
    lib.fgo_marginal_cov_many.argtypes = [C.c_void_p, C.c_int64, i64p, dp]
    lib.fgo_marginal_cov_all.restype = C.c_int64
    lib.fgo_marginal_cov_all.argtypes = [C.c_void_p, C.c_int64, i64p, dp]
    lib.fgo_marginal_cov_pairs.argtypes = [C.c_void_p, C.c_int64, i64p, i64p, dp]
    lib.fgo_debug_selinv_stats.argtypes = [C.c_void_p, dp]
    lib.fgo_debug_selinv_census.argtypes = [C.c_void_p, i64p]
    lib.fgo_gate_edges_se3.argtypes = [C.c_void_p, C.c_int64, i64p, i64p, dp, dp, C.c_int, dp, dp, dp]
    lib.fgo_edge_chi2_se3.argtypes = [C.c_void_p, C.c_int64, C.c_int64, dp]
    lib.fgo_debug_gate_stats.argtypes = [C.c_void_p, dp]
    lib.fgo_gate_plane_factors.argtypes = [C.c_void_p, C.c_int64, i64p, i64p, dp, dp, dp, dp, dp, dp, dp]
    lib.fgo_associate_planes.argtypes = [C.c_void_p, C.c_int64, C.c_int64, dp, dp, C.c_int64, i64p, C.c_double, C.c_double, i64p, dp, dp]
    lib.fgo_dist_unique_id.argtypes = [C.c_void_p]
    lib.fgo_dist_init_rccl.argtypes = [C.c_void_p, C.c_void_p]
    lib.fgo_debug_partition.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    lib.fgo_debug_allreduce.argtypes = [C.c_void_p, dp, C.c_int64]
    lib.fgo_debug_read_system.argtypes = [C.c_void_p, dp, dp, dp]
    lib.fgo_debug_read_reduced.argtypes = [C.c_void_p, C.c_double, dp, dp, i64p]
    lib.fgo_debug_solve_fused.argtypes = [C.c_void_p, C.c_double, dp]
    lib.fgo_debug_launch_census.argtypes = [C.c_void_p, C.c_int, i64p, i64p, i64p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                            C.POINTER(C.c_int), C.c_char_p, C.c_int]
    lib.fgo_debug_isam_last.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 6 + [C.c_int,
                                        C.POINTER(C.c_int), C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_char_p, dp, C.c_int64]
    lib.fgo_debug_linearize_census.argtypes = [C.c_void_p, i64p]
    lib.fgo_imu_params_vn100.argtypes = [dp]
    lib.fgo_preint_reset.argtypes = [dp, dp]
    lib.fgo_preint_integrate.argtypes = [dp, dp, dp, dp, C.c_double]
    lib.fgo_preint_predict.argtypes = [dp] * 7
    lib.fgo_set_fixed.argtypes = [C.c_void_p, C.c_int64, C.c_int]
    lib.fgo_preint_information.argtypes = [dp, dp]
    lib.fgo_preint_batch.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_int64), dp, dp, C.c_double, dp, dp, dp]
    lib.fgo_two_view_params_default.restype = None
    lib.fgo_two_view_params_default.argtypes = [C.POINTER(TwoViewParams)]
    lib.fgo_two_view_ba_batch.argtypes = [C.c_int, C.c_int64, i64p, dp, dp, dp, dp, dp, dp, C.POINTER(TwoViewParams), dp, dp, dp, dp,
                                          C.POINTER(TwoViewResult)]
    lib.fgo_plane_check_params_default.restype = None
    lib.fgo_plane_check_params_default.argtypes = [C.POINTER(PlaneCheckParams)]
    lib.fgo_plane_check_vro_batch.argtypes = [C.c_int, C.c_int64, dp, dp, dp, i64p, dp, dp, i64p, dp, dp, C.POINTER(PlaneCheckParams),
                                              C.POINTER(PlaneCheckResult), i64p, dp, dp, dp, dp, dp]
    lib.fgo_chi2_quantile.restype = C.c_double
    lib.fgo_chi2_quantile.argtypes = [C.c_int, C.c_double]
    lib.fgo_imu_check_params_default.restype = None
    lib.fgo_imu_check_params_default.argtypes = [C.POINTER(ImuCheckParams)]
    lib.fgo_imu_check_vro_batch.argtypes = [C.c_int, C.c_int64, dp, dp, dp, C.c_int64, dp, i64p, dp, dp, C.POINTER(ImuCheckParams),
                                            C.POINTER(ImuCheckResult), dp, dp]
    lib.fgo_vro_params_default.restype = None
    lib.fgo_vro_params_default.argtypes = [C.POINTER(VroParams)]
    lib.fgo_vro_ransac_batch.argtypes = [C.c_int, C.c_int64, i64p, dp, dp, C.POINTER(VroParams), dp, dp, dp, C.POINTER(C.c_ubyte),
                                         C.POINTER(C.c_int32), C.POINTER(VroResult)]
    lib.fgo_debug_vro_waves.argtypes = [C.c_int]
    lib.fgo_debug_vro_kernel_ms.restype = C.c_double
    lib.fgo_debug_vro_kernel_ms.argtypes = []
    lib.fgo_plane_extract_params_default.restype = None
    lib.fgo_plane_extract_params_default.argtypes = [C.POINTER(PlaneExtractParams)]
    lib.fgo_plane_extract_batch.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_uint16), C.POINTER(PlaneExtractParams),
                                            C.POINTER(PlaneExtractResult), dp, dp, dp, C.POINTER(PlaneExtractPlane),
                                            C.POINTER(C.c_int8), C.POINTER(C.c_int32)]
    lib.fgo_debug_plane_extract_kernel_ms.restype = C.c_double
    lib.fgo_debug_plane_extract_kernel_ms.argtypes = []
    lib.fgo_plane_propagate_params_default.restype = None
    lib.fgo_plane_propagate_params_default.argtypes = [C.POINTER(PlanePropagateParams)]
    lib.fgo_plane_propagate_batch.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8),
                                              C.POINTER(C.c_int8), C.POINTER(C.c_int32), dp, dp, C.c_int64, i64p, i64p, dp, dp, dp,
                                              C.POINTER(PlanePropagateParams), C.POINTER(PlanePropagateResult), dp, dp, dp,
                                              C.POINTER(PlanePropagatePlane), C.POINTER(PlanePropagatePred), C.POINTER(C.c_int8)]
    lib.fgo_debug_plane_propagate_kernel_ms.restype = C.c_double
    lib.fgo_debug_plane_propagate_kernel_ms.argtypes = []
    lib.fgo_match_params_default.restype = None
    lib.fgo_match_params_default.argtypes = [C.POINTER(MatchParams)]
    i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    lib.fgo_match_features_batch.argtypes = [C.c_int, C.c_int64, i64p, u8p, dp, dp, C.c_int64, i64p, i64p, dp, u8p, C.POINTER(MatchParams),
                                             C.POINTER(MatchResult), i64p, i32p, i32p, i32p, u8p, i64p, i64p, i64p, dp, dp, dp, dp, i32p]
    lib.fgo_debug_match_kernel_ms.restype = C.c_double
    lib.fgo_debug_match_kernel_ms.argtypes = []
    lib.fgo_map_params_default.restype = None
    lib.fgo_map_params_default.argtypes = [C.POINTER(MapParams)]
    lib.fgo_map_fuse_batch.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_uint16), u8p, C.c_int, dp, dp, C.POINTER(MapParams),
                                       C.c_int64, C.POINTER(MapResult), dp, u8p, C.POINTER(C.c_int32), i64p, i64p, dp]
    lib.fgo_debug_map_fuse_kernel_ms.restype = C.c_double
    lib.fgo_debug_map_fuse_kernel_ms.argtypes = []
    lib.fgo_map_clean_params_default.restype = None
    lib.fgo_map_clean_params_default.argtypes = [C.POINTER(MapCleanParams)]
    lib.fgo_map_clean.argtypes = [C.c_int, C.c_int64, dp, C.POINTER(MapCleanParams), C.POINTER(MapCleanResult), C.POINTER(C.c_int32), u8p,
                                  C.POINTER(C.c_int32), i64p, dp]
    lib.fgo_debug_map_clean_kernel_ms.restype = C.c_double
    lib.fgo_debug_map_clean_kernel_ms.argtypes = []
    lib.fgo_map_normals_params_default.restype = None
    lib.fgo_map_normals_params_default.argtypes = [C.POINTER(MapNormalsParams)]
    lib.fgo_map_normals.argtypes = [C.c_int, C.c_int64, dp, C.POINTER(MapNormalsParams), C.POINTER(MapNormalsResult), dp, dp, dp, i32p, u8p,
                                    i32p, i64p, i64p]
    lib.fgo_debug_map_normals_kernel_ms.restype = C.c_double
    lib.fgo_debug_map_normals_kernel_ms.argtypes = []
    lib.fgo_map_render_params_default.restype = None
    lib.fgo_map_render_params_default.argtypes = [C.POINTER(MapRenderParams)]
    lib.fgo_map_render_batch.argtypes = [C.c_int, C.c_int64, dp, u8p, C.c_int, C.c_int64, dp, dp, dp, C.c_int, C.c_int,
                                         C.POINTER(MapRenderParams), C.POINTER(C.c_uint16), C.POINTER(MapRenderResult),
                                         C.POINTER(MapRenderView), i32p, i32p, u8p, dp]
    lib.fgo_debug_map_render_kernel_ms.restype = C.c_double
    lib.fgo_debug_map_render_kernel_ms.argtypes = []
    lib.fgo_add_vec3.argtypes = [C.c_void_p, C.c_int64, dp]
    lib.fgo_add_bias.argtypes = [C.c_void_p, C.c_int64, dp]
    lib.fgo_add_prior_vec3.argtypes = [C.c_void_p, C.c_int64, dp, C.c_double]
    lib.fgo_add_prior_bias.argtypes = [C.c_void_p, C.c_int64, dp, C.c_double]
    lib.fgo_set_gravity.argtypes = [C.c_void_p, dp]
    lib.fgo_add_imu_combined.argtypes = [C.c_void_p, i64p, dp]
    lib.fgo_add_plane.argtypes = [C.c_void_p, C.c_int64, dp]
    lib.fgo_add_plane_factor.argtypes = [C.c_void_p, C.c_int64, C.c_int64, dp, dp]
    lib.fgo_add_point3.argtypes = [C.c_void_p, C.c_int64, dp]
    lib.fgo_add_prior_point3.argtypes = [C.c_void_p, C.c_int64, dp, C.c_double]
    lib.fgo_set_calib_ds2.argtypes = [C.c_void_p] + [C.c_double] * 9 + [dp]
    lib.fgo_add_reproj.argtypes = [C.c_void_p, C.c_int64, C.c_int64, dp, C.c_double]
    lib.fgo_add_points3.argtypes = [C.c_void_p, C.c_int64, i64p, dp, C.c_double]
    lib.fgo_add_reprojs.argtypes = [C.c_void_p, C.c_int64, i64p, i64p, dp, C.c_double]
    return lib


lib = _load()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


class FgoError(RuntimeError):
    pass


def preint_information(buf):
    """fgo_preint_information: the 15x15 information matrix fgo_add_imu_combined derives from a preintegration payload"""
    b = np.ascontiguousarray(buf, np.float64)
    out = np.zeros((15, 15))
    rc = lib.fgo_preint_information(_dp(b), _dp(out))
    if rc < 0:
        raise FgoError("fgo_preint_information failed: %d" % rc)
    return out


def preint_batch(sample_ptr, acc, gyro, dt, bias_hat=None, params=None, device=0):
    """fgo_preint_batch: every factor's samples integrated by one wave on the GPU; returns [n, PREINT_DOUBLES]"""
    sp = np.ascontiguousarray(sample_ptr, np.int64)
    n = len(sp) - 1
    a = np.ascontiguousarray(acc, np.float64); w = np.ascontiguousarray(gyro, np.float64)
    if params is None:
        params = np.zeros(IMU_PARAM_DOUBLES); lib.fgo_imu_params_vn100(_dp(params))
    params = np.ascontiguousarray(params, np.float64)
    out = np.zeros((n, PREINT_DOUBLES))
    bh = None if bias_hat is None else np.ascontiguousarray(bias_hat, np.float64)
    rc = lib.fgo_preint_batch(device, n, _i64p(sp), _dp(a), _dp(w), dt, None if bh is None else _dp(bh), _dp(params), _dp(out))
    if rc < 0:
        raise FgoError("fgo_preint_batch failed: %d" % rc)
    return out


def two_view_params(**kw):
    """fgo_two_view_params_default, with the given fields replaced"""
    p = TwoViewParams()
    lib.fgo_two_view_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(TwoViewParams._fields_):
            raise TypeError("fgo_two_view_params has no field %r" % k)
        setattr(p, k, v)
    return p


def two_view_ba_batch(match_ptr, xyz, uv_i, uv_j, calib9, pose_j0=None, body_P_sensor=None, params=None, device=0):
    """fgo_two_view_ba_batch: CGraphGT::bundleAdjust for every pair in one launch, one wave per pair.  Pair p owns the matches
    [match_ptr[p], match_ptr[p + 1]) of xyz (M x 3, camera i), uv_i / uv_j (M x 2).  Returns a dict of arrays over the pairs:
    pose_j, pose_i (n x 7), cov (n x 6 x 6, tangent [omega; v]), info (n x 21, upper triangle), status (FGO_TV_*), iterations,
    trials, error_initial, error_final, lambda_final."""
    mp = np.ascontiguousarray(match_ptr, np.int64)
    n = len(mp) - 1
    if n < 0:
        raise FgoError("two_view_ba_batch: match_ptr needs n_pairs + 1 entries")
    x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    a = np.ascontiguousarray(uv_i, np.float64).reshape(-1, 2); b = np.ascontiguousarray(uv_j, np.float64).reshape(-1, 2)
    m = int(mp[-1])
    if min(len(x), len(a), len(b)) < m:
        raise FgoError("two_view_ba_batch: match_ptr names %d matches, the arrays hold fewer" % m)
    c9 = np.ascontiguousarray(calib9, np.float64)
    if c9.shape != (9,):
        raise FgoError("two_view_ba_batch: calib9 = fx fy s u0 v0 k1 k2 p1 p2")
    p0 = None if pose_j0 is None else np.ascontiguousarray(pose_j0, np.float64).reshape(-1, 7)
    if p0 is not None and len(p0) != n:
        raise FgoError("two_view_ba_batch: pose_j0 needs one pose per pair")
    bps = None if body_P_sensor is None else np.ascontiguousarray(body_P_sensor, np.float64)
    if bps is not None and bps.shape != (7,):
        raise FgoError("two_view_ba_batch: body_P_sensor = t(3) q_xyzw(4)")
    pose_j = np.zeros((n, 7)); pose_i = np.zeros((n, 7)); cov = np.zeros((n, 6, 6)); info = np.zeros((n, 21))
    res = (TwoViewResult * max(n, 1))()
    rc = lib.fgo_two_view_ba_batch(device, n, _i64p(mp), _dp(x), _dp(a), _dp(b), None if p0 is None else _dp(p0), _dp(c9),
                                   None if bps is None else _dp(bps), None if params is None else C.byref(params),
                                   _dp(pose_j), _dp(pose_i), _dp(cov), _dp(info), res)
    if rc < 0:
        raise FgoError("fgo_two_view_ba_batch failed: %d" % rc)
    r = np.frombuffer(res, dtype=np.dtype([("status", "i4"), ("iterations", "i4"), ("trials", "i4"), ("_pad", "i4"), ("error_initial", "f8"),
                                           ("error_final", "f8"), ("lambda_final", "f8")]), count=n)
    out = {"pose_j": pose_j, "pose_i": pose_i, "cov": cov, "info": info}
    for k in ("status", "iterations", "trials", "error_initial", "error_final", "lambda_final"):
        out[k] = r[k].copy()
    return out


def plane_check_params(**kw):
    """fgo_plane_check_params_default, with the given fields replaced"""
    p = PlaneCheckParams()
    lib.fgo_plane_check_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(PlaneCheckParams._fields_):
            raise TypeError("fgo_plane_check_params has no field %r" % k)
        setattr(p, k, v)
    return p


def plane_check_vro_batch(pose_ij, pi_ptr, pi_abcd, pi_cov, pj_ptr, pj_abcd, pj_cov, info=None, cov=None, params=None, device=0):
    """fgo_plane_check_vro_batch: the plane check of gtsam/test_plane_check_vo.cpp for every record in one launch, one wave per
    record.  Record r has the pose pose_ij[r] (n x 7) of frame j in frame i with either info[r] (n x 21, what two_view_ba_batch
    returns) or cov[r] (n x 6 x 6), and owns the planes [pi_ptr[r], pi_ptr[r + 1]) of pi_abcd (Mi x 4) / pi_cov (Mi x 4 x 4, CPlane::m_CP)
    seen in frame i and likewise [pj_ptr[r], pj_ptr[r + 1]) of pj_abcd / pj_cov seen in frame j.  Returns a dict of arrays: over the
    records status (FGO_PC_*), n_matched, n_bad, best_i, best_j, err, err_raw; over the planes i match (index within the record's
    j-list or -1), d2, raw, pred_abcd (Mi x 4), pred_cov (Mi x 3 x 3), sdj."""
    ps = np.ascontiguousarray(pose_ij, np.float64).reshape(-1, 7)
    n = len(ps)
    ip = np.ascontiguousarray(pi_ptr, np.int64); jp = np.ascontiguousarray(pj_ptr, np.int64)
    if len(ip) != n + 1 or len(jp) != n + 1:
        raise FgoError("plane_check_vro_batch: pi_ptr and pj_ptr need n_records + 1 entries")
    planes = []
    for name, ptr, abcd, c16 in (("pi", ip, pi_abcd, pi_cov), ("pj", jp, pj_abcd, pj_cov)):
        a = np.ascontiguousarray(abcd, np.float64).reshape(-1, 4); c = np.ascontiguousarray(c16, np.float64).reshape(-1, 16)
        if min(len(a), len(c)) < int(ptr[-1]):
            raise FgoError("plane_check_vro_batch: %s_ptr names %d planes, the arrays hold fewer" % (name, int(ptr[-1])))
        planes += [a, c]
    if (info is None) == (cov is None):
        raise FgoError("plane_check_vro_batch: exactly one of info (n x 21) and cov (n x 6 x 6)")
    s = np.ascontiguousarray(info if cov is None else cov, np.float64).reshape(-1, 21 if cov is None else 36)
    if len(s) != n:
        raise FgoError("plane_check_vro_batch: info / cov needs one entry per record")
    mi = max(int(ip[-1]), 0)
    match = np.zeros(mi, np.int64); d2 = np.zeros(mi); raw = np.zeros(mi); sdj = np.zeros(mi)
    pred = np.zeros((mi, 4)); pcov = np.zeros((mi, 3, 3))
    res = (PlaneCheckResult * max(n, 1))()
    rc = lib.fgo_plane_check_vro_batch(device, n, _dp(ps), _dp(s) if cov is None else None, None if cov is None else _dp(s),
                                       _i64p(ip), _dp(planes[0]), _dp(planes[1]), _i64p(jp), _dp(planes[2]), _dp(planes[3]),
                                       None if params is None else C.byref(params), res, _i64p(match), _dp(d2), _dp(raw), _dp(pred),
                                       _dp(pcov), _dp(sdj))
    if rc < 0:
        raise FgoError("fgo_plane_check_vro_batch failed: %d" % rc)
    r = np.frombuffer(res, dtype=np.dtype([("status", "i4"), ("n_matched", "i4"), ("n_bad", "i4"), ("best_i", "i4"), ("best_j", "i4"),
                                           ("reserved", "i4"), ("err", "f8"), ("err_raw", "f8")]), count=n)
    out = {"match": match, "d2": d2, "raw": raw, "pred_abcd": pred, "pred_cov": pcov, "sdj": sdj}
    for k in ("status", "n_matched", "n_bad", "best_i", "best_j", "err", "err_raw"):
        out[k] = r[k].copy()
    return out


def chi2_quantile(dof, p):
    """fgo_chi2_quantile: the reference's utils::chi2(dof, alpha), the quantile of chi-square(dof) at probability p"""
    return float(lib.fgo_chi2_quantile(int(dof), float(p)))


def imu_check_params(**kw):
    """fgo_imu_check_params_default, with the given fields replaced"""
    p = ImuCheckParams()
    lib.fgo_imu_check_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(ImuCheckParams._fields_):
            raise TypeError("fgo_imu_check_params has no field %r" % k)
        setattr(p, k, v)
    return p


def imu_check_vro_batch(pose_ij, preint, preint_index, info=None, cov=None, bias_i=None, imu_q_cam=None, params=None, device=0,
                        want_dw=False, want_cov=False):
    """fgo_imu_check_vro_batch: the chi-square test of gtsam/test_vro_imu_graph.cpp:679-778 for every record in one launch, one wave
    per record.  Record r has the pose pose_ij[r] (n x 7, camera frame) with either info[r] (n x 21, what two_view_ba_batch returns)
    or cov[r] (n x 6 x 6) and is tested against the preintegration preint[preint_index[r]]; preint is the [n_preint, PREINT_DOUBLES]
    array preint_batch returns (or rows of Preintegrator.buf), bias_i (n x 6: acc, gyro) the bias at frame i (None = each
    preintegration's own), imu_q_cam the rotation of the camera in the IMU frame (x y z w, None = identity).  Returns a dict of
    arrays over the records: status (FGO_IC_*), reject (bit 0: d2 > d2_gate, bit 1: d2_ref > d2_ref_gate), d2, d2_ref, angle, and
    dw (n x 3) / cov_dw (n x 3 x 3) when asked for."""
    ps = np.ascontiguousarray(pose_ij, np.float64).reshape(-1, 7)
    n = len(ps)
    pm = np.ascontiguousarray(preint, np.float64).reshape(-1, PREINT_DOUBLES)
    ix = np.ascontiguousarray(preint_index, np.int64).reshape(-1)
    if len(ix) != n:
        raise FgoError("imu_check_vro_batch: preint_index needs one entry per record")
    if (info is None) == (cov is None):
        raise FgoError("imu_check_vro_batch: exactly one of info (n x 21) and cov (n x 6 x 6)")
    s = np.ascontiguousarray(info if cov is None else cov, np.float64).reshape(-1, 21 if cov is None else 36)
    if len(s) != n:
        raise FgoError("imu_check_vro_batch: info / cov needs one entry per record")
    b = None if bias_i is None else np.ascontiguousarray(bias_i, np.float64).reshape(-1, 6)
    if b is not None and len(b) != n:
        raise FgoError("imu_check_vro_batch: bias_i needs one entry per record")
    q = None if imu_q_cam is None else np.ascontiguousarray(imu_q_cam, np.float64)
    if q is not None and q.shape != (4,):
        raise FgoError("imu_check_vro_batch: imu_q_cam = x y z w")
    dw = np.zeros((n, 3)) if want_dw else None
    cdw = np.zeros((n, 3, 3)) if want_cov else None
    res = (ImuCheckResult * max(n, 1))()
    opt = lambda a: None if a is None else _dp(a)
    rc = lib.fgo_imu_check_vro_batch(device, n, _dp(ps), _dp(s) if cov is None else None, None if cov is None else _dp(s), len(pm),
                                     _dp(pm), _i64p(ix), opt(b), opt(q), None if params is None else C.byref(params), res, opt(dw),
                                     opt(cdw))
    if rc < 0:
        raise FgoError("fgo_imu_check_vro_batch failed: %d" % rc)
    r = np.frombuffer(res, dtype=np.dtype([("status", "i4"), ("reject", "i4"), ("d2", "f8"), ("d2_ref", "f8"), ("angle", "f8")]), count=n)
    out = {k: r[k].copy() for k in ("status", "reject", "d2", "d2_ref", "angle")}
    if want_dw:
        out["dw"] = dw
    if want_cov:
        out["cov_dw"] = cdw
    return out


def vro_params(**kw):
    """fgo_vro_params_default, with the given fields replaced (sigma_z: three coefficients)"""
    p = VroParams()
    lib.fgo_vro_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(VroParams._fields_):
            raise TypeError("fgo_vro_params has no field %r" % k)
        setattr(p, k, (C.c_double * 3)(*v) if k == "sigma_z" else v)
    return p


def vro_ransac_batch(match_ptr, xyz_i, xyz_j, params=None, device=0, want_info=True, want_cov=True, want_inliers=True,
                     want_hyp_counts=False):
    """fgo_vro_ransac_batch: RANSAC registration of every pair in one launch, one workgroup per pair.  Pair p owns the matches
    [match_ptr[p], match_ptr[p + 1]) of xyz_i / xyz_j (M x 3: the same feature in camera i / camera j).  Returns a dict of arrays
    over the pairs: pose_ij (n x 7, p_i = R p_j + t: what two_view_ba_batch takes as pose_j0 and the two checks as pose_ij), status
    (FGO_VRO_*), n_inliers, best_hypothesis, best_count, n_valid, rounds, rmse, and when asked for info (n x 21), cov (n x 6 x 6),
    inliers (M, uint8), hyp_counts (n x hypotheses, int32).  A failed pair carries the void record (identity, information 10000)."""
    mp = np.ascontiguousarray(match_ptr, np.int64)
    n = len(mp) - 1
    if n < 0:
        raise FgoError("vro_ransac_batch: match_ptr needs n_pairs + 1 entries")
    a = np.ascontiguousarray(xyz_i, np.float64).reshape(-1, 3); b = np.ascontiguousarray(xyz_j, np.float64).reshape(-1, 3)
    m = int(mp[-1])
    if min(len(a), len(b)) < m:
        raise FgoError("vro_ransac_batch: match_ptr names %d matches, the arrays hold fewer" % m)
    if params is None:
        params = vro_params()
    pose = np.zeros((n, 7))
    info = np.zeros((n, 21)) if want_info else None
    cov = np.zeros((n, 6, 6)) if want_cov else None
    inl = np.zeros(max(m, 0), np.uint8) if want_inliers else None
    hyp = np.zeros((n, max(params.hypotheses, 0)), np.int32) if want_hyp_counts else None
    res = (VroResult * max(n, 1))()
    opt = lambda x: None if x is None else _dp(x)
    rc = lib.fgo_vro_ransac_batch(device, n, _i64p(mp), _dp(a), _dp(b), C.byref(params), _dp(pose), opt(info), opt(cov),
                                  None if inl is None else inl.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                  None if hyp is None else hyp.ctypes.data_as(C.POINTER(C.c_int32)), res)
    if rc < 0:
        raise FgoError("fgo_vro_ransac_batch failed: %d" % rc)
    fields = ("status", "n_inliers", "best_hypothesis", "best_count", "n_valid", "rounds")
    r = np.frombuffer(res, dtype=np.dtype([(f, "i4") for f in fields] + [("rmse", "f8")]), count=n)
    out = {"pose_ij": pose}
    for k in fields + ("rmse",):
        out[k] = r[k].copy()
    for k, v in (("info", info), ("cov", cov), ("inliers", inl), ("hyp_counts", hyp)):
        if v is not None:
            out[k] = v
    return out


def plane_extract_params(**kw):
    """fgo_plane_extract_params_default, with the given fields replaced (sigma_z: three coefficients)"""
    p = PlaneExtractParams()
    lib.fgo_plane_extract_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(PlaneExtractParams._fields_):
            raise TypeError("fgo_plane_extract_params has no field %r" % k)
        setattr(p, k, (C.c_double * 3)(*v) if k == "sigma_z" else v)
    return p


def plane_extract_batch(depth, params=None, want_labels=False, want_hyp_counts=False, device=0):
    """fgo_plane_extract_batch: the planes of every depth frame in one launch, one workgroup per frame.  depth is n x H x W (or
    H x W for one frame) of uint16 depth words.  Returns a dict of arrays.  Over the frames: status (FGO_PX_*), n_planes,
    n_valid_pixels, rounds_run; with the fixed stride max_planes per frame (the slots past n_planes are zero): abcd_all
    (n x max_planes x 4), cov16_all (n x max_planes x 4 x 4), cov_ut6_all (n x max_planes x 6), n_pixels, best_hypothesis, best_count,
    n_valid_hyp, fits, rmse (n x max_planes) and centroid (n x max_planes x 3); packed, as plane_check_vro_batch takes them for
    either frame of a record: ptr (n + 1; frame f owns the planes [ptr[f], ptr[f + 1])), abcd (P x 4), cov16 (P x 16) and cov_ut6
    (P x 6, what Graph.add_plane_factor / gate_plane_factors / associate_planes take); when asked for labels (n x H x W, int8: -2 no
    depth, -1 no plane, k) and hyp_counts (n x max_planes x hypotheses, int32)."""
    d = np.ascontiguousarray(depth, np.uint16)
    if d.ndim == 2:
        d = d[None]
    if d.ndim != 3:
        raise FgoError("plane_extract_batch: depth is n x H x W")
    n, h, w = d.shape
    if params is None:
        params = plane_extract_params()
    mp = min(max(params.max_planes, 1), FGO_PX_MAX_PLANES)
    abcd = np.zeros((n, mp, 4)); cov16 = np.zeros((n, mp, 4, 4)); ut6 = np.zeros((n, mp, 6))
    planes = (PlaneExtractPlane * max(n * mp, 1))()
    res = (PlaneExtractResult * max(n, 1))()
    lab = np.zeros((n, h, w), np.int8) if want_labels else None
    hyp = np.zeros((n, mp, min(max(params.hypotheses, 0), 1 << 16)), np.int32) if want_hyp_counts else None
    rc = lib.fgo_plane_extract_batch(device, n, w, h, d.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(params), res, _dp(abcd), _dp(cov16),
                                     _dp(ut6), planes, None if lab is None else lab.ctypes.data_as(C.POINTER(C.c_int8)),
                                     None if hyp is None else hyp.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc < 0:
        raise FgoError("fgo_plane_extract_batch failed: %d" % rc)
    fields = ("status", "n_planes", "n_valid_pixels", "rounds_run")
    r = np.frombuffer(res, dtype=np.dtype([(f, "i4") for f in fields]), count=n)
    out = {k: r[k].copy() for k in fields}
    pf = ("n_pixels", "best_hypothesis", "best_count", "n_valid_hyp", "fits")
    pl = np.frombuffer(planes, dtype=np.dtype([(f, "i4") for f in pf] + [("reserved", "i4"), ("rmse", "f8"), ("centroid", "f8", 3)]),
                       count=n * mp).reshape(n, mp)
    for k in pf + ("rmse", "centroid"):
        out[k] = pl[k].copy()
    out.update(abcd_all=abcd, cov16_all=cov16, cov_ut6_all=ut6)
    keep = np.arange(mp)[None, :] < out["n_planes"][:, None]
    out["ptr"] = np.concatenate([[0], np.cumsum(out["n_planes"])]).astype(np.int64)
    out["abcd"] = abcd[keep]; out["cov16"] = cov16[keep].reshape(-1, 16); out["cov_ut6"] = ut6[keep]
    if lab is not None:
        out["labels"] = lab
    if hyp is not None:
        out["hyp_counts"] = hyp
    return out


def plane_propagate_params(**kw):
    """fgo_plane_propagate_params_default, with the given fields replaced (sigma_z: three coefficients)"""
    p = PlanePropagateParams()
    lib.fgo_plane_propagate_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(PlanePropagateParams._fields_):
            raise TypeError("fgo_plane_propagate_params has no field %r" % k)
        setattr(p, k, (C.c_double * 3)(*v) if k == "sigma_z" else v)
    return p


def plane_propagate_batch(depth, intensity, labels, n_planes, abcd, cov16, frame_i, frame_j, pose_ij, info=None, cov=None, params=None,
                          want_labels=True, want_pred=True, want_planes=True, want_ut6=True, device=0):
    """fgo_plane_propagate_batch: the planes of frame frame_i[p] carried into frame frame_j[p] for every pair in one launch, one
    workgroup per pair.  The frames: depth (n x H x W uint16), intensity (n x H x W uint8), labels (n x H x W int8: plane_extract_batch's
    labels, or this call's), n_planes (n), abcd (n x m x 4) and cov16 (n x m x 4 x 4) with m <= FGO_PX_MAX_PLANES (plane_extract_batch's
    abcd_all / cov16_all).  The pairs: frame_i, frame_j (indices), pose_ij (n_pairs x 7, the pose of frame j in frame i) and either info
    (n_pairs x 21) or cov (n_pairs x 6 x 6).  Returns a dict of arrays.  Over the pairs: status (FGO_PP_*), n_planes, num_added,
    search_rest; with the stride FGO_PX_MAX_PLANES per pair (the slots past n_planes are zero): abcd_all, cov16_all, cov_ut6_all,
    n_pixels, n_seed, source, rmse, centroid (per kept plane) and pred_abcd, sdj, n_prev, pred_n_seed, kept (per PREVIOUS plane); packed,
    as plane_extract_batch packs them: ptr, abcd, cov16, cov_ut6; and labels (n_pairs x H x W int8: k, -1 free, -2 free without a depth
    in range, -3 rejected, -4 claimed by a dropped prediction)."""
    d = np.ascontiguousarray(depth, np.uint16)
    if d.ndim != 3:
        raise FgoError("plane_propagate_batch: depth is n x H x W")
    nf, h, w = d.shape
    it = np.ascontiguousarray(intensity, np.uint8); lb = np.ascontiguousarray(labels, np.int8)
    if it.shape != d.shape or lb.shape != d.shape:
        raise FgoError("plane_propagate_batch: intensity and labels have the shape of depth")
    npl = np.ascontiguousarray(n_planes, np.int32).reshape(-1)
    MP = FGO_PX_MAX_PLANES
    a = np.asarray(abcd, np.float64).reshape(nf, -1, 4); c = np.asarray(cov16, np.float64).reshape(nf, -1, 16)
    if len(npl) != nf or a.shape[1] != c.shape[1] or a.shape[1] > MP:
        raise FgoError("plane_propagate_batch: n_planes (n), abcd (n x m x 4) and cov16 (n x m x 16), m <= %d" % MP)
    a8 = np.zeros((nf, MP, 4)); a8[:, :a.shape[1]] = a
    c8 = np.zeros((nf, MP, 16)); c8[:, :c.shape[1]] = c
    fi = np.ascontiguousarray(frame_i, np.int64).reshape(-1); fj = np.ascontiguousarray(frame_j, np.int64).reshape(-1)
    n = len(fi)
    ps = np.ascontiguousarray(pose_ij, np.float64).reshape(-1, 7)
    if (info is None) == (cov is None):
        raise FgoError("plane_propagate_batch: exactly one of info (n x 21) and cov (n x 6 x 6)")
    s = np.ascontiguousarray(info if cov is None else cov, np.float64).reshape(-1, 21 if cov is None else 36)
    if len(fj) != n or len(ps) != n or len(s) != n:
        raise FgoError("plane_propagate_batch: frame_i, frame_j, pose_ij and info / cov need one entry per pair")
    if params is None:
        params = plane_propagate_params()
    abcd_o = np.zeros((n, MP, 4)); cov16_o = np.zeros((n, MP, 4, 4))
    ut6 = np.zeros((n, MP, 6)) if want_ut6 else None
    planes = (PlanePropagatePlane * max(n * MP, 1))() if want_planes else None
    pred = (PlanePropagatePred * max(n * MP, 1))() if want_pred else None
    lab = np.zeros((n, h, w), np.int8) if want_labels else None
    res = (PlanePropagateResult * max(n, 1))()
    rc = lib.fgo_plane_propagate_batch(device, nf, w, h, d.ctypes.data_as(C.POINTER(C.c_uint16)), it.ctypes.data_as(C.POINTER(C.c_uint8)),
                                       lb.ctypes.data_as(C.POINTER(C.c_int8)), npl.ctypes.data_as(C.POINTER(C.c_int32)), _dp(a8), _dp(c8),
                                       n, _i64p(fi), _i64p(fj), _dp(ps), _dp(s) if cov is None else None, None if cov is None else _dp(s),
                                       C.byref(params), res, _dp(abcd_o), _dp(cov16_o), None if ut6 is None else _dp(ut6), planes, pred,
                                       None if lab is None else lab.ctypes.data_as(C.POINTER(C.c_int8)))
    if rc < 0:
        raise FgoError("fgo_plane_propagate_batch failed: %d" % rc)
    fields = ("status", "n_planes", "num_added", "search_rest")
    r = np.frombuffer(res, dtype=np.dtype([(f, "i4") for f in fields]), count=n)
    out = {k: r[k].copy() for k in fields}
    out.update(abcd_all=abcd_o, cov16_all=cov16_o)
    if planes is not None:
        pl = np.frombuffer(planes, dtype=np.dtype([("n_pixels", "i4"), ("n_seed", "i4"), ("source", "i4"), ("reserved", "i4"), ("rmse", "f8"),
                                                    ("centroid", "f8", 3)]), count=n * MP).reshape(n, MP)
        for k in ("n_pixels", "n_seed", "source", "rmse", "centroid"):
            out[k] = pl[k].copy()
    if pred is not None:
        pd = np.frombuffer(pred, dtype=np.dtype([("abcd", "f8", 4), ("sdj", "f8"), ("n_prev", "i4"), ("n_seed", "i4"), ("kept", "i4"),
                                                  ("reserved", "i4")]), count=n * MP).reshape(n, MP)
        out.update(pred_abcd=pd["abcd"].copy(), sdj=pd["sdj"].copy(), n_prev=pd["n_prev"].copy(), pred_n_seed=pd["n_seed"].copy(),
                   kept=pd["kept"].copy())
    keep = np.arange(MP)[None, :] < out["n_planes"][:, None]
    out["ptr"] = np.concatenate([[0], np.cumsum(out["n_planes"])]).astype(np.int64)
    out["abcd"] = abcd_o[keep]; out["cov16"] = cov16_o[keep].reshape(-1, 16)
    if ut6 is not None:
        out["cov_ut6_all"] = ut6; out["cov_ut6"] = ut6[keep]
    if lab is not None:
        out["labels"] = lab
    return out


def plane_node_batch(depth, intensity, labels, n_planes, abcd, cov16, frame_i, frame_j, pose_ij, info=None, cov=None, params=None,
                     extract_params=None, device=0):
    """CGraphGT::predictPlaneNode for every pair, by composition: plane_propagate_batch (part 1), then part 2
    (gtsam/gtsam_graph.cpp:1043-1077): for the pairs with search_rest != 0 the depth of every pixel of frame j whose label is not -1 is
    zeroed and plane_extract_batch (extract_params) runs on the result; the new planes are
    appended after the propagated ones with source = -1, as far as FGO_PX_MAX_PLANES allows.  The reference then merges overlapping
    planes (CPlaneNode::mergeOverlappedPlanes), which is not in the reference tree and stays out of scope: nothing is merged here.
    Returns the dict of plane_propagate_batch with n_planes, abcd_all, cov16_all, cov_ut6_all, n_pixels, rmse, centroid, source, ptr,
    abcd, cov16, cov_ut6 and labels extended (a new plane's pixels carry its slot), n_new (per pair) and `extracted`, the dict of the
    plane_extract_batch call over the pairs in `rest` (indices), or None when there was none."""
    out = plane_propagate_batch(depth, intensity, labels, n_planes, abcd, cov16, frame_i, frame_j, pose_ij, info=info, cov=cov, params=params,
                                device=device)
    MP = FGO_PX_MAX_PLANES
    n = len(out["status"])
    out["n_new"] = np.zeros(n, np.int32); out["rest"] = np.nonzero(out["search_rest"] != 0)[0]; out["extracted"] = None
    if len(out["rest"]):
        d = np.ascontiguousarray(depth, np.uint16)[np.asarray(frame_j, np.int64).reshape(-1)[out["rest"]]].copy()
        d[out["labels"][out["rest"]] != -1] = 0
        ex = plane_extract_batch(d, params=extract_params, want_labels=True, device=device)
        out["extracted"] = ex
        for r, p in enumerate(out["rest"]):
            k0 = int(out["n_planes"][p]); m = min(int(ex["n_planes"][r]), MP - k0)
            for f in ("abcd_all", "cov16_all", "cov_ut6_all", "n_pixels", "rmse", "centroid"):
                out[f][p, k0:k0 + m] = ex[f][r, :m]
            out["source"][p, k0:k0 + m] = -1
            for k in range(m):
                out["labels"][p][ex["labels"][r] == k] = k0 + k
            out["n_new"][p] = m
            out["n_planes"][p] = k0 + m
        keep = np.arange(MP)[None, :] < out["n_planes"][:, None]
        out["ptr"] = np.concatenate([[0], np.cumsum(out["n_planes"])]).astype(np.int64)
        out["abcd"] = out["abcd_all"][keep]; out["cov16"] = out["cov16_all"][keep].reshape(-1, 16); out["cov_ut6"] = out["cov_ut6_all"][keep]
    return out


def match_params(**kw):
    """fgo_match_params_default, with the given fields replaced"""
    p = MatchParams()
    lib.fgo_match_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(MatchParams._fields_):
            raise TypeError("fgo_match_params has no field %r" % k)
        setattr(p, k, v)
    return p


def match_features_batch(feat_ptr, desc, xyz, uv, frame_i, frame_j, pose_ij=None, guided=None, params=None, want_dist=False, device=0):
    """fgo_match_features_batch: the descriptor matches of every pair of frames in one launch, one workgroup per pair.  Frame f owns
    the features [feat_ptr[f], feat_ptr[f + 1]) of desc (F x 128 uint8), xyz (F x 3, camera frame) and uv (F x 2); pair p matches the
    features of frame_j[p] (queries) against those of frame_i[p] (trains).  pose_ij (n_pairs x 7, p_i = R p_j + t: vro_ransac_batch's
    pose_ij) guides every pair, or the pairs `guided` (n_pairs, bool) names.  Returns a dict of arrays.  Packed, as vro_ransac_batch and
    two_view_ba_batch take them: ptr (n_pairs + 1), idx_i, idx_j (global feature indices), xyz_i, xyz_j (M x 3), uv_i, uv_j (M x 2).
    Per query, indexed q_ptr[p] + a: best (the train's local index, -1 without a candidate), d1, d2 (-1: none), reason (0 kept, 1 not
    usable, 2 no candidate, 3 ratio test, 4 absolute cap, 5 cross-check).  Over the pairs: status (FGO_FM_*), n_query, n_train,
    n_matches, n_ratio, n_cross.  With want_dist, dist: the N_j x N_i matrix of every pair (int32, -1 where (a, b) is no candidate),
    one after the other."""
    fp = np.ascontiguousarray(feat_ptr, np.int64).reshape(-1)
    nf = len(fp) - 1
    if nf < 0:
        raise FgoError("match_features_batch: feat_ptr needs n_frames + 1 entries")
    F = max(int(fp[-1]), 0)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, FGO_FM_DIM)
    x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3); u = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
    if min(len(d), len(x), len(u)) < F:
        raise FgoError("match_features_batch: feat_ptr names %d features, the arrays hold fewer" % F)
    fi = np.ascontiguousarray(frame_i, np.int64).reshape(-1); fj = np.ascontiguousarray(frame_j, np.int64).reshape(-1)
    n = len(fi)
    if len(fj) != n:
        raise FgoError("match_features_batch: frame_i and frame_j need one entry per pair")
    ps = None if pose_ij is None else np.ascontiguousarray(pose_ij, np.float64).reshape(-1, 7)
    gd = None if guided is None else np.ascontiguousarray(np.asarray(guided) != 0, np.uint8).reshape(-1)
    if (ps is not None and len(ps) != n) or (gd is not None and len(gd) != n):
        raise FgoError("match_features_batch: pose_ij and guided need one entry per pair")
    if params is None:
        params = match_params()
    ok = (np.diff(fp) >= 0).all() and fp[0] >= 0 and ((fi >= 0) & (fi < nf) & (fj >= 0) & (fj < nf)).all()
    cnt = np.diff(fp)
    nq = cnt[fj] if ok else np.zeros(n, np.int64)               # a bad argument is the library's to refuse
    Q = int(nq.sum()); T = int((nq * cnt[fi]).sum()) if ok else 0
    q_ptr = np.zeros(n + 1, np.int64); ptr = np.zeros(n + 1, np.int64)
    best = np.zeros(Q, np.int32); d1 = np.zeros(Q, np.int32); d2 = np.zeros(Q, np.int32); why = np.zeros(Q, np.uint8)
    idx_i = np.zeros(Q, np.int64); idx_j = np.zeros(Q, np.int64)
    xi = np.zeros((Q, 3)); xj = np.zeros((Q, 3)); ui = np.zeros((Q, 2)); uj = np.zeros((Q, 2))
    dist = np.zeros(T, np.int32) if want_dist else None
    res = (MatchResult * max(n, 1))()
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    rc = lib.fgo_match_features_batch(device, nf, _i64p(fp), u8(d), _dp(x), _dp(u), n, _i64p(fi), _i64p(fj),
                                      None if ps is None else _dp(ps), None if gd is None else u8(gd), C.byref(params), res, _i64p(q_ptr),
                                      i32(best), i32(d1), i32(d2), u8(why), _i64p(ptr), _i64p(idx_i), _i64p(idx_j), _dp(xi), _dp(xj),
                                      _dp(ui), _dp(uj), None if dist is None else i32(dist))
    if rc < 0:
        raise FgoError("fgo_match_features_batch failed: %d" % rc)
    fields = ("status", "n_query", "n_train", "n_matches", "n_ratio", "n_cross")
    r = np.frombuffer(res, dtype=np.dtype([(f, "i4") for f in fields]), count=n)
    out = {k: r[k].copy() for k in fields}
    m = int(ptr[-1])
    out.update(ptr=ptr, idx_i=idx_i[:m], idx_j=idx_j[:m], xyz_i=xi[:m], xyz_j=xj[:m], uv_i=ui[:m], uv_j=uj[:m], q_ptr=q_ptr, best=best,
               d1=d1, d2=d2, reason=why)
    if dist is not None:
        out["dist"] = dist
    return out


def vro_adjust_batch(feat_ptr, desc, xyz, uv, frame_i, frame_j, pose_ij, info=None, params=None, ransac_params=None, min_matches=5,
                     device=0):
    """CGraphGT::vroAdjust (gtsam/gtsam_graph.cpp:450-498) for every record, by composition: the guided match of the pair under the
    record's pose (matchNodePairBA(ni, Tji, pcam): match_features_batch with pose_ij), then vro_ransac_batch on those matches (the
    reference's getTransformFromMatches on them).  A record with fewer than min_matches matches (5: matches.size() <= 4, :463), or
    whose registration fails, is left as it is.  Returns a dict: adjusted (n_pairs, bool), pose_ij (n_pairs x 7) and info
    (n_pairs x 21; the rows of the records left alone are the caller's, zeros where info was not given), n_matches, and the two
    calls' own dicts `match` and `vro` (vro covers the pairs in `tried`, None when there was none)."""
    ps = np.ascontiguousarray(pose_ij, np.float64).reshape(-1, 7)
    n = len(ps)
    m = match_features_batch(feat_ptr, desc, xyz, uv, frame_i, frame_j, pose_ij=ps, params=params, device=device)
    pose = ps.copy()
    nf = np.zeros((n, 21)) if info is None else np.array(info, np.float64).reshape(n, 21)
    adjusted = np.zeros(n, bool)
    tried = np.nonzero(m["n_matches"] >= min_matches)[0]
    out = dict(match=m, vro=None, tried=tried, n_matches=m["n_matches"].copy())
    if len(tried):
        sel = np.concatenate([np.arange(m["ptr"][p], m["ptr"][p + 1]) for p in tried]).astype(np.int64)
        sp = np.concatenate([[0], np.cumsum(m["n_matches"][tried])]).astype(np.int64)
        v = vro_ransac_batch(sp, m["xyz_i"][sel], m["xyz_j"][sel], params=ransac_params, device=device, want_cov=False, want_inliers=False)
        good = v["status"] == FGO_VRO_OK
        pose[tried[good]] = v["pose_ij"][good]; nf[tried[good]] = v["info"][good]
        adjusted[tried[good]] = True
        out["vro"] = v
    out.update(adjusted=adjusted, pose_ij=pose, info=nf)
    return out


def map_params(**kw):
    """fgo_map_params_default, with the given fields replaced (rect: su, sv, eu, ev)"""
    p = MapParams()
    lib.fgo_map_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(MapParams._fields_):
            raise TypeError("fgo_map_params has no field %r" % k)
        setattr(p, k, (C.c_int * 4)(*v) if k == "rect" else v)
    return p


def map_fuse_batch(depth, pose_w, color=None, extrinsic=None, params=None, max_voxels=None, want_keys=False, want_rt=False, device=0):
    """fgo_map_fuse_batch: the voxel-grid map of all depth frames in one call.  depth is n x H x W (or H x W for one frame) of uint16
    depth words, pose_w n x 7 (t, q_xyzw: Graph.get_poses), color None, n x H x W (grey) or n x H x W x 3 (uint8), extrinsic the 7
    numbers of Pu2c or None.  max_voxels defaults to the bound n_sampled.  Returns a dict: xyz (m x 3), color (m x channels, None
    without colour), count (m, int32), frame_points (n, int64), with want_keys key (m, int64) and with want_rt rt (n x 12), each
    trimmed to m = min(n_voxels, max_voxels), in ascending key; and the result fields status (FGO_MAP_*), table_log2, n_sampled,
    n_valid, n_out_of_range, n_voxels, n_dropped."""
    d = np.ascontiguousarray(depth, np.uint16)
    if d.ndim == 2:
        d = d[None]
    if d.ndim != 3:
        raise FgoError("map_fuse_batch: depth is n x H x W")
    n, h, w = d.shape
    ps = np.ascontiguousarray(pose_w, np.float64).reshape(-1, 7)
    if len(ps) != n:
        raise FgoError("map_fuse_batch: pose_w needs one row of 7 per frame")
    col, ch = None, 0
    if color is not None:
        col = np.ascontiguousarray(color, np.uint8)
        if col.shape == (h, w) or col.shape == (h, w, 3):
            col = col[None]
        if col.shape not in ((n, h, w), (n, h, w, 1), (n, h, w, 3)):
            raise FgoError("map_fuse_batch: color is n x H x W or n x H x W x 3")
        ch = 3 if col.shape[-1] == 3 and col.ndim == 4 else 1
    ext = None if extrinsic is None else np.ascontiguousarray(extrinsic, np.float64).reshape(7)
    if params is None:
        params = map_params()
    if max_voxels is None:                                        # the bound n_sampled; a bad argument is the library's to refuse
        su, sv, eu, ev = params.rect
        if (su, sv, eu, ev) == (0, 0, 0, 0):
            eu, ev = w, h
        k = max(params.skip, 1)
        max_voxels = n * max(-(-(eu - su) // k), 0) * max(-(-(ev - sv) // k), 0)
    cap = max(int(max_voxels), 0)
    xyz = np.zeros((cap, 3)); cout = np.zeros((cap, ch), np.uint8) if ch else None
    cnt = np.zeros(cap, np.int32); key = np.zeros(cap, np.int64) if want_keys else None
    fpts = np.zeros(n, np.int64); rt = np.zeros((n, 12)) if want_rt else None
    res = MapResult()
    u8 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))
    rc = lib.fgo_map_fuse_batch(device, n, w, h, d.ctypes.data_as(C.POINTER(C.c_uint16)), u8(col), ch, _dp(ps), None if ext is None else _dp(ext),
                                C.byref(params), int(max_voxels), C.byref(res), _dp(xyz), u8(cout), cnt.ctypes.data_as(C.POINTER(C.c_int32)),
                                None if key is None else _i64p(key), _i64p(fpts), None if rt is None else _dp(rt))
    if rc < 0:
        raise FgoError("fgo_map_fuse_batch failed: %d" % rc)
    out = {f: int(getattr(res, f)) for f, _ in MapResult._fields_}
    m = 0 if res.status == FGO_MAP_FULL else min(res.n_voxels, cap)
    out.update(xyz=xyz[:m], color=None if cout is None else cout[:m], count=cnt[:m], frame_points=fpts)
    if key is not None:
        out["key"] = key[:m]
    if rt is not None:
        out["rt"] = rt
    return out


def map_clean_params(**kw):
    """fgo_map_clean_params_default, with the given fields replaced"""
    p = MapCleanParams()
    lib.fgo_map_clean_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(MapCleanParams._fields_):
            raise TypeError("fgo_map_clean_params has no field %r" % k)
        setattr(p, k, v)
    return p


def map_clean(xyz, color=None, count=None, params=None, device=0):
    """fgo_map_clean: cluster filtering and floor removal of a cloud in one call.  xyz is n x 3 (map_fuse_batch's "xyz", or any
    cloud), color (n or n x channels) and count (n) ride along when given.  Returns a dict: label (n, int32; -1 out of range), reason
    (n, uint8: 0 kept, 1 out of range, 2 cluster size, 3 floor), cluster_size (n_clusters, int32), index (n_kept, int64, ascending),
    xyz (n_kept x 3, the floor at zero of the up axis), color and count gathered through index (None when not given); and the
    result fields n_points, n_out_of_range, n_cells, n_clusters, n_clusters_kept, n_after_clusters, n_floor_removed, n_kept,
    floor_bin, floor_bin_points, floor_height."""
    x = np.ascontiguousarray(xyz, np.float64)
    if x.ndim != 2 or x.shape[1] != 3:
        raise FgoError("map_clean: xyz is n x 3")
    n = len(x)
    col = None if color is None else np.asarray(color)
    if col is not None and (col.ndim not in (1, 2) or len(col) != n):
        raise FgoError("map_clean: color needs one row per point")
    cnt = None if count is None else np.asarray(count)
    if cnt is not None and cnt.shape != (n,):
        raise FgoError("map_clean: count needs one entry per point")
    if params is None:
        params = map_clean_params()
    label = np.zeros(n, np.int32); reason = np.zeros(n, np.uint8); csize = np.zeros(n, np.int32)
    index = np.zeros(n, np.int64); out_xyz = np.zeros((n, 3))
    res = MapCleanResult()
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rc = lib.fgo_map_clean(device, n, _dp(x), C.byref(params), C.byref(res), i32(label), reason.ctypes.data_as(C.POINTER(C.c_uint8)),
                           i32(csize), _i64p(index), _dp(out_xyz))
    if rc < 0:
        raise FgoError("fgo_map_clean failed: %d" % rc)
    out = {f: getattr(res, f) for f, _ in MapCleanResult._fields_}
    index = index[:res.n_kept]
    out.update(label=label, reason=reason, cluster_size=csize[:res.n_clusters], index=index, xyz=out_xyz[:res.n_kept],
               color=None if col is None else col[index], count=None if cnt is None else cnt[index])
    return out


def map_normals_params(**kw):
    """fgo_map_normals_params_default, with the given fields replaced (viewpoint: 3 numbers)"""
    p = MapNormalsParams()
    lib.fgo_map_normals_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(MapNormalsParams._fields_):
            raise TypeError("fgo_map_normals_params has no field %r" % k)
        setattr(p, k, (C.c_double * 3)(*v) if k == "viewpoint" else v)
    return p


def map_normals(xyz, params=None, want_neighbours=False, want_scatter=False, device=0):
    """fgo_map_normals: the k nearest neighbours of every point of a cloud and the surface normal and curvature fitted to them, in
    one call.  xyz is n x 3 (map_clean's "xyz", or any cloud).  Returns a dict: normal (n x 3, unit, turned towards the viewpoint),
    curvature (n), eigenvalues (n x 3, ascending), n_neighbours (n, int32), status (n, uint8: 0 valid, 1 out of range, 2 fewer than 3
    neighbours, 3 all neighbours coincide; NaN in the floating outputs unless 0); with want_neighbours neighbour (n x k, int32, the
    point itself included, padded with -1) and dist2 (n x k, int64, squared distances in quanta of 2^-20 m), with want_scatter
    scatter (n x 6, int64); and the result fields n_points, n_out_of_range, n_cells, n_valid, n_few, n_degenerate."""
    x = np.ascontiguousarray(xyz, np.float64)
    if x.ndim != 2 or x.shape[1] != 3:
        raise FgoError("map_normals: xyz is n x 3")
    n = len(x)
    if params is None:
        params = map_normals_params()
    k = max(int(params.k), 0)
    normal = np.zeros((n, 3)); curv = np.zeros(n); eig = np.zeros((n, 3))
    nn = np.zeros(n, np.int32); status = np.zeros(n, np.uint8)
    nb = np.zeros((n, k), np.int32) if want_neighbours else None
    d2 = np.zeros((n, k), np.int64) if want_neighbours else None
    sc = np.zeros((n, 6), np.int64) if want_scatter else None
    res = MapNormalsResult()
    rc = lib.fgo_map_normals(device, n, _dp(x), C.byref(params), C.byref(res), _dp(normal), _dp(curv), _dp(eig),
                             nn.ctypes.data_as(C.POINTER(C.c_int32)), status.ctypes.data_as(C.POINTER(C.c_uint8)),
                             None if nb is None else nb.ctypes.data_as(C.POINTER(C.c_int32)), None if d2 is None else _i64p(d2),
                             None if sc is None else _i64p(sc))
    if rc < 0:
        raise FgoError("fgo_map_normals failed: %d" % rc)
    out = {f: getattr(res, f) for f, _ in MapNormalsResult._fields_}
    out.update(normal=normal, curvature=curv, eigenvalues=eig, n_neighbours=nn, status=status)
    if want_neighbours:
        out.update(neighbour=nb, dist2=d2)
    if want_scatter:
        out["scatter"] = sc
    return out


def map_render_params(**kw):
    """fgo_map_render_params_default, with the given fields replaced (background: 3 numbers)"""
    p = MapRenderParams()
    lib.fgo_map_render_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(MapRenderParams._fields_):
            raise TypeError("fgo_map_render_params has no field %r" % k)
        setattr(p, k, (C.c_uint8 * 3)(*v) if k == "background" else v)
    return p


def map_render_batch(xyz, pose_w, color=None, extrinsic=None, view_offset=None, width=176, height=144, params=None, depth=None,
                     want_zq=True, want_index=False, want_color=None, want_rt=False, device=0):
    """fgo_map_render_batch: the cloud drawn from every pose in one call, by a z-buffer.  xyz is n x 3 (map_fuse_batch's "xyz", or any
    cloud), color None, n (grey) or n x 3 (uint8), pose_w V x 7 (t, q_xyzw: Graph.get_poses, or a list of look_at poses), extrinsic
    the 7 numbers of Pu2c or None, view_offset a further pose composed on the right or None (look_at((0, -2, -5), (0, 0, 5),
    (0, -0.98, 0.199)) is the reference's chase camera), depth None or V x H x W uint16 measured depth words to check the map
    against.  want_color defaults to whether color is given.  Returns a dict: with want_zq zq (V x H x W, int32: the depth in quanta
    of 2^-20 m, -1 where nothing was drawn), with want_index index (V x H x W, int32, the drawn point or -1), with want_color color
    (V x H x W x channels, uint8; V x H x W for grey), with want_rt rt (V x 12); the per-view counts n_valid, n_drawn, n_pixels,
    n_meas, n_both, n_agree, n_closer, n_through (V, int64); and the result fields n_points, n_nonfinite, form, tile_rows."""
    x = np.ascontiguousarray(xyz, np.float64)
    if x.ndim != 2 or x.shape[1] != 3:
        raise FgoError("map_render_batch: xyz is n x 3")
    n = len(x)
    ps = np.ascontiguousarray(pose_w, np.float64)
    if ps.ndim == 1 and ps.size == 7:
        ps = ps[None]
    if ps.ndim != 2 or ps.shape[1] != 7:
        raise FgoError("map_render_batch: pose_w is V x 7")
    nv, w, h = len(ps), int(width), int(height)
    col, ch, grey = None, 0, False
    if color is not None:
        col = np.ascontiguousarray(color, np.uint8)
        grey = col.ndim == 1
        if col.shape not in ((n,), (n, 1), (n, 3)):
            raise FgoError("map_render_batch: color is n or n x 3")
        ch = 3 if col.ndim == 2 and col.shape[1] == 3 else 1
    if want_color is None:
        want_color = ch > 0
    if want_color and ch == 0:
        raise FgoError("map_render_batch: want_color needs color")
    ext = None if extrinsic is None else np.ascontiguousarray(extrinsic, np.float64).reshape(7)
    off = None if view_offset is None else np.ascontiguousarray(view_offset, np.float64).reshape(7)
    dm = None
    if depth is not None:
        dm = np.ascontiguousarray(depth, np.uint16)
        if dm.shape == (h, w):
            dm = dm[None]
        if dm.shape != (nv, h, w):
            raise FgoError("map_render_batch: depth is V x H x W")
    if params is None:
        params = map_render_params()
    hh, ww = max(h, 0), max(w, 0)                                  # a bad size is the library's to refuse
    zq = np.zeros((nv, hh, ww), np.int32) if want_zq else None
    index = np.zeros((nv, hh, ww), np.int32) if want_index else None
    cout = np.zeros((nv, hh, ww, ch), np.uint8) if want_color else None
    rt = np.zeros((nv, 12)) if want_rt else None
    views = (MapRenderView * max(nv, 1))()
    res = MapRenderResult()
    u8 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))
    i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    opt = lambda a: None if a is None else _dp(a)
    rc = lib.fgo_map_render_batch(device, n, _dp(x), u8(col), ch, nv, _dp(ps), opt(ext), opt(off), w, h, C.byref(params),
                                  None if dm is None else dm.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(res), views, i32(zq),
                                  i32(index), u8(cout), opt(rt))
    if rc < 0:
        raise FgoError("fgo_map_render_batch failed: %d" % rc)
    out = {f: int(getattr(res, f)) for f, _ in MapRenderResult._fields_}
    counts = np.frombuffer(views, np.int64).reshape(-1, 8)[:nv]
    out.update({f: counts[:, k].copy() for k, (f, _) in enumerate(MapRenderView._fields_)})
    if zq is not None:
        out["zq"] = zq
    if index is not None:
        out["index"] = index
    if cout is not None:
        out["color"] = cout[..., 0] if grey else cout
    if rt is not None:
        out["rt"] = rt
    return out


def look_at_matrix(eye, target, up):
    """R = [x y z] (columns) of look_at: z = normalise(target - eye), x = normalise((-up) x z), y = z x x.  x is made orthogonal to
    z once more after the cross product, so that R stays orthonormal to rounding when up is close to the line of sight."""
    eye, target, up = (np.asarray(v, np.float64).reshape(3) for v in (eye, target, up))
    z = target - eye
    nz = np.linalg.norm(z)
    x = np.cross(-up, z)
    nx = np.linalg.norm(x)
    if not (nz > 0 and nx > 0 and np.isfinite(nz) and np.isfinite(nx)):
        raise FgoError("look_at: target equals eye, or up is parallel to the line of sight")
    z = z / nz; x = x / nx
    x = x - (x @ z) * z
    x = x / np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1)


def look_at(eye, target, up):
    """the pose7 (t, q_xyzw) of a camera at eye that looks at target, in the camera convention of the map calls (x right, y down,
    z forward): R = look_at_matrix(eye, target, up), t = eye.  As pose_w of map_render_batch it is a camera in the world (a list of
    them: an arc flown round the map); as view_offset it is a camera placed relative to every pose:
    look_at((0, -2, -5), (0, 0, 5), (0, -0.98, 0.199)) is the chase camera of the reference's mapping/map_video.cpp:119-127."""
    R = look_at_matrix(eye, target, up)
    # the quaternion of R by the branch with the largest denominator
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * np.sqrt(1.0 + tr)
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(R))); j = (i + 1) % 3; k = (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / s]
        q[i] = 0.25 * s; q[j] = (R[j, i] + R[i, j]) / s; q[k] = (R[k, i] + R[i, k]) / s
    q = np.asarray(q)
    return np.concatenate([np.asarray(eye, np.float64).reshape(3), q / np.linalg.norm(q)])


def write_ppm(path, image):
    """a binary PPM (P6) for an H x W x 3 uint8 image, a binary PGM (P5) for H x W: one frame of map_render_batch's "color", to be
    looked at without an image library"""
    im = np.asarray(image)
    if im.dtype != np.uint8 or not (im.ndim == 2 or (im.ndim == 3 and im.shape[2] == 3)):
        raise FgoError("write_ppm: image is H x W x 3 or H x W, uint8")
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P6" if im.ndim == 3 else b"P5", im.shape[1], im.shape[0]))
        f.write(np.ascontiguousarray(im).tobytes())


def write_ply(path, xyz, color=None, normals=None):
    """an ASCII PLY in the layout of the reference's headerPLY (mapping/mapping_PCD.cpp:169-181): float x y z, uchar red green blue.
    color is m x 3, m or m x 1 (grey, repeated three times) or None (255).  With normals (m x 3: map_normals' "normal") the vertex
    also has float nx ny nz after z, the XYZ+RGB+normal cloud of pcd2mesh.cpp:65-67; without, the file is what it always was."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    m = len(xyz)
    if color is None:
        rgb = np.full((m, 3), 255, np.uint8)
    else:
        rgb = np.asarray(color, np.uint8).reshape(m, -1)
        if rgb.shape[1] == 1:
            rgb = np.repeat(rgb, 3, 1)
        if rgb.shape[1] != 3:
            raise FgoError("write_ply: color is m x 3 or m")
    nrm = None
    if normals is not None:
        nrm = np.asarray(normals, np.float64)
        if nrm.shape != (m, 3):
            raise FgoError("write_ply: normals is m x 3")
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % m)
        if nrm is not None:
            f.write("property float nx\nproperty float ny\nproperty float nz\n")
        f.write("property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        if nrm is None:
            for p, c in zip(xyz, rgb):
                f.write("%.9g %.9g %.9g %d %d %d\n" % (p[0], p[1], p[2], c[0], c[1], c[2]))
        else:
            for p, v, c in zip(xyz, nrm, rgb):
                f.write("%.9g %.9g %.9g %.9g %.9g %.9g %d %d %d\n" % (p[0], p[1], p[2], v[0], v[1], v[2], c[0], c[1], c[2]))


def synth_manhattan3d(n_poses, lookback=5, n_loop=4, seed=42, sigma_t=0.02, sigma_q=0.005):
    """SURVEY.md §8d generator (host-only).  Returns dict of numpy arrays."""
    max_e = int(n_poses) * (1 + lookback + n_loop)
    init = np.zeros((n_poses, 7)); truth = np.zeros((n_poses, 7))
    ei = np.zeros(max_e, np.int64); ej = np.zeros(max_e, np.int64)
    meas = np.zeros((max_e, 7)); info = np.zeros((max_e, 21))
    e = lib.fgo_synth_manhattan3d(n_poses, lookback, n_loop, seed, sigma_t, sigma_q, _dp(init), _dp(truth),
                                  _i64p(ei), _i64p(ej), _dp(meas), _dp(info), max_e)
    if e < 0:
        raise FgoError("fgo_synth_manhattan3d failed: %d" % e)
    return dict(poses=init, truth=truth, ei=ei[:e].copy(), ej=ej[:e].copy(), meas=meas[:e].copy(), info=info[:e].copy())


def dist_unique_id():
    """ncclGetUniqueId through libfgo's run-time RCCL binding: 128 bytes rank 0 hands to every rank (Graph.init_rccl)"""
    buf = (C.c_char * 128)()
    rc = lib.fgo_dist_unique_id(C.cast(buf, C.c_void_p))
    if rc < 0:
        raise FgoError("fgo_dist_unique_id failed: %d (librccl not loadable?)" % rc)
    return bytes(buf)


def debug_partition(n, a, b, world):
    """host-only: group (owning rank, or `world` for the top) of every vertex of a block graph under fgo_set_shard(., world)"""
    a = np.ascontiguousarray(a, np.int32); b = np.ascontiguousarray(b, np.int32)
    out = np.zeros(n, np.int32)
    ip = C.POINTER(C.c_int)
    rc = lib.fgo_debug_partition(n, len(a), a.ctypes.data_as(ip), b.ctypes.data_as(ip), world, out.ctypes.data_as(ip))
    if rc < 0:
        raise FgoError("fgo_debug_partition failed: %d" % rc)
    return out


class _DevArray:
    """exposes a raw device pointer through __cuda_array_interface__ so torch can wrap it without a copy"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": (int(n),), "typestr": "<f8", "version": 2}


def device_tensor(ptr, n, device=0):
    """torch.float64 view of `n` doubles at device address `ptr` (plumbing for the multi-GPU all-reduce hook)"""
    import torch
    return torch.as_tensor(_DevArray(ptr, n), device=torch.device("cuda", device))


def torch_allreduce_hook(device=0):
    """all-reduce hook for Graph.set_shard backed by torch.distributed (backend "nccl" is RCCL on ROCm)"""
    import torch
    import torch.distributed as dist

    def hook(ptr, n):
        t = device_tensor(ptr, n, device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        torch.cuda.synchronize(device)
        return 0
    return hook


PREINT_DOUBLES = 287        # fgo_preint: dt, dR[4], dp[3], dv[3], 5 x 3x3 bias Jacobians, bhat[6], cov[225]
IMU_PARAM_DOUBLES = 9        # fgo_imu_params: 6 variances + gravity[3]


class Preintegrator:
    """Host-side mirror of the reference's imu_interface (fgo_preint_*): integrates (acc, gyro, dt) samples"""

    def __init__(self, bias_hat=None, params=None):
        self.params = np.zeros(IMU_PARAM_DOUBLES)
        lib.fgo_imu_params_vn100(_dp(self.params))
        if params is not None:
            self.params[:] = params
        self.buf = np.zeros(PREINT_DOUBLES)
        self.reset(np.zeros(6) if bias_hat is None else bias_hat)

    def reset(self, bias_hat):
        b = np.ascontiguousarray(bias_hat, np.float64)
        lib.fgo_preint_reset(_dp(self.buf), _dp(b))

    def integrate(self, acc, gyro, dt):
        a = np.ascontiguousarray(acc, np.float64); w = np.ascontiguousarray(gyro, np.float64)
        lib.fgo_preint_integrate(_dp(self.buf), _dp(self.params), _dp(a), _dp(w), dt)

    @property
    def gravity(self):
        return self.params[6:9]

    def predict(self, pose_i, vel_i, bias_i):
        xi, vi, bi = (np.ascontiguousarray(a, np.float64) for a in (pose_i, vel_i, bias_i))
        xj = np.zeros(7); vj = np.zeros(3); g = np.ascontiguousarray(self.gravity)
        lib.fgo_preint_predict(_dp(self.buf), _dp(g), _dp(xi), _dp(vi), _dp(bi), _dp(xj), _dp(vj))
        return xj, vj


class Graph:
    """Thin RAII wrapper over fgo_ctx (one per thread, like the reference's wrappers)."""

    def __init__(self, device=0, verbose=0, nd_leaf=0, order_candidates=0):
        cfg = FgoConfig()
        cfg.device, cfg.verbose, cfg.nd_leaf, cfg.order_candidates = device, verbose, nd_leaf, order_candidates
        self._h = lib.fgo_create(C.byref(cfg))
        if not self._h:
            raise FgoError("fgo_create failed: %s" % lib.fgo_last_error(None).decode())

    def close(self):
        if getattr(self, "_h", None):
            if lib is not None:                  # (module globals are already cleared at interpreter shutdown)
                lib.fgo_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc < 0:
            raise FgoError("fgo error %d: %s" % (rc, lib.fgo_last_error(self._h).decode()))
        return rc

    def add_poses(self, poses7, fixed=None, ids=None):
        poses7 = np.ascontiguousarray(poses7, np.float64)
        n = poses7.shape[0]
        fx = None if fixed is None else np.ascontiguousarray(fixed, np.uint8)
        idp = None if ids is None else _i64p(np.ascontiguousarray(ids, np.int64))
        self._chk(lib.fgo_add_poses(self._h, n, idp, _dp(poses7),
                                    None if fx is None else fx.ctypes.data_as(C.POINTER(C.c_ubyte))))

    def add_edges(self, ei, ej, meas7, info21, tangent_order=FGO_TANGENT_G2O):
        ei = np.ascontiguousarray(ei, np.int64); ej = np.ascontiguousarray(ej, np.int64)
        meas7 = np.ascontiguousarray(meas7, np.float64); info21 = np.ascontiguousarray(info21, np.float64)
        self._chk(lib.fgo_add_edges_se3(self._h, len(ei), _i64p(ei), _i64p(ej), _dp(meas7), _dp(info21), tangent_order))

    def set_pose(self, pid, pose7):
        p = np.ascontiguousarray(pose7, np.float64)
        self._chk(lib.fgo_set_pose(self._h, pid, _dp(p[:3].copy()), _dp(p[3:].copy())))

    def get_poses(self, n=None, ids=None):
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int64); n = len(ids)
        elif n is None:
            n = lib.fgo_num_poses(self._h)
        out = np.zeros((n, 7))
        self._chk(lib.fgo_get_poses(self._h, n, None if ids is None else _i64p(ids), _dp(out)))
        return out

    def chi2(self):
        v = lib.fgo_chi2(self._h)
        if v != v:
            raise FgoError("fgo_chi2 failed: %s" % lib.fgo_last_error(self._h).decode())
        return v

    def optimize(self, iters):
        st = FgoStats()
        rc = self._chk(lib.fgo_optimize(self._h, iters, C.byref(st)))
        return rc, st

    # ---- GTSAM-semantics graph
    def add_prior(self, pid, pose7, info21):
        p = np.ascontiguousarray(pose7, np.float64); w = np.ascontiguousarray(info21, np.float64)
        self._chk(lib.fgo_add_prior_pose(self._h, pid, _dp(p[:3].copy()), _dp(p[3:].copy()), _dp(w)))

    # ---- multi-GPU shard mode
    def set_shard(self, rank, world, allreduce=None):
        """allreduce(ptr: int, count: int) -> 0 must sum `count` doubles at device address `ptr` over all ranks in place"""
        self._chk(lib.fgo_set_shard(self._h, rank, world))
        self.rank, self.world = rank, world
        if allreduce is not None:
            self._ar_cb = ALLREDUCE_FN(lambda user, ptr, n: int(allreduce(ptr, n) or 0))   # keep a reference alive
            self._chk(lib.fgo_set_allreduce(self._h, self._ar_cb, None))

    def init_rccl(self, id128):
        """RCCL transport for the collectives of the distributed mode (after set_shard); id128: bytes from dist_unique_id()"""
        buf = (C.c_char * 128).from_buffer_copy(bytes(id128))
        self._chk(lib.fgo_dist_init_rccl(self._h, C.cast(buf, C.c_void_p)))

    def debug_allreduce(self, a):
        a = np.ascontiguousarray(a, np.float64).copy()
        self._chk(lib.fgo_debug_allreduce(self._h, _dp(a), a.size))
        return a

    def read_system(self):
        st = FgoStats()
        self._chk(lib.fgo_debug_read_system(self._h, None, None, None))              # builds the structure (no collective)
        self._chk(lib.fgo_get_stats(self._h, C.byref(st)))
        H = np.zeros(int(st.nnz_H_blocks) * 36); b = np.zeros(int(st.n_free) * 6); chi = C.c_double()
        self._chk(lib.fgo_debug_read_system(self._h, _dp(H), _dp(b), C.byref(chi)))
        return H, b, chi.value

    def read_reduced(self, lam=0.0):
        """dense reduced camera system (S, g) of a structure with the landmarks eliminated (fgo_debug_read_reduced)"""
        n = C.c_int64()
        self._chk(lib.fgo_debug_read_reduced(self._h, lam, None, None, C.byref(n)))
        m = 6 * int(n.value)
        S, g = np.zeros((m, m)), np.zeros(m)
        self._chk(lib.fgo_debug_read_reduced(self._h, lam, _dp(S), _dp(g), C.byref(n)))
        return S, g

    def add_vec3(self, pid, xyz):
        self._chk(lib.fgo_add_vec3(self._h, pid, _dp(np.ascontiguousarray(xyz, np.float64))))

    def add_bias(self, pid, b6):
        self._chk(lib.fgo_add_bias(self._h, pid, _dp(np.ascontiguousarray(b6, np.float64))))

    def add_prior_vec3(self, pid, xyz, sigma):
        self._chk(lib.fgo_add_prior_vec3(self._h, pid, _dp(np.ascontiguousarray(xyz, np.float64)), sigma))

    def add_prior_bias(self, pid, b6, sigma):
        self._chk(lib.fgo_add_prior_bias(self._h, pid, _dp(np.ascontiguousarray(b6, np.float64)), sigma))

    def set_gravity(self, g3):
        self._chk(lib.fgo_set_gravity(self._h, _dp(np.ascontiguousarray(g3, np.float64))))

    def add_imu(self, ids6, preint_buf):
        ids = np.ascontiguousarray(ids6, np.int64); buf = np.ascontiguousarray(preint_buf, np.float64)
        assert len(buf) == PREINT_DOUBLES
        self._chk(lib.fgo_add_imu_combined(self._h, _i64p(ids), _dp(buf)))

    def marginal_cov(self, pid):
        out = np.zeros((6, 6))
        self._chk(lib.fgo_marginal_cov(self._h, pid, _dp(out)))
        return out

    def marginal_cov_many(self, ids):
        ids = np.ascontiguousarray(ids, np.int64)
        out = np.zeros((len(ids), 6, 6))
        self._chk(lib.fgo_marginal_cov_many(self._h, len(ids), _i64p(ids), _dp(out)))
        return out

    def marginal_cov_all(self):
        """(ids, cov[n, 6, 6]): the marginal covariance of every free variable from one selected inversion"""
        n = self._chk(lib.fgo_marginal_cov_all(self._h, 0, None, None))
        ids = np.zeros(n, np.int64)
        out = np.zeros((n, 6, 6))
        self._chk(lib.fgo_marginal_cov_all(self._h, n, _i64p(ids), _dp(out)))
        return ids, out

    def marginal_cov_pairs(self, a, b):
        """cov[n, 6, 6]: Cov(x_a[k], x_b[k]), rows in a's tangent, columns in b's"""
        a = np.ascontiguousarray(a, np.int64); b = np.ascontiguousarray(b, np.int64)
        assert a.shape == b.shape and a.ndim == 1
        out = np.zeros((len(a), 6, 6))
        self._chk(lib.fgo_marginal_cov_pairs(self._h, len(a), _i64p(a), _i64p(b), _dp(out)))
        return out

    def joint_marginal_cov(self, ids):
        """dense (6n x 6n) joint covariance of the variables `ids` (GTSAM Marginals::jointMarginalCovariance)"""
        ids = np.ascontiguousarray(ids, np.int64)
        n = len(ids)
        ia, ib = np.triu_indices(n)
        blk = self.marginal_cov_pairs(ids[ia], ids[ib])
        J = np.zeros((6 * n, 6 * n))
        for k in range(len(ia)):
            i, j = ia[k], ib[k]
            J[6 * i:6 * i + 6, 6 * j:6 * j + 6] = blk[k]
            J[6 * j:6 * j + 6, 6 * i:6 * i + 6] = blk[k].T
        return J

    def selinv_stats(self):
        """timings of the last selected inversion (fgo_debug_selinv_stats)"""
        out = np.zeros(7)
        self._chk(lib.fgo_debug_selinv_stats(self._h, _dp(out)))
        return dict(t_lists_s=out[0], list_bytes=int(out[1]), ms_factor=out[2], ms_prep=out[3], ms_sweep=out[4], entries=int(out[5]),
                    fallback_pairs=int(out[6]))

    def selinv_census(self):
        """what a selected inversion of the built structure launches (fgo_debug_selinv_census; nothing runs): per sweep form
        ('w16', 'w4') launches, workgroups, columns, max_m, wrap_cols (m > 160 / 40) and max_task_cols; nb, empty_cols (m == 0),
        prep_workgroups and the device's compute units"""
        out = np.zeros(16, np.int64)
        self._chk(lib.fgo_debug_selinv_census(self._h, _i64p(out)))
        keys = ("launches", "workgroups", "columns", "max_m", "wrap_cols", "max_task_cols")
        return dict(w16=dict(zip(keys, (int(v) for v in out[0:6]))), w4=dict(zip(keys, (int(v) for v in out[6:12]))),
                    nb=int(out[12]), empty_cols=int(out[13]), prep_workgroups=int(out[14]), cus=int(out[15]))

    def gate_edges(self, a, b, meas7, info21, tangent_order=FGO_TANGENT_G2O, want_cov=False):
        """(d2, chi2[, P]) of candidate SE3 edges a[k] -> b[k] at the current estimate; nothing is added to the graph.
        d2: squared Mahalanobis distance of the innovation under the map's covariance (chi-square, 6 dof, for a correct
        candidate), chi2 = e' Omega e, P[n, 6, 6] = [Ja Jb] Sigma [Ja Jb]'."""
        a = np.ascontiguousarray(a, np.int64); b = np.ascontiguousarray(b, np.int64)
        assert a.shape == b.shape and a.ndim == 1
        n = len(a)
        meas7 = np.ascontiguousarray(meas7, np.float64).reshape(n, 7); info21 = np.ascontiguousarray(info21, np.float64).reshape(n, 21)
        d2 = np.zeros(n); chi2 = np.zeros(n)
        P = np.zeros((n, 6, 6)) if want_cov else None
        self._chk(lib.fgo_gate_edges_se3(self._h, n, _i64p(a), _i64p(b), _dp(meas7), _dp(info21), tangent_order, _dp(d2), _dp(chi2),
                                         _dp(P) if want_cov else None))
        return (d2, chi2, P) if want_cov else (d2, chi2)

    def edge_chi2(self, first=0, n=None):
        """e' Omega e of the SE3 edges [first, first + n) in the order they were added (n = None: all from `first`)"""
        if n is None:
            n = max(0, lib.fgo_num_edges(self._h) - first)
        out = np.zeros(n)
        self._chk(lib.fgo_edge_chi2_se3(self._h, first, n, _dp(out)))
        return out

    def gate_plane_factors(self, pose, plane, z, cov6, want_cov=False, want_resid=False):
        """(d2, chi2, cos[, P][, e]) of candidate plane observations pose[k] -> plane[k] at the current estimate (GTSAM semantics);
        nothing is added to the graph.  z[n, 4]: measured plane in the pose frame, cov6[n, 6]: upper triangle of its 3x3 covariance,
        both as add_plane_factor takes them.  d2: squared Mahalanobis distance of the innovation under the map's covariance
        (chi-square, 3 dof, for a correct association), chi2 = e' S^-1 e, cos: cosine between predicted and measured normal,
        P[n, 3, 3] = [Jx Jp] Sigma [Jx Jp]', e[n, 3] the residual."""
        pose = np.ascontiguousarray(pose, np.int64); plane = np.ascontiguousarray(plane, np.int64)
        assert pose.shape == plane.shape and pose.ndim == 1
        n = len(pose)
        z = np.ascontiguousarray(z, np.float64).reshape(n, 4); cov6 = np.ascontiguousarray(cov6, np.float64).reshape(n, 6)
        d2 = np.zeros(n); chi2 = np.zeros(n); cos = np.zeros(n)
        P = np.zeros((n, 3, 3)) if want_cov else None
        e = np.zeros((n, 3)) if want_resid else None
        self._chk(lib.fgo_gate_plane_factors(self._h, n, _i64p(pose), _i64p(plane), _dp(z), _dp(cov6), _dp(d2), _dp(chi2), _dp(cos),
                                             _dp(e) if want_resid else None, _dp(P) if want_cov else None))
        return (d2, chi2, cos) + ((P,) if want_cov else ()) + ((e,) if want_resid else ())

    def associate_planes(self, pose, z, cov6, plane_ids, d2_gate=7.815, cos_min=-1.0, want_matrix=False):
        """(match, best2[, d2_matrix]): k plane observations z[k, 4] / cov6[k, 6] made from `pose` against the distinct planes
        plane_ids[m].  match[k]: the plane with the smallest d2 if that is < d2_gate (7.815 = chi-square 3 dof, 95 %), else -1;
        best2[k, 2]: smallest and second smallest d2 (+inf when absent); d2_matrix[k, m]: +inf where cos < cos_min or a covariance
        is not positive definite.  A tie goes to the earlier entry of plane_ids."""
        z = np.ascontiguousarray(z, np.float64).reshape(-1, 4)
        k = len(z)
        cov6 = np.ascontiguousarray(cov6, np.float64).reshape(k, 6)
        plane_ids = np.ascontiguousarray(plane_ids, np.int64).reshape(-1)
        m = len(plane_ids)
        match = np.full(k, -1, np.int64); best2 = np.full((k, 2), np.inf)
        D = np.full((k, m), np.inf) if want_matrix else None
        self._chk(lib.fgo_associate_planes(self._h, int(pose), k, _dp(z), _dp(cov6), m, _i64p(plane_ids), d2_gate, cos_min,
                                           _i64p(match), _dp(best2), _dp(D) if want_matrix else None))
        return (match, best2, D) if want_matrix else (match, best2)

    def gate_stats(self):
        """figures of the last gate call of either kind (fgo_debug_gate_stats)"""
        out = np.zeros(4)
        self._chk(lib.fgo_debug_gate_stats(self._h, _dp(out)))
        return dict(off_pattern=int(out[0]), column_groups=int(out[1]), ms_kernel=out[2], ms_solves=out[3])

    def add_plane(self, pid, abcd):
        a = np.ascontiguousarray(abcd, np.float64)
        self._chk(lib.fgo_add_plane(self._h, pid, _dp(a)))

    def add_plane_factor(self, pose_id, plane_id, z_abcd, cov_ut6):
        z = np.ascontiguousarray(z_abcd, np.float64); s = np.ascontiguousarray(cov_ut6, np.float64)
        self._chk(lib.fgo_add_plane_factor(self._h, pose_id, plane_id, _dp(z), _dp(s)))

    def add_point(self, pid, xyz):
        a = np.ascontiguousarray(xyz, np.float64)
        self._chk(lib.fgo_add_point3(self._h, pid, _dp(a)))

    def add_prior_point(self, pid, xyz, sigma):
        a = np.ascontiguousarray(xyz, np.float64)
        self._chk(lib.fgo_add_prior_point3(self._h, pid, _dp(a), sigma))

    def set_calibration(self, calib9, body_P_sensor7=None):
        c9 = [float(x) for x in calib9]
        b = None if body_P_sensor7 is None else _dp(np.ascontiguousarray(body_P_sensor7, np.float64))
        self._chk(lib.fgo_set_calib_ds2(self._h, *c9, b))

    def add_reproj(self, pose_id, point_id, uv, sigma=1.0):
        a = np.ascontiguousarray(uv, np.float64)
        self._chk(lib.fgo_add_reproj(self._h, pose_id, point_id, _dp(a), sigma))

    def optimize_gtsam(self, max_iters=100):
        st = FgoStats()
        rc = self._chk(lib.fgo_optimize_gtsam(self._h, max_iters, C.byref(st)))
        return rc, st

    def isam2_update(self, relinearize_threshold=0.1):
        """ISAM2::update(new factors, new values) + calculateEstimate() (gtsam_graph.cpp:1768-1776)"""
        st = FgoStats()
        self._chk(lib.fgo_isam2_update(self._h, relinearize_threshold, C.byref(st)))
        return st

    def isam2_set_wildfire(self, threshold):
        """ISAM2Params::wildfireThreshold analogue; 0 (default) = exact back-substitution"""
        self._chk(lib.fgo_isam2_set_wildfire(self._h, threshold))

    def isam2_reserve(self, reserve_variables, window=0):
        self._chk(lib.fgo_isam2_reserve(self._h, reserve_variables, window))

    def set_growth(self, reserve_variables, window=0):
        """growth reserve of a g2o-semantics context (fgo_set_growth): new vertices / local edges without a structure rebuild"""
        self._chk(lib.fgo_set_growth(self._h, reserve_variables, window))

    def isam2_reset(self):
        self._chk(lib.fgo_isam2_reset(self._h))

    def isam2_state(self, pid):
        th = np.zeros(7); de = np.zeros(6)
        self._chk(lib.fgo_isam2_get_state(self._h, pid, _dp(th), _dp(de)))
        return th, de

    def error(self):
        v = lib.fgo_error(self._h)
        if v != v:
            raise FgoError("fgo_error failed: %s" % lib.fgo_last_error(self._h).decode())
        return v

    def trace(self, cap=256):
        a = np.zeros(cap); b = np.zeros(cap)
        m = self._chk(lib.fgo_trace(self._h, _dp(a), _dp(b), cap))
        return a[:m], b[:m]

    def linearize(self, dense=True):
        chi = C.c_double(); nf = C.c_int64()
        if not dense:
            self._chk(lib.fgo_linearize(self._h, C.byref(chi), None, None, C.byref(nf)))
            return chi.value, None, None
        self._chk(lib.fgo_linearize(self._h, C.byref(chi), None, None, C.byref(nf)))
        m = 6 * nf.value
        H = np.zeros((m, m)); b = np.zeros(m)
        self._chk(lib.fgo_linearize(self._h, C.byref(chi), _dp(H), _dp(b), C.byref(nf)))
        return chi.value, H, b

    def solve_step(self, lam):
        chi = C.c_double(); nf = C.c_int64()
        self._chk(lib.fgo_linearize(self._h, C.byref(chi), None, None, C.byref(nf)))
        d = np.zeros(6 * nf.value)
        self._chk(lib.fgo_solve_step(self._h, lam, _dp(d)))
        return d

    def solve_fused(self, lam):
        """the damped solve as an LM trial runs it: forward solve fused into the factor sweep (fgo_debug_solve_fused)"""
        chi = C.c_double(); nf = C.c_int64()
        self._chk(lib.fgo_linearize(self._h, C.byref(chi), None, None, C.byref(nf)))
        d = np.zeros(6 * nf.value)
        self._chk(lib.fgo_debug_solve_fused(self._h, lam, _dp(d)))
        return d

    def launch_census(self, fused=True):
        """what one factor + solve launches (fgo_debug_launch_census; nothing runs): dict with 'forms' {instantiation:
        (launches, workgroups, work items)}, 'level_riders', 'level_long' (per schedule level), 'chain_on', 'chain_mode'"""
        ip = C.POINTER(C.c_int)
        names = C.create_string_buffer(4096)
        n = self._chk(lib.fgo_debug_launch_census(self._h, int(fused), None, None, None, 0, None, None, 0, None, names, len(names)))
        nl = int(self.stats().n_levels)
        la = np.zeros(n, np.int64); wg = np.zeros(n, np.int64); it = np.zeros(n, np.int64)
        lr = np.zeros(max(nl, 1), np.int32); ll = np.zeros(max(nl, 1), np.int32); ch = np.zeros(2, np.int32)
        self._chk(lib.fgo_debug_launch_census(self._h, int(fused), _i64p(la), _i64p(wg), _i64p(it), n, lr.ctypes.data_as(ip), ll.ctypes.data_as(ip), nl,
                                              ch.ctypes.data_as(ip), None, 0))
        keys = names.value.decode().split("\n")[:n]
        return dict(forms={k: (int(a), int(w), int(i)) for k, a, w, i in zip(keys, la, wg, it)}, level_riders=[int(v) for v in lr[:nl]],
                    level_long=[int(v) for v in ll[:nl]], chain_on=bool(ch[0]), chain_mode=int(ch[1]))

    def isam2_last(self):
        """what the last isam2_update ran (fgo_debug_isam_last): dict with 'sweep' (0 full, 1 masked, 2 ranged), 'cut', 'chain_low', per level
        'level_lo' / 'level_hi' / 'level_ntask' / 'level_fwd' / 'level_fwtab', per task 'task_level' / 'task_dirty' / 'task_run', per variable in the order added
        'var_task' / 'var_chg' / 'delta' [n, 6]"""
        ip = C.POINTER(C.c_int)
        info = np.zeros(5, np.int32)
        n = self._chk(lib.fgo_debug_isam_last(self._h, info.ctypes.data_as(ip), None, None, None, None, None, 0, None, None, None, 0, None, None, None, 0))
        nl, nt = int(info[2]), int(info[3])
        lo = np.zeros(max(nl, 1), np.int32); hi = np.zeros(max(nl, 1), np.int32); cnt = np.zeros(max(nl, 1), np.int32)
        fw = np.zeros(max(nl, 1), np.int32); ft = np.zeros(max(nl, 1), np.int32)
        tl = np.zeros(max(nt, 1), np.int32); td = np.zeros(max(nt, 1), np.uint8); tr = np.zeros(max(nt, 1), np.uint8)
        vt = np.zeros(max(n, 1), np.int32); vc = np.zeros(max(n, 1), np.uint8); de = np.zeros((max(n, 1), 6))
        cp = lambda a: a.ctypes.data_as(C.c_char_p)
        self._chk(lib.fgo_debug_isam_last(self._h, info.ctypes.data_as(ip), lo.ctypes.data_as(ip), hi.ctypes.data_as(ip), cnt.ctypes.data_as(ip),
                                          fw.ctypes.data_as(ip), ft.ctypes.data_as(ip), nl,
                                          tl.ctypes.data_as(ip), cp(td), cp(tr), nt, vt.ctypes.data_as(ip), cp(vc), _dp(de), n))
        return dict(sweep=int(info[0]), cut=bool(info[1]), chain_low=int(info[4]), level_lo=lo[:nl], level_hi=hi[:nl], level_ntask=cnt[:nl], level_fwd=fw[:nl], level_fwtab=ft[:nl], task_level=tl[:nt],
                    task_dirty=td[:nt], task_run=tr[:nt], var_task=vt[:n], var_chg=vc[:n], delta=de[:n])

    LINEARIZE_CENSUS = ("n_hubs", "n_hub_vars", "n_hub_multi", "hub_deg", "hub_cap", "n_dup_groups", "n_dup_members", "n_priors",
                        "n_phantom", "imu_ncolor", "maskable", "structure_rebuilt")

    def linearize_census(self):
        """what the next linearisation launches (fgo_debug_linearize_census; nothing runs): dict of the counts in LINEARIZE_CENSUS"""
        out = np.zeros(12, np.int64)
        self._chk(lib.fgo_debug_linearize_census(self._h, _i64p(out)))
        return {k: int(v) for k, v in zip(self.LINEARIZE_CENSUS, out)}

    def bench_phase(self, phase, reps):
        ms = C.c_double()
        self._chk(lib.fgo_bench_phase(self._h, phase, reps, C.byref(ms)))
        return ms.value

    def stats(self):
        st = FgoStats()
        self._chk(lib.fgo_get_stats(self._h, C.byref(st)))
        return st
