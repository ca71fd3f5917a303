"""The C ABI of libfgo.so as ctypes: the structs and constants of include/fgo.h, one table of prototypes for every function it
declares, the loaded library, and the helpers the wrapper modules share to pass arrays in and read structs out."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FGO_LIB", os.path.join(_HERE, "libfgo.so"))      # (FGO_LIB: developer A/B of two builds on the same GPU box)

FGO_TANGENT_G2O = 0
FGO_TANGENT_GTSAM = 1


class FgoConfig(C.Structure):
    c_name = "fgo_config"
    _fields_ = [("device", C.c_int), ("verbose", C.c_int), ("ordering", C.c_int), ("nd_leaf", C.c_int), ("order_candidates", C.c_int),
                ("reserved", C.c_int * 11)]


class FgoStats(C.Structure):
    c_name = "fgo_stats"
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
    c_name = "fgo_two_view_params"
    _fields_ = [("pose_prior_sigma", C.c_double), ("point_sigma", C.c_double), ("pixel_sigma", C.c_double),
                ("max_iters", C.c_int), ("min_matches", C.c_int)]


class TwoViewResult(C.Structure):
    c_name = "fgo_two_view_result"
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("trials", C.c_int),
                ("error_initial", C.c_double), ("error_final", C.c_double), ("lambda_final", C.c_double)]


FGO_TV_OK, FGO_TV_TOO_FEW, FGO_TV_NUM = 0, 1, 2


class PlaneCheckParams(C.Structure):
    c_name = "fgo_plane_check_params"
    _fields_ = [("cos_min", C.c_double), ("d_max", C.c_double), ("failed_info00", C.c_double)]


class PlaneCheckResult(C.Structure):
    c_name = "fgo_plane_check_result"
    _fields_ = [("status", C.c_int), ("n_matched", C.c_int), ("n_bad", C.c_int), ("best_i", C.c_int), ("best_j", C.c_int),
                ("reserved", C.c_int), ("err", C.c_double), ("err_raw", C.c_double)]


FGO_PC_OK, FGO_PC_SKIPPED, FGO_PC_NUM = 0, 1, 2


class ImuCheckParams(C.Structure):
    c_name = "fgo_imu_check_params"
    _fields_ = [("d2_gate", C.c_double), ("d2_ref_gate", C.c_double), ("failed_info00", C.c_double)]


class ImuCheckResult(C.Structure):
    c_name = "fgo_imu_check_result"
    _fields_ = [("status", C.c_int), ("reject", C.c_int), ("d2", C.c_double), ("d2_ref", C.c_double), ("angle", C.c_double)]


FGO_IC_OK, FGO_IC_SKIPPED, FGO_IC_NUM = 0, 1, 2


class VroParams(C.Structure):
    c_name = "fgo_vro_params"
    _fields_ = [("hypotheses", C.c_int), ("seed", C.c_uint64), ("max_dist", C.c_double), ("min_side", C.c_double),
                ("rigid_tol", C.c_double), ("refine_rounds", C.c_int), ("min_inliers", C.c_int), ("fx", C.c_double), ("fy", C.c_double),
                ("sigma_px", C.c_double), ("sigma_z", C.c_double * 3)]


class VroResult(C.Structure):
    c_name = "fgo_vro_result"
    _fields_ = [("status", C.c_int), ("n_inliers", C.c_int), ("best_hypothesis", C.c_int), ("best_count", C.c_int),
                ("n_valid", C.c_int), ("rounds", C.c_int), ("rmse", C.c_double)]


FGO_VRO_OK, FGO_VRO_TOO_FEW, FGO_VRO_NUM = 0, 1, 2


class PlaneExtractParams(C.Structure):
    c_name = "fgo_plane_extract_params"
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("z_scale", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("hypotheses", C.c_int), ("seed", C.c_uint64), ("max_dist", C.c_double),
                ("min_area", C.c_double), ("min_pixels", C.c_int), ("max_planes", C.c_int), ("refine_rounds", C.c_int),
                ("sigma_px", C.c_double), ("sigma_z", C.c_double * 3)]


class PlaneExtractResult(C.Structure):
    c_name = "fgo_plane_extract_result"
    _fields_ = [("status", C.c_int), ("n_planes", C.c_int), ("n_valid_pixels", C.c_int), ("rounds_run", C.c_int)]


class PlaneExtractPlane(C.Structure):
    c_name = "fgo_plane_extract_plane"
    _fields_ = [("n_pixels", C.c_int), ("best_hypothesis", C.c_int), ("best_count", C.c_int), ("n_valid_hyp", C.c_int),
                ("fits", C.c_int), ("reserved", C.c_int), ("rmse", C.c_double), ("centroid", C.c_double * 3)]


FGO_PX_OK, FGO_PX_NUM = 0, 2
FGO_PX_MAX_PLANES = 8


class PlanePropagateParams(C.Structure):
    c_name = "fgo_plane_propagate_params"
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("z_scale", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("sigma_px", C.c_double), ("sigma_z", C.c_double * 3),
                ("d_floor", C.c_double), ("intensity_tol", C.c_int), ("keep_ratio", C.c_double), ("rest_ratio", C.c_double)]


class PlanePropagateResult(C.Structure):
    c_name = "fgo_plane_propagate_result"
    _fields_ = [("status", C.c_int), ("n_planes", C.c_int), ("num_added", C.c_int), ("search_rest", C.c_int)]


class PlanePropagatePlane(C.Structure):
    c_name = "fgo_plane_propagate_plane"
    _fields_ = [("n_pixels", C.c_int), ("n_seed", C.c_int), ("source", C.c_int), ("reserved", C.c_int), ("rmse", C.c_double),
                ("centroid", C.c_double * 3)]


class PlanePropagatePred(C.Structure):
    c_name = "fgo_plane_propagate_pred"
    _fields_ = [("abcd", C.c_double * 4), ("sdj", C.c_double), ("n_prev", C.c_int), ("n_seed", C.c_int), ("kept", C.c_int),
                ("reserved", C.c_int)]


FGO_PP_OK, FGO_PP_NUM = 0, 2


class MatchParams(C.Structure):
    c_name = "fgo_match_params"
    _fields_ = [("ratio", C.c_double), ("ratio_test", C.c_int), ("cross_check", C.c_int), ("max_desc_dist2", C.c_int32),
                ("min_matches", C.c_int), ("radius_px", C.c_double), ("max_dist_3d", C.c_double), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double)]


class MatchResult(C.Structure):
    c_name = "fgo_match_result"
    _fields_ = [("status", C.c_int), ("n_query", C.c_int), ("n_train", C.c_int), ("n_matches", C.c_int), ("n_ratio", C.c_int),
                ("n_cross", C.c_int)]


FGO_FM_OK, FGO_FM_TOO_FEW = 0, 1
FGO_FM_DIM, FGO_FM_MAX_FEATURES = 128, 4096


class MapParams(C.Structure):
    c_name = "fgo_map_params"
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("z_scale", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("skip", C.c_int), ("rect", C.c_int * 4), ("leaf", C.c_double),
                ("min_points", C.c_int), ("table_log2", C.c_int)]


class MapResult(C.Structure):
    c_name = "fgo_map_result"
    _fields_ = [("status", C.c_int), ("table_log2", C.c_int), ("n_sampled", C.c_int64), ("n_valid", C.c_int64),
                ("n_out_of_range", C.c_int64), ("n_voxels", C.c_int64), ("n_dropped", C.c_int64)]


FGO_MAP_OK, FGO_MAP_TRUNCATED, FGO_MAP_FULL = 0, 1, 2


class MapCleanParams(C.Structure):
    c_name = "fgo_map_clean_params"
    _fields_ = [("tolerance", C.c_double), ("min_cluster_size", C.c_int), ("max_cluster_size", C.c_int), ("remove_floor", C.c_int),
                ("up_axis", C.c_int), ("up_sign", C.c_int), ("floor_res", C.c_double), ("floor_span", C.c_double),
                ("floor_clearance", C.c_double)]


class MapCleanResult(C.Structure):
    c_name = "fgo_map_clean_result"
    _fields_ = [("n_points", C.c_int64), ("n_out_of_range", C.c_int64), ("n_cells", C.c_int64), ("n_clusters", C.c_int64),
                ("n_clusters_kept", C.c_int64), ("n_after_clusters", C.c_int64), ("n_floor_removed", C.c_int64), ("n_kept", C.c_int64),
                ("floor_bin", C.c_int64), ("floor_bin_points", C.c_int64), ("floor_height", C.c_double)]


class MapNormalsParams(C.Structure):
    c_name = "fgo_map_normals_params"
    _fields_ = [("k", C.c_int), ("max_radius", C.c_double), ("cell", C.c_double), ("viewpoint", C.c_double * 3)]


class MapNormalsResult(C.Structure):
    c_name = "fgo_map_normals_result"
    _fields_ = [("n_points", C.c_int64), ("n_out_of_range", C.c_int64), ("n_cells", C.c_int64), ("n_valid", C.c_int64),
                ("n_few", C.c_int64), ("n_degenerate", C.c_int64)]


class MapRenderParams(C.Structure):
    c_name = "fgo_map_render_params"
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("z_scale", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("splat", C.c_int), ("radius", C.c_double), ("max_half", C.c_int),
                ("agree_tol", C.c_double), ("background", C.c_uint8 * 3)]


class MapRenderView(C.Structure):
    c_name = "fgo_map_render_view"
    _fields_ = [(f, C.c_int64) for f in ("n_valid", "n_drawn", "n_pixels", "n_meas", "n_both", "n_agree", "n_closer", "n_through")]


class MapRenderResult(C.Structure):
    c_name = "fgo_map_render_result"
    _fields_ = [("n_points", C.c_int64), ("n_nonfinite", C.c_int64), ("form", C.c_int), ("tile_rows", C.c_int)]


FGO_MAP_RENDER_TILES, FGO_MAP_RENDER_GLOBAL = 0, 1


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)     # fgo_allreduce_fn


PREINT_DOUBLES = 287        # fgo_preint: dt, dR[4], dp[3], dv[3], 5 x 3x3 bias Jacobians, bhat[6], cov[225]
IMU_PARAM_DOUBLES = 9        # fgo_imu_params: 6 variances + gravity[3]


def _prototypes():
    """{function: argtypes, or (restype, argtypes) where it does not return int}, one entry for every function include/fgo.h
    declares and in its order (tests/test_abi_cpu.py holds the two together).  fgo_ctx * is a void pointer; fgo_preint * and
    fgo_imu_params * are passed as the double arrays they are made of (PREINT_DOUBLES, IMU_PARAM_DOUBLES)."""
    vp, i, i64, u64, d, P = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_double, C.POINTER
    dp, ip, i64p, i32p, i8p, u8p, u16p = (P(t) for t in (d, i, i64, C.c_int32, C.c_int8, C.c_uint8, C.c_uint16))
    return {
        "fgo_create": (vp, [P(FgoConfig)]),
        "fgo_destroy": (None, [vp]),
        "fgo_last_error": (C.c_char_p, [vp]),
        "fgo_version": (C.c_char_p, []),
        "fgo_device_count": [],
        "fgo_add_pose": [vp, i64, dp, dp, i],
        "fgo_set_pose": [vp, i64, dp, dp],
        "fgo_set_fixed": [vp, i64, i],
        "fgo_get_pose": [vp, i64, dp],
        "fgo_has_pose": [vp, i64],
        "fgo_num_poses": (i64, [vp]),
        "fgo_num_edges": (i64, [vp]),
        "fgo_add_poses": [vp, i64, i64p, dp, u8p],
        "fgo_get_poses": [vp, i64, i64p, dp],
        "fgo_add_edge_se3": [vp, i64, i64, dp, dp, dp, i],
        "fgo_add_edges_se3": [vp, i64, i64p, i64p, dp, dp, i],
        "fgo_add_prior_pose": [vp, i64, dp, dp, dp],
        "fgo_add_plane": [vp, i64, dp],
        "fgo_add_plane_factor": [vp, i64, i64, dp, dp],
        "fgo_add_point3": [vp, i64, dp],
        "fgo_add_prior_point3": [vp, i64, dp, d],
        "fgo_set_calib_ds2": [vp] + [d] * 9 + [dp],
        "fgo_add_reproj": [vp, i64, i64, dp, d],
        "fgo_add_points3": [vp, i64, i64p, dp, d],
        "fgo_add_reprojs": [vp, i64, i64p, i64p, dp, d],
        "fgo_two_view_params_default": (None, [P(TwoViewParams)]),
        "fgo_two_view_ba_batch": [i, i64, i64p, dp, dp, dp, dp, dp, dp, P(TwoViewParams), dp, dp, dp, dp, P(TwoViewResult)],
        "fgo_plane_check_params_default": (None, [P(PlaneCheckParams)]),
        "fgo_plane_check_vro_batch": [i, i64, dp, dp, dp, i64p, dp, dp, i64p, dp, dp, P(PlaneCheckParams), P(PlaneCheckResult), i64p,
                                      dp, dp, dp, dp, dp],
        "fgo_plane_extract_params_default": (None, [P(PlaneExtractParams)]),
        "fgo_plane_extract_batch": [i, i64, i, i, u16p, P(PlaneExtractParams), P(PlaneExtractResult), dp, dp, dp, P(PlaneExtractPlane),
                                    i8p, i32p],
        "fgo_debug_plane_extract_kernel_ms": (d, []),
        "fgo_plane_propagate_params_default": (None, [P(PlanePropagateParams)]),
        "fgo_plane_propagate_batch": [i, i64, i, i, u16p, u8p, i8p, i32p, dp, dp, i64, i64p, i64p, dp, dp, dp, P(PlanePropagateParams),
                                      P(PlanePropagateResult), dp, dp, dp, P(PlanePropagatePlane), P(PlanePropagatePred), i8p],
        "fgo_debug_plane_propagate_kernel_ms": (d, []),
        "fgo_chi2_quantile": (d, [i, d]),
        "fgo_imu_params_vn100": (None, [dp]),
        "fgo_preint_reset": (None, [dp, dp]),
        "fgo_preint_integrate": (None, [dp, dp, dp, dp, d]),
        "fgo_preint_predict": (None, [dp] * 7),
        "fgo_preint_batch": [i, i64, i64p, dp, dp, d, dp, dp, dp],
        "fgo_add_vec3": [vp, i64, dp],
        "fgo_add_bias": [vp, i64, dp],
        "fgo_add_prior_vec3": [vp, i64, dp, d],
        "fgo_add_prior_bias": [vp, i64, dp, d],
        "fgo_set_gravity": [vp, dp],
        "fgo_add_imu_combined": [vp, i64p, dp],
        "fgo_preint_information": [dp, dp],
        "fgo_imu_check_params_default": (None, [P(ImuCheckParams)]),
        "fgo_imu_check_vro_batch": [i, i64, dp, dp, dp, i64, dp, i64p, dp, dp, P(ImuCheckParams), P(ImuCheckResult), dp, dp],
        "fgo_vro_params_default": (None, [P(VroParams)]),
        "fgo_vro_ransac_batch": [i, i64, i64p, dp, dp, P(VroParams), dp, dp, dp, u8p, i32p, P(VroResult)],
        "fgo_debug_vro_waves": [i],
        "fgo_debug_vro_kernel_ms": (d, []),
        "fgo_debug_grid_cap": [i],
        "fgo_match_params_default": (None, [P(MatchParams)]),
        "fgo_match_features_batch": [i, i64, i64p, u8p, dp, dp, i64, i64p, i64p, dp, u8p, P(MatchParams), P(MatchResult), i64p, i32p,
                                     i32p, i32p, u8p, i64p, i64p, i64p, dp, dp, dp, dp, i32p],
        "fgo_debug_match_kernel_ms": (d, []),
        "fgo_map_params_default": (None, [P(MapParams)]),
        "fgo_map_fuse_batch": [i, i64, i, i, u16p, u8p, i, dp, dp, P(MapParams), i64, P(MapResult), dp, u8p, i32p, i64p, i64p, dp],
        "fgo_debug_map_fuse_kernel_ms": (d, []),
        "fgo_map_clean_params_default": (None, [P(MapCleanParams)]),
        "fgo_map_clean": [i, i64, dp, P(MapCleanParams), P(MapCleanResult), i32p, u8p, i32p, i64p, dp],
        "fgo_debug_map_clean_kernel_ms": (d, []),
        "fgo_map_normals_params_default": (None, [P(MapNormalsParams)]),
        "fgo_map_normals": [i, i64, dp, P(MapNormalsParams), P(MapNormalsResult), dp, dp, dp, i32p, u8p, i32p, i64p, i64p],
        "fgo_debug_map_normals_kernel_ms": (d, []),
        "fgo_map_render_params_default": (None, [P(MapRenderParams)]),
        "fgo_map_render_batch": [i, i64, dp, u8p, i, i64, dp, dp, dp, i, i, P(MapRenderParams), u16p, P(MapRenderResult),
                                 P(MapRenderView), i32p, i32p, u8p, dp],
        "fgo_debug_map_render_kernel_ms": (d, []),
        "fgo_optimize_gtsam": [vp, i, P(FgoStats)],
        "fgo_isam2_update": [vp, d, P(FgoStats)],
        "fgo_isam2_reserve": [vp, i, i],
        "fgo_set_growth": [vp, i, i],
        "fgo_isam2_set_wildfire": [vp, d],
        "fgo_isam2_reset": [vp],
        "fgo_isam2_get_state": [vp, i64, dp, dp],
        "fgo_error": (d, [vp]),
        "fgo_marginal_cov": [vp, i64, dp],
        "fgo_marginal_cov_many": [vp, i64, i64p, dp],
        "fgo_marginal_cov_all": (i64, [vp, i64, i64p, dp]),
        "fgo_marginal_cov_pairs": [vp, i64, i64p, i64p, dp],
        "fgo_debug_selinv_stats": [vp, dp],
        "fgo_debug_selinv_census": [vp, i64p],
        "fgo_gate_edges_se3": [vp, i64, i64p, i64p, dp, dp, i, dp, dp, dp],
        "fgo_edge_chi2_se3": [vp, i64, i64, dp],
        "fgo_gate_plane_factors": [vp, i64, i64p, i64p, dp, dp, dp, dp, dp, dp, dp],
        "fgo_associate_planes": [vp, i64, i64, dp, dp, i64, i64p, d, d, i64p, dp, dp],
        "fgo_debug_gate_stats": [vp, dp],
        "fgo_optimize": [vp, i, P(FgoStats)],
        "fgo_chi2": (d, [vp]),
        "fgo_trace": [vp, dp, dp, i],
        "fgo_linearize": [vp, dp, dp, dp, i64p],
        "fgo_solve_step": [vp, d, dp],
        "fgo_bench_phase": [vp, i, i, dp],
        "fgo_get_stats": [vp, P(FgoStats)],
        "fgo_synth_manhattan3d": (i64, [i64, i, i, u64, d, d, dp, dp, i64p, i64p, dp, dp, i64]),
        "fgo_set_shard": [vp, i, i],
        "fgo_set_allreduce": [vp, ALLREDUCE_FN, vp],
        "fgo_dist_unique_id": [vp],
        "fgo_dist_init_rccl": [vp, vp],
        "fgo_debug_partition": [i, i64, ip, ip, i, ip],
        "fgo_debug_allreduce": [vp, dp, i64],
        "fgo_shard_range": [i64, i, i, i64p, i64p],
        "fgo_debug_read_scratch": [vp, dp, i64],
        "fgo_debug_read_system": [vp, dp, dp, dp],
        "fgo_debug_read_reduced": [vp, d, dp, dp, i64p],
        "fgo_debug_solve_fused": [vp, d, dp],
        "fgo_debug_launch_census": [vp, i, i64p, i64p, i64p, i, ip, ip, i, ip, C.c_char_p, i],
        "fgo_debug_isam_last": [vp] + [ip] * 6 + [i, ip, u8p, u8p, i, ip, u8p, dp, i64],
        "fgo_debug_linearize_census": [vp, i64p],
    }


PROTOTYPES = _prototypes()


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "graph_slam_amd: %s is missing — build it with `python -m graph_slam_amd.build` "
            "(hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, proto in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = proto if isinstance(proto, tuple) else (C.c_int, proto)
    return lib


lib = _load()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


class FgoError(RuntimeError):
    pass



def ptr(a):
    """the pointer to a numpy array's data, in the ctypes type of its dtype"""
    return a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def opt(a):
    """ptr(a), or NULL for None: an argument the C call may go without"""
    return None if a is None else ptr(a)


def params(struct, **kw):
    """a parameter struct as its fgo_*_params_default fills it, with the given fields replaced; an array field takes a sequence"""
    p = struct()
    getattr(lib, struct.c_name + "_default")(C.byref(p))
    fields = dict(struct._fields_)
    for k, v in kw.items():
        if k not in fields:
            raise TypeError("%s has no field %r" % (struct.c_name, k))
        setattr(p, k, fields[k](*v) if issubclass(fields[k], C.Array) else v)
    return p


def records(buf, n, shape=None):
    """the first n structs of a ctypes array as a dict of numpy columns, each a copy, of the shape `shape` (default: n) + the
    field's own (centroid[3]: + (3,)); the dtype, padding included, is numpy's reading of the Structure; fields named `reserved`
    are left out"""
    r = np.frombuffer(buf, np.dtype(buf._type_), count=n)
    if shape is not None:
        r = r.reshape(shape)
    return {k: r[k].copy() for k in r.dtype.names if k != "reserved"}


def fields(struct):
    """the fields of one result struct as a dict of Python numbers"""
    return {k: getattr(struct, k) for k, _ in struct._fields_ if k != "reserved"}


def call(name, *args):
    """the library's function `name` on args; a negative return is an FgoError that carries it"""
    rc = getattr(lib, name)(*args)
    if rc < 0:
        raise FgoError("%s failed: %d" % (name, rc))
    return rc
