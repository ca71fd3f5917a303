"""Dense depth alignment of key-frame pairs (include/fgo_dense.h): projective point-to-plane ICP on the depth frames, for the pairs
whose feature registration failed.  The structures and prototypes of that header live here, not in _abi (which is held to
include/fgo.h alone); tests/test_abi_dense_cpu.py holds them to fgo_dense.h."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import FGO_VRO_OK, FgoError, call, lib, opt, ptr, records

FGO_DA_OK, FGO_DA_TOO_FEW, FGO_DA_DEGENERATE, FGO_DA_NUM = 0, 1, 2, 3
FGO_DA_MAX_LEVELS = 3
FGO_DA_MAX_PIXELS = 1 << 24
# the `source` flag of align_failed_records
FGO_DA_SOURCE_VRO, FGO_DA_SOURCE_DENSE, FGO_DA_SOURCE_VOID = 0, 1, 2


class DepthAlignParams(C.Structure):
    c_name = "fgo_depth_align_params"
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("z_scale", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double), ("sigma_px", C.c_double), ("sigma_z", C.c_double * 3),
                ("n_levels", C.c_int), ("skip", C.c_int * 3), ("iters", C.c_int * 3), ("normal_step", C.c_int),
                ("normal_jump", C.c_double), ("max_dist", C.c_double), ("min_cos", C.c_double), ("min_pairs", C.c_int),
                ("eps_rot", C.c_double), ("eps_trans", C.c_double), ("min_pivot", C.c_double)]


class DepthAlignResult(C.Structure):
    c_name = "fgo_depth_align_result"
    _fields_ = [("status", C.c_int), ("n_pairs_used", C.c_int), ("iterations", C.c_int), ("converged", C.c_int), ("rmse", C.c_double),
                ("chi2", C.c_double), ("min_pivot", C.c_double)]


def _prototypes():
    """{function: argtypes, or (restype, argtypes) where it does not return int}, one entry for every function
    include/fgo_dense.h declares and in its order"""
    i, i64, d, P = C.c_int, C.c_int64, C.c_double, C.POINTER
    dp, i64p, u16p = (P(t) for t in (d, i64, C.c_uint16))
    return {
        "fgo_depth_align_params_default": (None, [P(DepthAlignParams)]),
        "fgo_depth_align_batch": [i, i64, i, i, u16p, i64, i64p, i64p, dp, P(DepthAlignParams), dp, dp, dp, dp, P(DepthAlignResult)],
        "fgo_debug_depth_align_kernel_ms": (d, []),
        "fgo_debug_depth_align_form": (i, [i]),
    }


DENSE_PROTOTYPES = _prototypes()
for _name, _proto in DENSE_PROTOTYPES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _proto if isinstance(_proto, tuple) else (C.c_int, _proto)


def depth_align_params(**kw):
    """fgo_depth_align_params_default, with the given fields replaced (sigma_z, skip, iters: three entries each)"""
    return _abi.params(DepthAlignParams, **kw)


def depth_align_batch(depth, frame_i, frame_j, pose_ij=None, params=None, want_cov=True, want_normal_eq=False, device=0):
    """fgo_depth_align_batch: the dense alignment of every pair in one launch, one workgroup per pair.  depth is n_frames x H x W
    uint16 depth words; pair p aligns frame_j[p] (the source) to frame_i[p] (the target) from pose_ij[p] (n x 7, t then q_xyzw;
    None = the identity).  Returns a dict of arrays over the pairs: pose_ij (n x 7, p_i = R p_j + t, as vro_ransac_batch's), info
    (n x 21), status (FGO_DA_*), n_pairs_used, iterations, converged, rmse, chi2, min_pivot, and when asked for cov (n x 6 x 6) and
    normal_eq (n x 28: H upper 21, g 6, chi2 of the first evaluation).  A failed pair carries the void record (identity,
    information 10000)."""
    d = np.ascontiguousarray(depth, np.uint16)
    if d.ndim != 3:
        raise FgoError("depth_align_batch: depth is n_frames x H x W")
    fi = np.ascontiguousarray(frame_i, np.int64).reshape(-1); fj = np.ascontiguousarray(frame_j, np.int64).reshape(-1)
    n = len(fi)
    if len(fj) != n:
        raise FgoError("depth_align_batch: frame_i and frame_j differ in length")
    p0 = None if pose_ij is None else np.ascontiguousarray(pose_ij, np.float64).reshape(-1, 7)
    if p0 is not None and len(p0) != n:
        raise FgoError("depth_align_batch: pose_ij needs one pose per pair")
    if params is None:
        params = depth_align_params()
    pose = np.zeros((n, 7)); info = np.zeros((n, 21))
    cov = np.zeros((n, 6, 6)) if want_cov else None
    neq = np.zeros((n, 28)) if want_normal_eq else None
    res = (DepthAlignResult * max(n, 1))()
    call("fgo_depth_align_batch", device, d.shape[0], d.shape[2], d.shape[1], ptr(d), n, ptr(fi), ptr(fj), opt(p0), C.byref(params),
         ptr(pose), ptr(info), opt(cov), opt(neq), res)
    out = {"pose_ij": pose, "info": info}
    out.update(records(res, n))
    if want_cov:
        out["cov"] = cov
    if want_normal_eq:
        out["normal_eq"] = neq
    return out


def align_failed_records(depth, frame_i, frame_j, vro, pose_ij=None, params=None, device=0):
    """The records of a vro_ransac_batch result whose status is not FGO_VRO_OK, sent through depth_align_batch in one call and merged
    back: vro is that result (pose_ij, info, status), frame_i / frame_j name the depth frames of every record, pose_ij (n x 7, or
    None) the starting poses of the alignment.  Returns a dict over ALL records: pose_ij and info (an OK record's own, bit for bit;
    a repaired one's from the alignment; the void record where the alignment failed too), source (FGO_DA_SOURCE_VRO / _DENSE /
    _VOID), dense_index (the failed records, in order) and dense (depth_align_batch's result for them)."""
    status = np.asarray(vro["status"])
    fi = np.ascontiguousarray(frame_i, np.int64).reshape(-1); fj = np.ascontiguousarray(frame_j, np.int64).reshape(-1)
    if not len(status) == len(fi) == len(fj):
        raise FgoError("align_failed_records: one frame pair per record")
    pose = np.array(vro["pose_ij"], np.float64).reshape(-1, 7); info = np.array(vro["info"], np.float64).reshape(-1, 21)
    source = np.full(len(status), FGO_DA_SOURCE_VRO, np.int32)
    bad = np.flatnonzero(status != FGO_VRO_OK)
    p0 = None if pose_ij is None else np.ascontiguousarray(pose_ij, np.float64).reshape(-1, 7)[bad]
    dense = depth_align_batch(depth, fi[bad], fj[bad], p0, params, want_cov=False, device=device)
    pose[bad] = dense["pose_ij"]; info[bad] = dense["info"]
    source[bad] = np.where(dense["status"] == FGO_DA_OK, FGO_DA_SOURCE_DENSE, FGO_DA_SOURCE_VOID)
    return {"pose_ij": pose, "info": info, "source": source, "dense_index": bad, "dense": dense}
