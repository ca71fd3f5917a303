"""The batched front ends of libfgo.so, one wrapper per call: IMU preintegration, two-view bundle adjustment, the plane and IMU
checks of visual-odometry records, RANSAC registration, plane extraction and propagation, descriptor matching, and the
compositions of them that the reference runs as one step."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import (FGO_FM_DIM, FGO_PX_MAX_PLANES, FGO_VRO_OK, IMU_PARAM_DOUBLES, PREINT_DOUBLES, FgoError, ImuCheckParams, ImuCheckResult,
                   MatchParams, MatchResult, PlaneCheckParams, PlaneCheckResult, PlaneExtractParams, PlaneExtractPlane, PlaneExtractResult,
                   PlanePropagateParams, PlanePropagatePlane, PlanePropagatePred, PlanePropagateResult, TwoViewParams, TwoViewResult,
                   VroParams, VroResult, call, lib, opt, ptr, records)


def _info_or_cov(who, info, cov):
    """the uncertainty of the records of a call that takes exactly one of info (n x 21) and cov (n x 6 x 6): the array, as n x 21
    or n x 36, and the call's two pointer arguments (info, cov), one of them NULL"""
    if (info is None) == (cov is None):
        raise FgoError("%s: exactly one of info (n x 21) and cov (n x 6 x 6)" % who)
    s = np.ascontiguousarray(info if cov is None else cov, np.float64).reshape(-1, 21 if cov is None else 36)
    return s, ((ptr(s), None) if cov is None else (None, ptr(s)))


def _pack_planes(out, ut6):
    """adds to `out` the planes of its abcd_all / cov16_all and of ut6 (n x stride x ...; the first n_planes[f] slots of frame f
    count) packed frame after frame, as plane_check_vro_batch takes them: ptr (n + 1), abcd, cov16 and, unless ut6 is None,
    cov_ut6_all = ut6 and cov_ut6"""
    keep = np.arange(out["abcd_all"].shape[1])[None, :] < out["n_planes"][:, None]
    out["ptr"] = np.concatenate([[0], np.cumsum(out["n_planes"])]).astype(np.int64)
    out["abcd"] = out["abcd_all"][keep]; out["cov16"] = out["cov16_all"][keep].reshape(-1, 16)
    if ut6 is not None:
        out["cov_ut6_all"] = ut6; out["cov_ut6"] = ut6[keep]


def preint_information(buf):
    """fgo_preint_information: the 15x15 information matrix fgo_add_imu_combined derives from a preintegration payload"""
    b = np.ascontiguousarray(buf, np.float64)
    out = np.zeros((15, 15))
    call("fgo_preint_information", ptr(b), ptr(out))
    return out


def preint_batch(sample_ptr, acc, gyro, dt, bias_hat=None, params=None, device=0):
    """fgo_preint_batch: every factor's samples integrated by one wave on the GPU; returns [n, PREINT_DOUBLES]"""
    sp = np.ascontiguousarray(sample_ptr, np.int64)
    n = len(sp) - 1
    a = np.ascontiguousarray(acc, np.float64); w = np.ascontiguousarray(gyro, np.float64)
    if params is None:
        params = np.zeros(IMU_PARAM_DOUBLES); lib.fgo_imu_params_vn100(ptr(params))
    params = np.ascontiguousarray(params, np.float64)
    out = np.zeros((n, PREINT_DOUBLES))
    bh = None if bias_hat is None else np.ascontiguousarray(bias_hat, np.float64)
    call("fgo_preint_batch", device, n, ptr(sp), ptr(a), ptr(w), dt, opt(bh), ptr(params), ptr(out))
    return out


def two_view_params(**kw):
    """fgo_two_view_params_default, with the given fields replaced"""
    return _abi.params(TwoViewParams, **kw)


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
    call("fgo_two_view_ba_batch", device, n, ptr(mp), ptr(x), ptr(a), ptr(b), opt(p0), ptr(c9), opt(bps),
         None if params is None else C.byref(params), ptr(pose_j), ptr(pose_i), ptr(cov), ptr(info), res)
    out = {"pose_j": pose_j, "pose_i": pose_i, "cov": cov, "info": info}
    out.update(records(res, n))
    return out


def plane_check_params(**kw):
    """fgo_plane_check_params_default, with the given fields replaced"""
    return _abi.params(PlaneCheckParams, **kw)


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
    for name, own, abcd, c16 in (("pi", ip, pi_abcd, pi_cov), ("pj", jp, pj_abcd, pj_cov)):
        a = np.ascontiguousarray(abcd, np.float64).reshape(-1, 4); c = np.ascontiguousarray(c16, np.float64).reshape(-1, 16)
        if min(len(a), len(c)) < int(own[-1]):
            raise FgoError("plane_check_vro_batch: %s_ptr names %d planes, the arrays hold fewer" % (name, int(own[-1])))
        planes += [a, c]
    s, info_cov = _info_or_cov("plane_check_vro_batch", info, cov)
    if len(s) != n:
        raise FgoError("plane_check_vro_batch: info / cov needs one entry per record")
    mi = max(int(ip[-1]), 0)
    match = np.zeros(mi, np.int64); d2 = np.zeros(mi); raw = np.zeros(mi); sdj = np.zeros(mi)
    pred = np.zeros((mi, 4)); pcov = np.zeros((mi, 3, 3))
    res = (PlaneCheckResult * max(n, 1))()
    call("fgo_plane_check_vro_batch", device, n, ptr(ps), *info_cov, ptr(ip), ptr(planes[0]), ptr(planes[1]), ptr(jp), ptr(planes[2]),
         ptr(planes[3]), None if params is None else C.byref(params), res, ptr(match), ptr(d2), ptr(raw), ptr(pred), ptr(pcov), ptr(sdj))
    out = {"match": match, "d2": d2, "raw": raw, "pred_abcd": pred, "pred_cov": pcov, "sdj": sdj}
    out.update(records(res, n))
    return out


def chi2_quantile(dof, p):
    """fgo_chi2_quantile: the reference's utils::chi2(dof, alpha), the quantile of chi-square(dof) at probability p"""
    return float(lib.fgo_chi2_quantile(int(dof), float(p)))


def imu_check_params(**kw):
    """fgo_imu_check_params_default, with the given fields replaced"""
    return _abi.params(ImuCheckParams, **kw)


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
    s, info_cov = _info_or_cov("imu_check_vro_batch", info, cov)
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
    call("fgo_imu_check_vro_batch", device, n, ptr(ps), *info_cov, len(pm), ptr(pm), ptr(ix), opt(b), opt(q),
         None if params is None else C.byref(params), res, opt(dw), opt(cdw))
    out = records(res, n)
    if want_dw:
        out["dw"] = dw
    if want_cov:
        out["cov_dw"] = cdw
    return out


def vro_params(**kw):
    """fgo_vro_params_default, with the given fields replaced (sigma_z: three coefficients)"""
    return _abi.params(VroParams, **kw)


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
    call("fgo_vro_ransac_batch", device, n, ptr(mp), ptr(a), ptr(b), C.byref(params), ptr(pose), opt(info), opt(cov), opt(inl), opt(hyp),
         res)
    out = {"pose_ij": pose}
    out.update(records(res, n))
    for k, v in (("info", info), ("cov", cov), ("inliers", inl), ("hyp_counts", hyp)):
        if v is not None:
            out[k] = v
    return out


def plane_extract_params(**kw):
    """fgo_plane_extract_params_default, with the given fields replaced (sigma_z: three coefficients)"""
    return _abi.params(PlaneExtractParams, **kw)


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
    call("fgo_plane_extract_batch", device, n, w, h, ptr(d), C.byref(params), res, ptr(abcd), ptr(cov16), ptr(ut6), planes, opt(lab),
         opt(hyp))
    out = records(res, n)
    out.update(records(planes, n * mp, (n, mp)))
    out.update(abcd_all=abcd, cov16_all=cov16, cov_ut6_all=ut6)
    _pack_planes(out, ut6)
    if lab is not None:
        out["labels"] = lab
    if hyp is not None:
        out["hyp_counts"] = hyp
    return out


def plane_propagate_params(**kw):
    """fgo_plane_propagate_params_default, with the given fields replaced (sigma_z: three coefficients)"""
    return _abi.params(PlanePropagateParams, **kw)


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
    s, info_cov = _info_or_cov("plane_propagate_batch", info, cov)
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
    call("fgo_plane_propagate_batch", device, nf, w, h, ptr(d), ptr(it), ptr(lb), ptr(npl), ptr(a8), ptr(c8), n, ptr(fi), ptr(fj), ptr(ps),
         *info_cov, C.byref(params), res, ptr(abcd_o), ptr(cov16_o), opt(ut6), planes, pred, opt(lab))
    out = records(res, n)
    out.update(abcd_all=abcd_o, cov16_all=cov16_o)
    if planes is not None:
        out.update(records(planes, n * MP, (n, MP)))
    if pred is not None:
        pd = records(pred, n * MP, (n, MP))
        out.update(pred_abcd=pd["abcd"], sdj=pd["sdj"], n_prev=pd["n_prev"], pred_n_seed=pd["n_seed"], kept=pd["kept"])
    _pack_planes(out, ut6)
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
        _pack_planes(out, out["cov_ut6_all"])
    return out


def match_params(**kw):
    """fgo_match_params_default, with the given fields replaced"""
    return _abi.params(MatchParams, **kw)


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
    q_ptr = np.zeros(n + 1, np.int64); mptr = np.zeros(n + 1, np.int64)
    best = np.zeros(Q, np.int32); d1 = np.zeros(Q, np.int32); d2 = np.zeros(Q, np.int32); why = np.zeros(Q, np.uint8)
    idx_i = np.zeros(Q, np.int64); idx_j = np.zeros(Q, np.int64)
    xi = np.zeros((Q, 3)); xj = np.zeros((Q, 3)); ui = np.zeros((Q, 2)); uj = np.zeros((Q, 2))
    dist = np.zeros(T, np.int32) if want_dist else None
    res = (MatchResult * max(n, 1))()
    call("fgo_match_features_batch", device, nf, ptr(fp), ptr(d), ptr(x), ptr(u), n, ptr(fi), ptr(fj), opt(ps), opt(gd), C.byref(params),
         res, ptr(q_ptr), ptr(best), ptr(d1), ptr(d2), ptr(why), ptr(mptr), ptr(idx_i), ptr(idx_j), ptr(xi), ptr(xj), ptr(ui), ptr(uj),
         opt(dist))
    out = records(res, n)
    m = int(mptr[-1])
    out.update(ptr=mptr, idx_i=idx_i[:m], idx_j=idx_j[:m], xyz_i=xi[:m], xyz_j=xj[:m], uv_i=ui[:m], uv_j=uj[:m], q_ptr=q_ptr, best=best,
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
