"""The optimiser of libfgo.so: Graph, the wrapper of an fgo_ctx, and what goes with it -- the host-side IMU preintegrator, the
synthetic pose graph, and the helpers of the multi-GPU mode."""
import ctypes as C

import numpy as np

from ._abi import (ALLREDUCE_FN, FGO_TANGENT_G2O, IMU_PARAM_DOUBLES, PREINT_DOUBLES, FgoConfig, FgoError, FgoStats, _dp, _i64p, call,
                   lib, opt, ptr)


def synth_manhattan3d(n_poses, lookback=5, n_loop=4, seed=42, sigma_t=0.02, sigma_q=0.005):
    """SURVEY.md §8d generator (host-only).  Returns dict of numpy arrays."""
    max_e = int(n_poses) * (1 + lookback + n_loop)
    init = np.zeros((n_poses, 7)); truth = np.zeros((n_poses, 7))
    ei = np.zeros(max_e, np.int64); ej = np.zeros(max_e, np.int64)
    meas = np.zeros((max_e, 7)); info = np.zeros((max_e, 21))
    e = call("fgo_synth_manhattan3d", n_poses, lookback, n_loop, seed, sigma_t, sigma_q, _dp(init), _dp(truth), _i64p(ei), _i64p(ej),
             _dp(meas), _dp(info), max_e)
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
    call("fgo_debug_partition", n, len(a), ptr(a), ptr(b), world, ptr(out))
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
            if lib is not None:                  # (this module's globals are already cleared at interpreter shutdown)
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
        ids = None if ids is None else np.ascontiguousarray(ids, np.int64)
        self._chk(lib.fgo_add_poses(self._h, n, opt(ids), _dp(poses7), opt(fx)))

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

    def _linearize(self, H=None, b=None):
        """fgo_linearize: (chi2, number of free variables); the dense H and b are written where given"""
        chi = C.c_double(); nf = C.c_int64()
        self._chk(lib.fgo_linearize(self._h, C.byref(chi), opt(H), opt(b), C.byref(nf)))
        return chi.value, nf.value

    def linearize(self, dense=True):
        chi, nf = self._linearize()
        if not dense:
            return chi, None, None
        H = np.zeros((6 * nf, 6 * nf)); b = np.zeros(6 * nf)
        return self._linearize(H, b)[0], H, b

    def _solve(self, solver, lam):
        d = np.zeros(6 * self._linearize()[1])
        self._chk(solver(self._h, lam, _dp(d)))
        return d

    def solve_step(self, lam):
        return self._solve(lib.fgo_solve_step, lam)

    def solve_fused(self, lam):
        """the damped solve as an LM trial runs it: forward solve fused into the factor sweep (fgo_debug_solve_fused)"""
        return self._solve(lib.fgo_debug_solve_fused, lam)

    def launch_census(self, fused=True):
        """what one factor + solve launches (fgo_debug_launch_census; nothing runs): dict with 'forms' {instantiation:
        (launches, workgroups, work items)}, 'level_riders', 'level_long' (per schedule level), 'chain_on', 'chain_mode'"""
        names = C.create_string_buffer(4096)
        n = self._chk(lib.fgo_debug_launch_census(self._h, int(fused), None, None, None, 0, None, None, 0, None, names, len(names)))
        nl = int(self.stats().n_levels)
        la = np.zeros(n, np.int64); wg = np.zeros(n, np.int64); it = np.zeros(n, np.int64)
        lr = np.zeros(max(nl, 1), np.int32); ll = np.zeros(max(nl, 1), np.int32); ch = np.zeros(2, np.int32)
        self._chk(lib.fgo_debug_launch_census(self._h, int(fused), _i64p(la), _i64p(wg), _i64p(it), n, ptr(lr), ptr(ll), nl, ptr(ch), None, 0))
        keys = names.value.decode().split("\n")[:n]
        return dict(forms={k: (int(a), int(w), int(i)) for k, a, w, i in zip(keys, la, wg, it)}, level_riders=[int(v) for v in lr[:nl]],
                    level_long=[int(v) for v in ll[:nl]], chain_on=bool(ch[0]), chain_mode=int(ch[1]))

    def isam2_last(self):
        """what the last isam2_update ran (fgo_debug_isam_last): dict with 'sweep' (0 full, 1 masked, 2 ranged), 'cut', 'chain_low', per level
        'level_lo' / 'level_hi' / 'level_ntask' / 'level_fwd' / 'level_fwtab', per task 'task_level' / 'task_dirty' / 'task_run', per variable in the order added
        'var_task' / 'var_chg' / 'delta' [n, 6]"""
        info = np.zeros(5, np.int32)
        n = self._chk(lib.fgo_debug_isam_last(self._h, ptr(info), None, None, None, None, None, 0, None, None, None, 0, None, None, None, 0))
        nl, nt = int(info[2]), int(info[3])
        lo = np.zeros(max(nl, 1), np.int32); hi = np.zeros(max(nl, 1), np.int32); cnt = np.zeros(max(nl, 1), np.int32)
        fw = np.zeros(max(nl, 1), np.int32); ft = np.zeros(max(nl, 1), np.int32)
        tl = np.zeros(max(nt, 1), np.int32); td = np.zeros(max(nt, 1), np.uint8); tr = np.zeros(max(nt, 1), np.uint8)
        vt = np.zeros(max(n, 1), np.int32); vc = np.zeros(max(n, 1), np.uint8); de = np.zeros((max(n, 1), 6))
        self._chk(lib.fgo_debug_isam_last(self._h, ptr(info), ptr(lo), ptr(hi), ptr(cnt), ptr(fw), ptr(ft), nl, ptr(tl), ptr(td), ptr(tr), nt,
                                          ptr(vt), ptr(vc), _dp(de), n))
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
