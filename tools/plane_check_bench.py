"""Plane check of visual-odometry records (gtsam/test_plane_check_vo.cpp computePlaneNodeDis / computePlaneDis), batched.  One JSON
line:
  batch_ms / batch_us_per_record      wall time of ONE fgo_plane_check_vro_batch call over all records (uploads and downloads of
                                      every output included), median of --reps calls after a warm-up call
Records: consistent records with --planes planes in either frame, all of them shared, the j-list in random order (a vectorised
form of the generator of tests/plane_check_reference.py: noise drawn from the covariances the check is told).
    python tools/plane_check_bench.py [--records 4096] [--planes 4] [--reps 31] [--mode info|cov]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graph_slam_amd as G  # noqa: E402


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rot(q, v):
    """rotate v (..., 3) by the unit quaternion q (..., 4, xyzw)"""
    u, w = q[..., :3], q[..., 3:]
    return v + 2 * np.cross(u, np.cross(u, v) + w * v)


def records(n, m, seed=7):
    rng = np.random.default_rng(seed)
    w = _unit(rng.normal(size=(n, 3))) * rng.uniform(0, 0.3, (n, 1)); th = np.linalg.norm(w, axis=1, keepdims=True)
    q = np.concatenate([np.sin(0.5 * th) / th * w, np.cos(0.5 * th)], 1); t = rng.uniform(-0.3, 0.3, (n, 3))
    pose = np.concatenate([t, q], 1)
    A = rng.normal(size=(n, 6, 6)); D = np.array([0.005] * 3 + [0.01] * 3)
    cov = (A @ A.transpose(0, 2, 1) / 6 + 0.5 * np.eye(6)) * D[:, None] * D[None, :]
    info = np.linalg.inv(cov)[:, np.triu_indices(6)[0], np.triu_indices(6)[1]]
    # true planes: the normals of one record lie at least ~35 deg apart (perturbed vertices of a cube's axes and diagonals)
    dirs = _unit(np.array([[1, 0.2, 0.1], [0.1, 1, 0.2], [0.2, 0.1, 1], [1, 1, 1], [1, -1, 0.3], [-1, 0.3, 1], [0.3, 1, -1], [1, -1, -1]], float))
    assert m <= len(dirs)
    n_i = _unit(dirs[None, :m] + 0.03 * rng.normal(size=(n, m, 3))); d_i = rng.uniform(0.5, 3.0, (n, m))
    conj = q * np.array([-1, -1, -1, 1.0])
    n_j = _rot(conj[:, None, :], n_i); d_j = np.einsum("nmk,nk->nm", n_i, t) + d_i
    perm = np.argsort(rng.random((n, m)), 1)
    n_j = np.take_along_axis(n_j, perm[:, :, None], 1); d_j = np.take_along_axis(d_j, perm, 1)
    noisy = lambda nn, dd: np.concatenate([_unit(nn + 0.01 * rng.normal(size=nn.shape)), (dd + 0.01 * rng.normal(size=dd.shape))[..., None]], 2)
    C = np.zeros((n, m, 4, 4)); C[:, :, [0, 1, 2, 3], [0, 1, 2, 3]] = 1e-4
    ptr = np.arange(n + 1, dtype=np.int64) * m
    # the record's pose: the true one retracted by noise from its covariance (translation part to first order)
    xi = np.einsum("nab,nb->na", np.linalg.cholesky(cov), rng.normal(size=(n, 6)))
    a = np.linalg.norm(xi[:, :3], axis=1, keepdims=True)
    dq = np.concatenate([np.sin(0.5 * a) / a * xi[:, :3], np.cos(0.5 * a)], 1)
    qr = np.concatenate([q[:, 3:] * dq[:, :3] + dq[:, 3:] * q[:, :3] + np.cross(q[:, :3], dq[:, :3]),
                         q[:, 3:] * dq[:, 3:] - np.sum(q[:, :3] * dq[:, :3], 1, keepdims=True)], 1)
    pose = np.concatenate([t + _rot(q, xi[:, 3:]), qr], 1)
    return dict(pose=pose, info=info, cov=cov, ptr=ptr, pi=noisy(n_i, d_i).reshape(-1, 4), pj=noisy(n_j, d_j).reshape(-1, 4),
                c=C.reshape(-1, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--planes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--mode", choices=("info", "cov"), default="info")
    a = ap.parse_args()
    r = records(a.records, a.planes)
    call = lambda: G.plane_check_vro_batch(r["pose"], r["ptr"], r["pi"], r["c"], r["ptr"], r["pj"], r["c"], **{a.mode: r[a.mode]})
    out = call()                                                               # warm-up: code object load, first allocations
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter(); out = call(); times.append(1e3 * (time.perf_counter() - t0))
    batch_ms = float(np.median(times))
    print(json.dumps(dict(
        records=a.records, planes=a.planes, mode=a.mode, batch_ms=round(batch_ms, 3), batch_us_per_record=round(1e3 * batch_ms / a.records, 4),
        batch_ms_all_reps=[round(t, 3) for t in times], status_ok=int((out["status"] == 0).sum()), matched=int(out["n_matched"].sum()),
        bad=int(out["n_bad"].sum()), err_mean=round(float(out["err"].mean()), 3), err_above_16_27=int((out["err"] > 16.27).sum()))))


if __name__ == "__main__":
    main()
