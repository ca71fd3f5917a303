"""RANSAC registration of visual-odometry records (fgo_vro_ransac_batch), batched.  One JSON line per number of hypotheses:
  batch_ms / batch_us_per_pair    wall time of ONE fgo_vro_ransac_batch call over all pairs (upload of the matches and download of
                                  the poses, informations, covariances, masks and results included), median of --reps calls after
                                  a warm-up call
  kernel_ms                       the kernel alone by HIP events, median over the same calls
  host_ms_per_pair                the numpy restatement (tests/vro_ransac_reference.py) on the host, mean over --host-pairs pairs:
                                  for scale only
Pairs: --pairs pairs of --matches matches, points of camera i in [-1.5, 1.5] x [-1, 1] x [0.8, 5] m, a planted rotation of up to
0.3 rad and translation of up to 0.2 m, 2 mm noise, --outliers of the matches displaced by 0.3 - 1 m.  --waves 1 / 4 selects the
workgroup shape (one wave per pair, or four waves that split the hypotheses); 0 is the library's default.
    python tools/vro_ransac_bench.py [--pairs 4096] [--matches 100] [--outliers 0.3] [--hypotheses 500 5000] [--reps 21] [--waves 0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graph_slam_amd as G  # noqa: E402


def _rot(w):
    th = np.linalg.norm(w, axis=1)[:, None, None]
    k = w / np.maximum(np.linalg.norm(w, axis=1, keepdims=True), 1e-300)
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pairs(n, m, share, seed=11):
    rng = np.random.default_rng(seed)
    R = _rot(rng.uniform(-1, 1, (n, 3)) * 0.3 / np.sqrt(3)); t = rng.uniform(-0.2, 0.2, (n, 1, 3))
    pi = rng.uniform([-1.5, -1.0, 0.8], [1.5, 1.0, 5.0], (n, m, 3))
    pj = np.einsum("nba,nmb->nma", R, pi - t)                     # R^T (p_i - t)
    out = rng.uniform(size=(n, m)) < share
    d = rng.normal(size=(n, m, 3)); d *= rng.uniform(0.3, 1.0, (n, m, 1)) / np.linalg.norm(d, axis=2, keepdims=True)
    pj = pj + out[..., None] * d
    xi = pi + 0.002 * rng.normal(size=pi.shape); xj = pj + 0.002 * rng.normal(size=pj.shape)
    return np.arange(n + 1, dtype=np.int64) * m, xi.reshape(-1, 3), xj.reshape(-1, 3), out.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--matches", type=int, default=100)
    ap.add_argument("--outliers", type=float, default=0.3)
    ap.add_argument("--hypotheses", type=int, nargs="+", default=[500, 5000])
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--waves", type=int, default=0, choices=(0, 1, 4))
    ap.add_argument("--host-pairs", type=int, default=3)
    a = ap.parse_args()
    ptr, xi, xj, planted_out = pairs(a.pairs, a.matches, a.outliers)
    waves = G.lib.fgo_debug_vro_waves(a.waves)
    for K in a.hypotheses:
        params = G.vro_params(hypotheses=K)
        call = lambda: G.vro_ransac_batch(ptr, xi, xj, params=params)
        out = call()                                              # warm-up: code object load, first allocations
        times, kernel = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); out = call(); times.append(1e3 * (time.perf_counter() - t0))
            kernel.append(G.lib.fgo_debug_vro_kernel_ms())
        host = None
        if a.host_pairs > 0:
            from tests import vro_ransac_reference as ref
            t0 = time.perf_counter()
            for p in range(a.host_pairs):
                ref.ransac_pair(xi[ptr[p]:ptr[p + 1]], xj[ptr[p]:ptr[p + 1]], hypotheses=K)
            host = round(1e3 * (time.perf_counter() - t0) / a.host_pairs, 2)
        batch_ms = float(np.median(times))
        ok = out["status"] == G.FGO_VRO_OK
        print(json.dumps(dict(
            pairs=a.pairs, matches=a.matches, outliers=a.outliers, hypotheses=K, waves=waves, batch_ms=round(batch_ms, 3),
            batch_us_per_pair=round(1e3 * batch_ms / a.pairs, 3), kernel_ms=round(float(np.median(kernel)), 3),
            hypothesis_match_products_per_s=round(a.pairs * K * a.matches / (1e-3 * float(np.median(kernel))), 0), host_ms_per_pair=host,
            status_ok=int(ok.sum()), mask_equals_planted=int(sum(
                np.array_equal(out["inliers"][ptr[p]:ptr[p + 1]] == 0, planted_out[ptr[p]:ptr[p + 1]]) for p in np.nonzero(ok)[0])),
            rmse_median=round(float(np.median(out["rmse"][ok])), 5) if ok.any() else None,
            batch_ms_all_reps=[round(t, 3) for t in times])), flush=True)
    G.lib.fgo_debug_vro_waves(0)


if __name__ == "__main__":
    main()
