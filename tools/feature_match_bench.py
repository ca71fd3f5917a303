"""Descriptor matching of key-frame pairs (fgo_match_features_batch), batched.  One JSON line per shape:
  batch_ms / batch_us_per_pair    wall time of ONE fgo_match_features_batch call over all pairs (upload of the frames, download of
                                  the per-query arrays and the host's packing of the matches included), median of --reps calls
                                  after a warm-up call
  kernel_ms                       the two launches alone (norms, match) by HIP events, median over the same calls
  distances_per_s                 pairs x N_j x N_i / kernel time; one distance is 128 int8 multiply-adds
  i8_mfma_peak_share              distances_per_s x 256 operations over the dense int8 MFMA peak (--peak-tops, 5000: twice the
                                  2.5 PFLOP/s of bf16)
  host_ms_per_pair                the numpy restatement (tests/feature_match_reference.py) on the host, mean over --host-pairs
                                  pairs: for scale only
Frames: pairs + 1 key-frames of --features features each over one static scene of 2 x features points (a frame sees a random half
of them, descriptor noise +-8, 2 mm on the points); pair p matches frame p + 1 against frame p.  --guided gates every pair under
the identity pose.
    python tools/feature_match_bench.py [--shapes 4096x256 512x2048] [--reps 21] [--guided] [--host-pairs 1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graph_slam_amd as G  # noqa: E402


def frames(n_frames, n, seed=13):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (2 * n, 128), dtype=np.int16)
    pts = rng.uniform([-1.5, -1.0, 2.0], [1.5, 1.0, 5.0], (2 * n, 3))
    ids = np.argsort(rng.random((n_frames, 2 * n)), axis=1)[:, :n]
    desc = np.empty((n_frames * n, 128), np.uint8)
    for f in range(n_frames):                                    # a frame at a time: the noise of all of them at once is large
        desc[f * n:(f + 1) * n] = np.clip(base[ids[f]] + rng.integers(-8, 9, (n, 128), dtype=np.int16), 0, 255)
    xyz = pts[ids.reshape(-1)] + 0.002 * rng.normal(size=(n_frames * n, 3))
    uv = np.stack([250.5773 * xyz[:, 0] / xyz[:, 2] + 90.0, 250.5773 * xyz[:, 1] / xyz[:, 2] + 70.0], 1)
    return np.arange(n_frames + 1, dtype=np.int64) * n, desc, xyz, uv, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x256", "512x2048"], help="PAIRSxFEATURES")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--guided", action="store_true")
    ap.add_argument("--host-pairs", type=int, default=1)
    ap.add_argument("--peak-tops", type=float, default=5000.0)
    a = ap.parse_args()
    for shape in a.shapes:
        n_pairs, n = (int(x) for x in shape.split("x"))
        ptr, desc, xyz, uv, ids = frames(n_pairs + 1, n)
        fi = np.arange(n_pairs, dtype=np.int64); fj = fi + 1
        pose = np.tile([0, 0, 0, 0, 0, 0, 1.0], (n_pairs, 1)) if a.guided else None
        call = lambda: G.match_features_batch(ptr, desc, xyz, uv, fi, fj, pose_ij=pose)
        out = call()                                              # warm-up: code object load, first allocations
        times, kernel = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); out = call(); times.append(1e3 * (time.perf_counter() - t0))
            kernel.append(G.lib.fgo_debug_match_kernel_ms())
        host = None
        if a.host_pairs > 0:
            from tests import feature_match_reference as ref
            fr = lambda f: dict(desc=desc[ptr[f]:ptr[f + 1]], xyz=xyz[ptr[f]:ptr[f + 1]], uv=uv[ptr[f]:ptr[f + 1]])
            t0 = time.perf_counter()
            for p in range(a.host_pairs):
                r = ref.match_pair(fr(p + 1), fr(p), None if pose is None else pose[p])
                assert np.array_equal(r["best"], out["best"][out["q_ptr"][p]:out["q_ptr"][p + 1]]) and r["n_matches"] == out["n_matches"][p]
            host = round(1e3 * (time.perf_counter() - t0) / a.host_pairs, 2)
        batch_ms, k_ms = float(np.median(times)), float(np.median(kernel))
        rate = n_pairs * n * n / (1e-3 * k_ms)
        right = ids.reshape(-1)[out["idx_i"]] == ids.reshape(-1)[out["idx_j"]]
        print(json.dumps(dict(
            pairs=n_pairs, features=n, guided=bool(a.guided), batch_ms=round(batch_ms, 3), batch_us_per_pair=round(1e3 * batch_ms / n_pairs, 3),
            kernel_ms=round(k_ms, 3), distances_per_s=round(rate, 0), i8_mfma_peak_share=round(rate * 256 / (a.peak_tops * 1e12), 4),
            host_ms_per_pair=host, matches_per_pair=round(float(out["n_matches"].mean()), 1), matches_right=round(float(right.mean()), 4),
            batch_ms_all_reps=[round(t, 3) for t in times])), flush=True)


if __name__ == "__main__":
    main()
