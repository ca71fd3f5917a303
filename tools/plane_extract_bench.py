"""Plane extraction from depth frames (fgo_plane_extract_batch), batched.  One JSON line per number of hypotheses:
  batch_ms / batch_us_per_frame   wall time of ONE fgo_plane_extract_batch call over all frames (upload of the depth words and download
                                  of the planes, covariances and results included; the labels too with --labels), median of --reps
                                  calls after a warm-up call
  kernel_ms                       the kernel alone by HIP events, median over the same calls
  host_ms_per_frame               the numpy restatement (tests/plane_extract_reference.py) on the host, mean over --host-frames
                                  frames: for scale only
Frames: --frames frames of --width x --height, drawn from --scenes distinct renders of a room corner (front wall, right wall and
floor in view) from slightly different poses, sigma_z = 0.014 m depth noise, 1 mm depth words; the SR4000's intrinsics.
    python tools/plane_extract_bench.py [--frames 4096] [--width 176] [--height 144] [--hypotheses 128 512] [--reps 5] [--labels]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graph_slam_amd as G  # noqa: E402
from tests import plane_extract_reference as ref  # noqa: E402


def frames(n, W, H, scenes, seed=11):
    rng = np.random.default_rng(seed)
    cam = ref.camera(W, H)
    lo, hi = np.array([-40.0, -40.0, -40.0]), np.array([1.6, 1.1, 2.2])
    pool = []
    for _ in range(scenes):
        R = ref.rot_y(np.deg2rad(40.0 + rng.uniform(-4, 4))) @ ref.rot_x(np.deg2rad(-25.0 + rng.uniform(-3, 3)))
        pool.append(ref.render(ref.room_planes(lo, hi, R, rng.uniform(-0.1, 0.1, 3)), W, H, cam, 0.014, rng)[0])
    pool = np.stack(pool)
    return pool[np.arange(n) % scenes], cam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--width", type=int, default=176)
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--hypotheses", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--labels", action="store_true")
    ap.add_argument("--host-frames", type=int, default=2)
    a = ap.parse_args()
    depth, cam = frames(a.frames, a.width, a.height, min(a.scenes, a.frames))
    for K in a.hypotheses:
        P = dict(cam, hypotheses=K, min_pixels=max(3, a.width * a.height // 17))     # 1500 at 176 x 144
        params = G.plane_extract_params(**P)
        call = lambda: G.plane_extract_batch(depth, params=params, want_labels=a.labels)
        out = call()                                              # warm-up: code object load, first allocations
        times, kernel = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); out = call(); times.append(1e3 * (time.perf_counter() - t0))
            kernel.append(G.lib.fgo_debug_plane_extract_kernel_ms())
        host = None
        if a.host_frames > 0:
            t0 = time.perf_counter()
            for f in range(a.host_frames):
                ref.extract_frame(depth[f], **P)
            host = round(1e3 * (time.perf_counter() - t0) / a.host_frames, 2)
        batch_ms, kernel_ms = float(np.median(times)), float(np.median(kernel))
        print(json.dumps(dict(
            frames=a.frames, width=a.width, height=a.height, hypotheses=K, labels=a.labels, batch_ms=round(batch_ms, 3),
            batch_us_per_frame=round(1e3 * batch_ms / a.frames, 3), kernel_ms=round(kernel_ms, 3),
            kernel_us_per_frame=round(1e3 * kernel_ms / a.frames, 3), host_ms_per_frame=host,
            status_ok=int((out["status"] == G.FGO_PX_OK).sum()), planes_mean=round(float(out["n_planes"].mean()), 3),
            rounds_mean=round(float(out["rounds_run"].mean()), 3),
            rmse_median=round(float(np.median(out["rmse"][out["n_pixels"] > 0])), 5) if (out["n_pixels"] > 0).any() else None,
            batch_ms_all_reps=[round(t, 3) for t in times])), flush=True)


if __name__ == "__main__":
    main()
