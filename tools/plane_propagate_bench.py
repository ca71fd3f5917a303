"""Plane propagation between depth frames (fgo_plane_propagate_batch), batched.  One JSON line:
  batch_ms / batch_us_per_pair    wall time of ONE fgo_plane_propagate_batch call over all pairs (upload of the frames, their labels and
                                  planes and of the pairs, download of the planes, covariances and records included; the label images
                                  too with --labels), median of --reps calls after a warm-up call
  kernel_ms                       the kernel alone by HIP events, median over the same calls
  extract_kernel_ms               for scale, in the same session: the kernel of fgo_plane_extract_batch (--hypotheses) over the frame j of
                                  every pair, the step a caller without propagation runs instead
  host_ms_per_pair                the numpy restatement (tests/plane_propagate_reference.py) on the host, mean over --host-pairs pairs
Frames: --scenes distinct renders of --width x --height of a room corner (front wall, right wall and floor in view) along a path of
small steps, sigma_z = 0.014 m depth noise, 1 mm depth words, one intensity level per wall with a texture of +-2; the SR4000's
intrinsics.  Their labels and planes come from fgo_plane_extract_batch.  Pair p carries frame p % scenes into the next frame of the
path under the true relative pose and a pose covariance of 0.01 rad / 0.03 m (an IMU-only prediction).
    python tools/plane_propagate_bench.py [--pairs 4096] [--width 176] [--height 144] [--scenes 64] [--reps 5] [--labels]"""
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
from tests import plane_propagate_reference as pp  # noqa: E402


def scenes(n, W, H, seed=11):
    """n frames along a path: depth, intensity, and the poses"""
    rng = np.random.default_rng(seed)
    cam = ref.camera(W, H)
    depth, inten, poses = [], [], []
    for s in range(n):
        a = 2 * np.pi * s / n                                     # a closed path: the last frame is a small step from the first
        R = ref.rot_y(np.deg2rad(40.0 + 3 * np.sin(a))) @ ref.rot_x(np.deg2rad(-25.0 + 2 * np.cos(a)))
        t = 0.08 * np.array([np.sin(a), 0.5 * np.cos(a), np.sin(2 * a)])
        d, wall = ref.render(ref.room_planes(pp.LO, pp.HI, R, t), W, H, cam, 0.014, rng)
        depth.append(d); inten.append(pp.intensity_of(wall, rng)); poses.append((R, t))
    return np.stack(depth), np.stack(inten), poses, cam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--width", type=int, default=176)
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--hypotheses", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--labels", action="store_true")
    ap.add_argument("--host-pairs", type=int, default=2)
    a = ap.parse_args()
    ns = max(2, min(a.scenes, a.pairs))
    depth, inten, poses, cam = scenes(ns, a.width, a.height)
    X = G.plane_extract_params(**dict(cam, hypotheses=a.hypotheses, min_pixels=max(3, a.width * a.height // 17)))
    ex = G.plane_extract_batch(depth, params=X, want_labels=True)
    fi = np.arange(a.pairs) % ns; fj = (fi + 1) % ns
    pose = np.array([pp.rel_pose(*poses[i], *poses[j]) for i, j in zip(fi, fj)])
    S = np.diag([0.01 ** 2] * 3 + [0.03 ** 2] * 3)
    cov = np.tile(S, (a.pairs, 1, 1))
    params = G.plane_propagate_params(**cam)
    call = lambda: G.plane_propagate_batch(depth, inten, ex["labels"], ex["n_planes"], ex["abcd_all"], ex["cov16_all"], fi, fj, pose, cov=cov,
                                           params=params, want_labels=a.labels)
    out = call()                                                  # warm-up: code object load, first allocations
    times, kernel = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); out = call(); times.append(1e3 * (time.perf_counter() - t0))
        kernel.append(G.lib.fgo_debug_plane_propagate_kernel_ms())
    xk = []
    for _ in range(1 + min(a.reps, 3)):
        G.plane_extract_batch(depth[fj], params=X)
        xk.append(G.lib.fgo_debug_plane_extract_kernel_ms())
    host = None
    if a.host_pairs > 0:
        t0 = time.perf_counter()
        for p in range(a.host_pairs):
            k = int(ex["n_planes"][fi[p]])
            pp.propagate_pair(depth[fi[p]], ex["labels"][fi[p]], ex["abcd_all"][fi[p], :k], ex["cov16_all"][fi[p], :k].reshape(k, 16), depth[fj[p]],
                              inten[fj[p]], pose[p], S, **cam)
        host = round(1e3 * (time.perf_counter() - t0) / a.host_pairs, 2)
    batch_ms, kernel_ms = float(np.median(times)), float(np.median(kernel))
    print(json.dumps(dict(
        pairs=a.pairs, width=a.width, height=a.height, scenes=ns, labels=a.labels, batch_ms=round(batch_ms, 3),
        batch_us_per_pair=round(1e3 * batch_ms / a.pairs, 3), kernel_ms=round(kernel_ms, 3), kernel_us_per_pair=round(1e3 * kernel_ms / a.pairs, 3),
        extract_hypotheses=a.hypotheses, extract_kernel_ms=round(float(np.median(xk[1:])), 3), host_ms_per_pair=host,
        status_ok=int((out["status"] == G.FGO_PP_OK).sum()), planes_in_mean=round(float(ex["n_planes"][fi].mean()), 3),
        planes_kept_mean=round(float(out["n_planes"].mean()), 3), added_share_mean=round(float(out["num_added"].mean()) / (a.width * a.height), 4),
        search_rest_counts=[int((out["search_rest"] == k).sum()) for k in range(3)], batch_ms_all_reps=[round(t, 3) for t in times])), flush=True)


if __name__ == "__main__":
    main()
