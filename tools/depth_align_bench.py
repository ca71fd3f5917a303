"""Dense depth alignment of key-frame pairs (fgo_depth_align_batch), batched.  One JSON line:
  batch_ms / batch_us_per_pair    wall time of ONE fgo_depth_align_batch call over all pairs (upload of the depth words, download of the
                                  poses, informations and covariances included), median of --reps calls after a warm-up call
  kernel_ms_lds / kernel_ms_global  the device work alone by HIP events, per kernel form (fgo_debug_depth_align_form), median over
                                  the same number of calls; the two forms are checked to return the same bits
  evals_per_pair                  evaluations a pair made (its iterations + 1), mean
  plane_extract_kernel_ms         the plane-extraction kernel (fgo_plane_extract_batch, 128 hypotheses) on the target frames of the
                                  same pairs in the same session: a same-hardware yardstick, nothing the alignment is gated on
  host_ms_per_pair                the numpy restatement (tests/depth_align_reference.py) on the host, over --host-pairs pairs: for scale
Frames: tools/map_fuse_bench.py's corner sweep (front wall, right wall and floor in view, sigma_z = 0.014 m depth noise, 1 mm words,
the SR4000's intrinsics), --pairs + --gap frames of --width x --height; pair p aligns frame p + gap to frame p from the identity.
With 4096 pairs and the gap 256 a pair is 1 degree of yaw and 2.5 cm apart.
    python tools/depth_align_bench.py [--pairs 4096] [--gap 256] [--width 176] [--height 144] [--reps 5] [--host-pairs 4]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import graph_slam_amd as G  # noqa: E402
from graph_slam_amd import dense as D  # noqa: E402
from map_fuse_bench import trajectory  # noqa: E402
from tests import depth_align_reference as ref  # noqa: E402


def timed(call, reps, kernel_ms):
    call()                                                        # warm-up: code object load, first allocations
    times, kernel = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); out = call(); times.append(1e3 * (time.perf_counter() - t0))
        kernel.append(kernel_ms())
    return out, times, kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--gap", type=int, default=256)
    ap.add_argument("--width", type=int, default=176)
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=4)
    a = ap.parse_args()
    depth, _, cam = trajectory(a.pairs + a.gap, a.width, a.height)
    fi = np.arange(a.pairs); fj = fi + a.gap
    P = dict(cam)
    params = D.depth_align_params(**P)
    host = None
    if a.host_pairs > 0:
        k = min(a.host_pairs, a.pairs)
        t0 = time.perf_counter()
        for p in range(k):
            ref.align(depth[fi[p]], depth[fj[p]], None, ref.default_params(**P))
        host = round(1e3 * (time.perf_counter() - t0) / k, 2)
    runs = {}
    for name, form in (("lds", 1), ("global", 2)):
        assert G.lib.fgo_debug_depth_align_form(form) == form
        runs[name] = timed(lambda: D.depth_align_batch(depth, fi, fj, None, params), a.reps, G.lib.fgo_debug_depth_align_kernel_ms)
    G.lib.fgo_debug_depth_align_form(0)
    out, times, k_lds = runs["lds"]
    k_glb = runs["global"][2]
    same = all(np.array_equal(out[k], runs["global"][0][k]) for k in out)
    xp = G.plane_extract_params(hypotheses=128, min_pixels=max(3, a.width * a.height // 17), **P)
    _, _, k_px = timed(lambda: G.plane_extract_batch(depth[:a.pairs], params=xp), a.reps, G.lib.fgo_debug_plane_extract_kernel_ms)
    ok = out["status"] == D.FGO_DA_OK
    evals = out["iterations"] + ok
    batch_ms, kl, kg = float(np.median(times)), float(np.median(k_lds)), float(np.median(k_glb))
    print(json.dumps(dict(
        pairs=a.pairs, gap=a.gap, width=a.width, height=a.height, batch_ms=round(batch_ms, 3), batch_us_per_pair=round(1e3 * batch_ms / a.pairs, 3),
        kernel_ms_lds=round(kl, 3), kernel_ms_global=round(kg, 3), kernel_us_per_pair_lds=round(1e3 * kl / a.pairs, 3),
        forms_same_bits=bool(same), status_ok=int(ok.sum()), converged=int(out["converged"].sum()),
        iterations_mean=round(float(out["iterations"].mean()), 2), evals_per_pair=round(float(evals.mean()), 2),
        n_pairs_used_median=int(np.median(out["n_pairs_used"])), rmse_median=round(float(np.median(out["rmse"][ok])), 5) if ok.any() else None,
        plane_extract_kernel_ms=round(float(np.median(k_px)), 3), host_ms_per_pair=host,
        kernel_ms_lds_min_max=[round(min(k_lds), 3), round(max(k_lds), 3)], kernel_ms_global_min_max=[round(min(k_glb), 3), round(max(k_glb), 3)],
        batch_ms_all_reps=[round(t, 3) for t in times])), flush=True)


if __name__ == "__main__":
    main()
