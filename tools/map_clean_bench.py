"""Cluster filtering and floor removal of the fused map (fgo_map_clean).  One JSON line per cloud:
  call_ms         wall time of ONE fgo_map_clean call (upload of the cloud, the allocation, download of labels, reasons and the kept
                  rows included), median of --reps calls after a warm-up call
  kernel_ms       the device work alone by HIP events (quantise, sort, cells, link, flatten, number, floor, compact), median over the
                  same calls
  points_per_s    points over kernel_ms
  host_ms         the numpy restatement (tests/map_clean_reference.py) on the host, on the same cloud: the only yardstick there is
Clouds: `map` is the fused map of tools/map_fuse_bench.py's corner sweep (--frames frames of --width x --height, skip and leaf as
given), cleaned with the defaults and the camera's y as the down axis; `chain` is the worst case of the union-find, --chain points
spaced exactly one tolerance apart along (1, 2, 2) in shuffled order: one cluster, one point per lane to hook, the deepest trees;
`sheet` is a wall of --sheet points, a square grid at the leaf's spacing with 5 mm of jitter, in shuffled order: a large map.
    python tools/map_clean_bench.py [--frames 1024] [--width 176] [--height 144] [--skip 2] [--leaf 0.02] [--chain 1000000] [--sheet 2000000]
                                    [--reps 21]"""
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
from map_fuse_bench import trajectory  # noqa: E402
from tests import map_clean_reference as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--width", type=int, default=176)
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--skip", type=int, default=2)
    ap.add_argument("--leaf", type=float, default=0.02)
    ap.add_argument("--chain", type=int, default=1000000)
    ap.add_argument("--sheet", type=int, default=2000000)
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    clouds = []
    if a.frames > 0:
        depth, poses, cam = trajectory(a.frames, a.width, a.height)
        fused = G.map_fuse_batch(depth, poses, params=G.map_params(skip=a.skip, leaf=a.leaf, **cam))
        clouds.append(("map", fused["xyz"], dict(up_axis=1, up_sign=-1)))
    if a.chain > 0:
        x, P = ref.chain(a.chain)
        clouds.append(("chain", x, P))
    if a.sheet > 0:
        rng = np.random.default_rng(17)
        side = int(np.ceil(np.sqrt(a.sheet)))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:a.sheet] - side // 2
        x = np.concatenate([a.leaf * g, np.full((a.sheet, 1), 0.7)], 1) + rng.uniform(-0.005, 0.005, (a.sheet, 3))
        clouds.append(("sheet", x[rng.permutation(a.sheet)], dict(remove_floor=0)))
    for name, x, P in clouds:
        t0 = time.perf_counter()
        want = ref.clean(x, **P)
        host_ms = 1e3 * (time.perf_counter() - t0)
        params = G.map_clean_params(**P)
        call = lambda: G.map_clean(x, params=params)
        out = call()                                          # warm-up: code object load, first allocations
        same = all(out[f] == want[f] for f in ref.RESULT_FIELDS) and all(np.array_equal(out[f], want[f]) for f in ref.ARRAYS)
        times, kernel = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); out = call(); times.append(1e3 * (time.perf_counter() - t0))
            kernel.append(G.lib.fgo_debug_map_clean_kernel_ms())
        call_ms, kernel_ms = float(np.median(times)), float(np.median(kernel))
        print(json.dumps(dict(
            cloud=name, points=len(x), call_ms=round(call_ms, 3), kernel_ms=round(kernel_ms, 3),
            points_per_s=float("%.4g" % (len(x) / (1e-3 * kernel_ms))), host_ms=round(host_ms, 1), equals_host=bool(same),
            **{f: out[f] for f in ref.RESULT_FIELDS}, largest_cluster=int(out["cluster_size"].max(initial=0)),
            kernel_ms_min_max=[round(min(kernel), 3), round(max(kernel), 3)], call_ms_all_reps=[round(t, 3) for t in times])), flush=True)


if __name__ == "__main__":
    main()
