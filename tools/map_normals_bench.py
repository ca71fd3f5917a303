"""k-nearest-neighbour surface normals of the map (fgo_map_normals).  One JSON line per cloud:
  call_ms            wall time of ONE fgo_map_normals call (upload of the cloud, the allocation, download of normals, curvatures,
                     eigenvalues, counts and status included; the neighbour lists are not asked for), median of --reps calls after a
                     warm-up call
  kernel_ms          the device work alone by HIP events (quantise, sort, gather, search and fit), median over the same calls
  points_per_s       points over kernel_ms
  host_ms_per_point  the numpy restatement (tests/map_normals_reference.py) on the host, on --rows points of the same cloud drawn at
                     random (it measures every pair, so a whole map is out of its reach): the only yardstick there is
  equals_host        on those points: the integer outputs (lists, distances, scatter, status) EQUAL, and the worst floating errors
                     in the units of the GPU test (eps l2; eps l2 / (l1 - l0)) next to its bound K
Clouds: `map` is the fused map of tools/map_fuse_bench.py's corner sweep (--frames frames of --width x --height, skip and leaf as
given), cleaned with the defaults and the camera's y as the down axis; `sheet` is a wall of --sheet points, a square grid at the
leaf's spacing with 5 mm of jitter, in shuffled order: a large map.  --k, --radius and --cell are the call's parameters.
    python tools/map_normals_bench.py [--frames 1024] [--width 176] [--height 144] [--skip 2] [--leaf 0.02] [--sheet 2000000]
                                      [--k 20] [--radius 0.16] [--cell 0.04] [--rows 256] [--reps 21]"""
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
from tests import map_normals_reference as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--width", type=int, default=176)
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--skip", type=int, default=2)
    ap.add_argument("--leaf", type=float, default=0.02)
    ap.add_argument("--sheet", type=int, default=2000000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--radius", type=float, default=0.16)
    ap.add_argument("--cell", type=float, default=0.04)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    P = dict(k=a.k, max_radius=a.radius, cell=a.cell)
    clouds = []
    if a.frames > 0:
        depth, poses, cam = trajectory(a.frames, a.width, a.height)
        fused = G.map_fuse_batch(depth, poses, params=G.map_params(skip=a.skip, leaf=a.leaf, **cam))
        clouds.append(("map", G.map_clean(fused["xyz"], params=G.map_clean_params(up_axis=1, up_sign=-1))["xyz"]))
    if a.sheet > 0:
        rng = np.random.default_rng(17)
        side = int(np.ceil(np.sqrt(a.sheet)))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:a.sheet] - side // 2
        x = np.concatenate([a.leaf * g, np.full((a.sheet, 1), 0.7)], 1) + rng.uniform(-0.005, 0.005, (a.sheet, 3))
        clouds.append(("sheet", x[rng.permutation(a.sheet)]))
    params = G.map_normals_params(**P)
    for name, x in clouds:
        rows = np.sort(np.random.default_rng(18).choice(len(x), min(a.rows, len(x)), replace=False))
        t0 = time.perf_counter()
        want = ref.normals(x, rows=rows, **P)
        host_ms = 1e3 * (time.perf_counter() - t0)
        out = G.map_normals(x, params=params, want_neighbours=True, want_scatter=True)       # warm-up, and the comparison
        same = all(np.array_equal(out[f][rows], want[f]) for f in ref.INT_ARRAYS)
        same = same and all(out[f] == want[f] for f in ("n_points", "n_out_of_range", "n_cells"))
        v = want["status"] == 0
        n, e, we = out["normal"][rows][v], out["eigenvalues"][rows][v], want["eigenvalues"][v]
        gap = (we[:, 1] - we[:, 0]) >= ref.GAP_MIN * we[:, 2]
        errors = dict(eigenvalues=float(ref.eigenvalue_error(e, we, we[:, 2]).max(initial=0)),
                      residual=float(ref.residual(want["A"][v], n, e[:, 0], we[:, 2]).max(initial=0)),
                      direction=float(ref.direction_error(n[gap], want["normal"][v][gap], we[gap]).max(initial=0)), K=ref.K)
        call = lambda: G.map_normals(x, params=params)
        times, kernel = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); out = call(); times.append(1e3 * (time.perf_counter() - t0))
            kernel.append(G.lib.fgo_debug_map_normals_kernel_ms())
        call_ms, kernel_ms = float(np.median(times)), float(np.median(kernel))
        print(json.dumps(dict(
            cloud=name, points=len(x), **P, call_ms=round(call_ms, 3), kernel_ms=round(kernel_ms, 3),
            points_per_s=float("%.4g" % (len(x) / (1e-3 * kernel_ms))), host_rows=len(rows), host_ms_per_point=round(host_ms / len(rows), 3),
            equals_host=bool(same), errors_in_eps={k: round(v, 2) for k, v in errors.items()},
            **{f: out[f] for f in ref.RESULT_FIELDS}, mean_neighbours=round(float(out["n_neighbours"].mean()), 2),
            kernel_ms_min_max=[round(min(kernel), 3), round(max(kernel), 3)], call_ms_all_reps=[round(t, 3) for t in times])), flush=True)


if __name__ == "__main__":
    main()
