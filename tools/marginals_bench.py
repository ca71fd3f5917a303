"""Marginal covariances of the whole map at config 2 (100k poses): one JSON line with the host time and size of the
selected inversion's pair tables, the device time of the undamped factorisation, the prep kernel and the reverse sweep (HIP
events), the per-block cost of the column-solve path (marginal_cov_many on 64 ids) and the implied speed-up for all blocks.
    python tools/marginals_bench.py [--poses 100000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graph_slam_amd as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--many", type=int, default=64)
    args = ap.parse_args()
    n = args.poses
    g = G.synth_manhattan3d(n, 5, 4, seed=args.seed)
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    gr = G.Graph()
    gr.add_poses(g["poses"], fixed)
    gr.add_edges(g["ei"], g["ej"], g["meas"], g["info"])
    gr.chi2()                                            # structure phase out of the way
    t0 = time.perf_counter()
    ids, cov = gr.marginal_cov_all()
    wall_all = time.perf_counter() - t0
    st = gr.selinv_stats()
    t0 = time.perf_counter()
    _, cov2 = gr.marginal_cov_all()                      # cached: the gather and the copy only
    wall_cached = time.perf_counter() - t0
    assert np.array_equal(cov, cov2)
    pick = np.random.default_rng(7).choice(ids, args.many, replace=False)
    t0 = time.perf_counter()
    many = gr.marginal_cov_many(pick)
    per_block = (time.perf_counter() - t0) / args.many
    pos = {int(v): k for k, v in enumerate(ids)}
    rel = max(float(np.abs(cov[pos[int(v)]] - many[k]).max() / np.abs(many[k]).max()) for k, v in enumerate(pick))
    dev_ms = st["ms_factor"] + st["ms_prep"] + st["ms_sweep"]
    print(json.dumps(dict(
        poses=n, blocks=int(len(ids)), n_levels=gr.stats().n_levels, nnz_L_blocks=int(gr.stats().nnz_L_blocks),
        list_build_s=round(st["t_lists_s"], 4), list_bytes=st["list_bytes"], list_entries=st["entries"],
        factor_ms=round(st["ms_factor"], 3), prep_ms=round(st["ms_prep"], 3), sweep_ms=round(st["ms_sweep"], 3),
        device_ms_total=round(dev_ms, 3), wall_all_s=round(wall_all, 3), wall_cached_s=round(wall_cached, 3),
        many_per_block_ms=round(1e3 * per_block, 3), many_all_blocks_est_s=round(per_block * len(ids), 1),
        speedup_vs_many=round(per_block * len(ids) / wall_all, 1), max_rel_diff_vs_many=rel)))


if __name__ == "__main__":
    main()
