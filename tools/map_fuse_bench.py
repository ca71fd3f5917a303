"""Voxel-grid map fusion of depth frames (fgo_map_fuse_batch), batched.  One JSON line per insert form and table size:
  batch_ms / batch_us_per_frame   wall time of ONE fgo_map_fuse_batch call over all frames (upload of the depth words, the table's
                                  allocation, download of the voxels included), median of --reps calls after a warm-up call
  kernel_ms                       the device work alone by HIP events (table init, insert, pack; sort, finalise), median over the same calls
  points_per_s                    valid points over kernel_ms
  depth_read_share                the depth bytes the insert kernel reads (2 per sampled pixel) per second of kernel_ms, over 8 TB/s
  host_ms_per_frame               the numpy restatement (tests/map_fuse_reference.py) on the host, over --host-frames frames: for scale only
Frames: --frames frames of --width x --height along a trajectory through a room corner (front wall, right wall and floor in view: the
scene tools/plane_extract_bench.py renders), the camera sweeping 16 degrees of yaw and 0.4 m sideways, sigma_z = 0.014 m depth noise,
1 mm depth words; the SR4000's intrinsics.  --insert names the insert forms to time (FGO_MAP_INSERT): lds = a run of 512 sampled pixels of one
frame pre-aggregated in LDS, frames = a run of 4 pixels of 128 consecutive frames pre-aggregated in LDS (the default of the library), plain = every point straight to the device-wide table.  --table-log2: the table sizes to time; a caller who knows the map is
small sets one, and the table's initialisation and the pack's sweep over it shrink with it.
    python tools/map_fuse_bench.py [--frames 4096] [--width 176] [--height 144] [--skip 2] [--leaf 0.02] [--insert lds frames plain] [--table-log2 0 17]
                                   [--shuffle] [--reps 21]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graph_slam_amd as G  # noqa: E402
from tests import map_fuse_reference as ref  # noqa: E402


def trajectory(n, W, H, seed=11):
    """depth (n x H x W), poses (n x 7) and the camera: a sweep through the corner, a little jitter on every pose"""
    rng = np.random.default_rng(seed)
    cam = ref.px.camera(W, H)
    s = np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1)
    poses = np.zeros((n, 7)); depth = np.zeros((n, H, W), np.uint16)
    for f in range(n):
        q = ref.quat_mul(ref.quat_axis(1, np.deg2rad(40.0 + 8.0 * s[f])), ref.quat_axis(0, np.deg2rad(-25.0 + rng.uniform(-1, 1))))
        poses[f] = np.concatenate([[0.2 * s[f], 0.02 * rng.uniform(-1, 1), 0.1 * s[f]], q])
        depth[f] = ref.render_frame(poses[f], W, H, cam, ref.SIGMA_Z, rng)[0]
    return depth, poses, cam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--width", type=int, default=176)
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--skip", type=int, default=2)
    ap.add_argument("--leaf", type=float, default=0.02)
    ap.add_argument("--channels", type=int, default=0, choices=(0, 1, 3))
    ap.add_argument("--insert", nargs="+", default=["lds", "frames", "plain"], choices=("lds", "frames", "plain"))
    ap.add_argument("--table-log2", type=int, nargs="+", default=[0], help="0 = automatic: the smallest 2^T >= 2 n_sampled")
    ap.add_argument("--shuffle", action="store_true", help="the frames in random order: the same map, no neighbours in a tile's frames")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host-frames", type=int, default=16)
    a = ap.parse_args()
    depth, poses, cam = trajectory(a.frames, a.width, a.height)
    if a.shuffle:
        order = np.random.default_rng(5).permutation(a.frames)
        depth, poses = np.ascontiguousarray(depth[order]), np.ascontiguousarray(poses[order])
    color = None
    if a.channels:
        shape = depth.shape if a.channels == 1 else depth.shape + (3,)
        color = np.random.default_rng(3).integers(0, 256, shape).astype(np.uint8)
    P = dict(cam, skip=a.skip, leaf=a.leaf)
    host = None
    if a.host_frames > 0:
        k = min(a.host_frames, a.frames)
        t0 = time.perf_counter()
        ref.fuse(depth[:k], poses[:k], None if color is None else color[:k], **P)
        host = round(1e3 * (time.perf_counter() - t0) / k, 3)
    for form, T in [(form, T) for T in a.table_log2 for form in a.insert]:
        os.environ["FGO_MAP_INSERT"] = form
        params = G.map_params(table_log2=T, **P)
        call = lambda: G.map_fuse_batch(depth, poses, color, params=params)
        out = call()                                              # warm-up: code object load, first allocations
        times, kernel = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); out = call(); times.append(1e3 * (time.perf_counter() - t0))
            kernel.append(G.lib.fgo_debug_map_fuse_kernel_ms())
        batch_ms, kernel_ms = float(np.median(times)), float(np.median(kernel))
        print(json.dumps(dict(
            insert=form, shuffled=a.shuffle, frames=a.frames, width=a.width, height=a.height, skip=a.skip, leaf=a.leaf, channels=a.channels,
            batch_ms=round(batch_ms, 3), batch_us_per_frame=round(1e3 * batch_ms / a.frames, 3), kernel_ms=round(kernel_ms, 3),
            kernel_us_per_frame=round(1e3 * kernel_ms / a.frames, 3), points_per_s=float("%.4g" % (out["n_valid"] / (1e-3 * kernel_ms))),
            depth_read_share=float("%.3g" % (2.0 * out["n_sampled"] / (1e-3 * kernel_ms) / 8e12)), status=out["status"],
            table_log2=out["table_log2"], n_sampled=out["n_sampled"], n_valid=out["n_valid"], voxels=out["n_voxels"],
            points_per_voxel=round(out["n_valid"] / max(out["n_voxels"], 1), 2), host_ms_per_frame=host,
            kernel_ms_min_max=[round(min(kernel), 3), round(max(kernel), 3)], batch_ms_all_reps=[round(t, 3) for t in times])), flush=True)


if __name__ == "__main__":
    main()
