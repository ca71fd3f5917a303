"""Z-buffer rendering of the map from trajectory poses (fgo_map_render_batch), batched.  One JSON line per setup, footprint, number of
views and kernel form:
  call_ms / call_us_per_view   wall time of ONE fgo_map_render_batch call over all views (upload of the cloud and, in the depth
                               setup, of the measured depth words, the allocation, download of what the setup asks for), median of
                               --reps calls after a warm-up call
  kernel_ms                    the device work alone by HIP events (all kernels of the call), median over the same calls
  projections_per_s            views x points over kernel_ms: what the global form projects; the tiles form projects every point
                               once per strip, `strips` times as many
  host_ms_per_view             the numpy restatement (tests/map_render_reference.py) on the host, over --host-views views: for scale only
The cloud is the fused map of tools/map_fuse_bench.py's corner sweep (--frames frames of --width x --height, skip and leaf as there,
with a random colour per pixel), rendered at --width x --height from --views of the sweep's poses (evenly taken).  Setups: `chase` =
through the reference's chase camera (view_offset = look_at((0, -2, -5), (0, 0, 5), (0, -0.98, 0.199))), the colour image out and
nothing else; `depth` = from the frames' own cameras with the frames' depth words given, counts only (no image comes back).  Each
with footprints of one pixel (splat 0, radius 0) and with radius = leaf.  --form names the kernel forms to time (FGO_MAP_RENDER).
    python tools/map_render_bench.py [--frames 4096] [--views 1024 4096] [--width 176] [--height 144] [--skip 2] [--leaf 0.02]
                                     [--form tiles global] [--setup chase depth] [--reps 21] [--host-views 2]"""
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
from tests import map_render_reference as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--views", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--width", type=int, default=176)
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--skip", type=int, default=2)
    ap.add_argument("--leaf", type=float, default=0.02)
    ap.add_argument("--form", nargs="+", default=["tiles", "global"], choices=("tiles", "global"))
    ap.add_argument("--setup", nargs="+", default=["chase", "depth"], choices=("chase", "depth"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host-views", type=int, default=2)
    a = ap.parse_args()
    W, H = a.width, a.height
    depth, poses, cam = trajectory(a.frames, W, H)
    frame_color = np.random.default_rng(3).integers(0, 256, depth.shape + (3,)).astype(np.uint8)
    fused = G.map_fuse_batch(depth, poses, frame_color, params=G.map_params(skip=a.skip, leaf=a.leaf, **cam))
    del frame_color
    xyz, color = fused["xyz"], fused["color"]
    chase = G.look_at(ref.CHASE_EYE, ref.CHASE_TARGET, ref.CHASE_UP)
    for n_views in a.views:
        pick = np.unique(np.linspace(0, a.frames - 1, min(n_views, a.frames)).round().astype(np.int64))
        vp, vd = np.ascontiguousarray(poses[pick]), np.ascontiguousarray(depth[pick])
        for setup, radius in [(s, r) for s in a.setup for r in (0.0, a.leaf)]:
            P = dict(cam, radius=radius)
            if setup == "chase":
                kw = dict(color=color, view_offset=chase, want_zq=False, want_color=True)
                host_kw = dict(color=color, view_offset=chase)
            else:
                kw = dict(depth=vd, want_zq=False, want_color=False)
                host_kw = dict(depth=vd[:a.host_views])
            host = None
            if a.host_views > 0:
                k = min(a.host_views, len(vp))
                t0 = time.perf_counter()
                ref.render(xyz, vp[:k], width=W, height=H, **host_kw, **P)
                host = round(1e3 * (time.perf_counter() - t0) / k, 3)
            for form in a.form:
                os.environ["FGO_MAP_RENDER"] = form
                params = G.map_render_params(**P)
                call = lambda: G.map_render_batch(xyz, vp, width=W, height=H, params=params, **kw)
                out = call()                                      # warm-up: code object load, first allocations
                times, kernel = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter(); out = call(); times.append(1e3 * (time.perf_counter() - t0))
                    kernel.append(G.lib.fgo_debug_map_render_kernel_ms())
                call_ms, kernel_ms = float(np.median(times)), float(np.median(kernel))
                strips = -(-H // out["tile_rows"]) if out["tile_rows"] else 1
                print(json.dumps(dict(
                    setup=setup, radius=radius, form=form, form_ran=out["form"], tile_rows=out["tile_rows"], strips=strips, views=len(vp),
                    points=len(xyz), width=W, height=H, call_ms=round(call_ms, 3), call_us_per_view=round(1e3 * call_ms / len(vp), 3),
                    kernel_ms=round(kernel_ms, 3), kernel_us_per_view=round(1e3 * kernel_ms / len(vp), 3),
                    projections_per_s=float("%.4g" % (len(vp) * len(xyz) / (1e-3 * kernel_ms))),
                    drawn_per_view=round(float(out["n_drawn"].mean()), 1), pixels_per_view=round(float(out["n_pixels"].mean()), 1),
                    agree_share=None if setup != "depth" else round(float(out["n_agree"].sum() / max(out["n_both"].sum(), 1)), 4),
                    host_ms_per_view=host, kernel_ms_min_max=[round(min(kernel), 3), round(max(kernel), 3)],
                    call_ms_all_reps=[round(t, 3) for t in times])), flush=True)


if __name__ == "__main__":
    main()
