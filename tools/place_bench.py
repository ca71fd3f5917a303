"""Place recognition by visual words (fgo_vocab_train, fgo_place_query_batch).  One JSON line per shape FRAMESxFEATURESxWORDS:
  train_ms / train_kernel_ms      wall time of ONE fgo_vocab_train call over all descriptors at --iters iterations (upload of the
                                  descriptors included), and its loop alone by HIP events (the launches and the 16-byte read of the
                                  changed-count per iteration); median of --train-reps calls after a warm-up call
  batch_ms / batch_us_per_frame   wall time of ONE fgo_place_query_batch call (upload of the descriptors and the vocabulary, download
                                  of the candidates and the host's packing of the pairs included), median of --reps calls after a
                                  warm-up call
  assign_ms, hist_ms, score_ms    the kernels alone by HIP events, median over the same calls: the norms and the assignment; the
                                  per-frame histograms; the weighting and the scoring with its top-k
  assign_distances_per_s          F x V / assign_ms; one distance is 128 int8 multiply-adds -- to be read beside the distances_per_s
                                  tools/feature_match_bench.py reports for k_match in the same session
  pair_scores_per_s               the (a, b) pairs scored / score_ms
  host_ms_per_frame               the numpy restatement (tests/place_reference.py) on the first --host-frames frames, with the
                                  device's weights; its words and norms are compared with the device's: for scale only
  revisits_found                  the share of the frames of the second lap whose first-lap frame is among their candidates
Frames: two laps over FRAMES / 2 places; a place looks at a window of 2 x FEATURES landmarks of one world, advancing FEATURES per
place, a frame sees a random half of it with descriptor noise +-8.
    python tools/place_bench.py [--shapes 4096x256x4096] [--reps 11] [--train-reps 3] [--iters 10] [--host-frames 8]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import graph_slam_amd as G  # noqa: E402


def frames(n_frames, n, seed=17):
    rng = np.random.default_rng(seed)
    places = n_frames // 2
    world = rng.integers(0, 256, (n * (places + 1), 128), dtype=np.int16)
    desc = np.empty((n_frames * n, 128), np.uint8)
    for f in range(n_frames):                                    # a frame at a time: the noise of all of them at once is large
        ids = n * (f % places) + rng.permutation(2 * n)[:n]
        desc[f * n:(f + 1) * n] = np.clip(world[ids] + rng.integers(-8, 9, (n, 128), dtype=np.int16), 0, 255)
    return np.arange(n_frames + 1, dtype=np.int64) * n, desc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x256x4096"], help="FRAMESxFEATURESxWORDS")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--train-reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--min-gap", type=int, default=10)
    ap.add_argument("--host-frames", type=int, default=8)
    a = ap.parse_args()
    for shape in a.shapes:
        n_frames, n, n_words = (int(x) for x in shape.split("x"))
        ptr, desc = frames(n_frames, n)
        vo = G.vocab_options(n_words=n_words, n_iters=a.iters)
        voc = G.vocab_train(desc, vo)                            # warm-up: code object load, first allocations
        t_train, k_train = [], []
        for _ in range(a.train_reps):
            t0 = time.perf_counter(); voc = G.vocab_train(desc, vo); t_train.append(1e3 * (time.perf_counter() - t0))
            k_train.append(G.lib.fgo_debug_place_kernel_ms())
        po = G.place_options(top_k=a.top_k, min_gap=a.min_gap)
        call = lambda: G.place_query_batch(ptr, desc, voc["centres"], options=po)
        out = call()
        times, parts = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); out = call(); times.append(1e3 * (time.perf_counter() - t0))
            p = np.zeros(3); G.lib.fgo_debug_place_phase_ms(G.ptr(p)); parts.append(p)
        host = None
        if a.host_frames > 0:
            from tests import place_reference as ref
            h = a.host_frames
            dev = G.place_query_batch(ptr[:h + 1], desc, voc["centres"], weights=out["weights"], options=G.place_options(min_gap=1), want_words=True)
            t0 = time.perf_counter()
            r = ref.query(ptr[:h + 1], desc, voc["centres"], weights=out["weights"], min_gap=1)
            host = round(1e3 * (time.perf_counter() - t0) / h, 2)
            assert np.array_equal(r["word"], dev["word"]) and np.array_equal(r["norm2"], dev["norm2"])
            assert np.array_equal(r["cand_frame"], dev["cand_frame"]) and np.array_equal(r["cand_score"], dev["cand_score"])
        assign_ms, hist_ms, score_ms = (float(x) for x in np.median(np.array(parts), axis=0))
        places = n_frames // 2
        last = np.arange(n_frames) - a.min_gap
        n_scored = int((last[last >= 0] + 1).sum())
        found = np.mean([(f - places) in out["cand_frame"][f] for f in range(places, n_frames)])
        batch_ms = float(np.median(times))
        print(json.dumps(dict(
            frames=n_frames, features=n, words=n_words, iters=a.iters, train_ms=round(float(np.median(t_train)), 3),
            train_kernel_ms=round(float(np.median(k_train)), 3), train_iterations=int(voc["iterations"]), train_converged=int(voc["converged"]),
            train_n_empty=int(voc["n_empty"]), batch_ms=round(batch_ms, 3), batch_us_per_frame=round(1e3 * batch_ms / n_frames, 3),
            assign_ms=round(assign_ms, 3), hist_ms=round(hist_ms, 3), score_ms=round(score_ms, 3),
            assign_distances_per_s=round(n_frames * n * n_words / (1e-3 * assign_ms), 0), pair_scores_per_s=round(n_scored / (1e-3 * score_ms), 0),
            host_ms_per_frame=host, pairs=int(len(out["frame_i"])), revisits_found=round(float(found), 4),
            batch_ms_all_reps=[round(t, 3) for t in times])), flush=True)


if __name__ == "__main__":
    main()
