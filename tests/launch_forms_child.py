"""Child runner of tests/test_gpu_launch_forms.py: FGO_TUNE and several selection constants are read once per process, so every
override set runs in a fresh process -- this script.  It builds a fixed list of small graphs and prints one JSON record per graph:
the launch census (fused and stand-alone), status, and the path of an .npz holding delta from fgo_solve_step, delta from
fgo_debug_solve_fused, b and (with --dense) the dense H of linearize(dense=True), stored as its non-zero entries.  It computes no
reference: the parent does.

usage: launch_forms_child.py --out DIR [--dense] [--graphs a,b,...]"""
import argparse
import json
import os
import resource
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import graph_slam_amd as G  # noqa: E402
from tests.util import pose_mul, pose_inv, noisy, random_info, info_ut  # noqa: E402


def synth(n, lookback, n_loop, seed):
    g = G.synth_manhattan3d(n, lookback, n_loop, seed)
    g["fixed"] = np.zeros(n, np.uint8); g["fixed"][0] = 1
    return g


def random_truth(rng, n, spread=3.0):
    out = []
    for _ in range(n):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        ang = rng.uniform(-1.0, 1.0)
        out.append(np.concatenate([rng.normal(size=3) * spread, ax * np.sin(ang / 2), [np.cos(ang / 2)]]))
    return np.array(out)


def from_pairs(rng, truth, pairs, fixed, noise=0.02, init_noise=0.05):
    meas, info = [], []
    for a, b in pairs:
        meas.append(noisy(rng, pose_mul(pose_inv(truth[a]), truth[b]), noise, noise * 0.5))
        info.append(info_ut(random_info(rng)))
    init = np.array([noisy(rng, t, init_noise, init_noise * 0.3) for t in truth])
    fx = np.zeros(len(truth), np.uint8)
    fx[list(fixed)] = 1
    init[list(fixed)] = np.asarray(truth)[list(fixed)]
    return dict(poses=init, fixed=fx, ei=np.array([p[0] for p in pairs], np.int32), ej=np.array([p[1] for p in pairs], np.int32),
                meas=np.array(meas), info=np.array(info))


def star(n):
    """tests/test_gpu_edgecases.py::test_star_hub"""
    rng = np.random.default_rng(3)
    truth = random_truth(rng, n)
    return from_pairs(rng, truth, [(0, k) for k in range(1, n)] + [(k, k + 1) for k in range(1, n - 1, 3)], fixed=[1])


def complete(n):
    """tests/test_gpu_edgecases.py::test_complete_graph_is_one_dense_hierarchy"""
    rng = np.random.default_rng(7)
    truth = random_truth(rng, n, spread=1.0)
    return from_pairs(rng, truth, [(a, b) for a in range(n) for b in range(a + 1, n)], fixed=[0])


_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return dict(_memo[key])


def negated(g):
    g["info"] = -np.asarray(g["info"])
    return g


def negdef():
    """tests/test_gpu_panels.py::test_not_positive_definite_is_reported"""
    return negated(synth(200, 3, 1, seed=5))


# name -> (graph, environment of the context, kind)
GRAPHS = [
    ("synth150_w1", lambda: synth(150, 5, 4, 250), {"FGO_TASK_WORK": "1"}, "solve"),
    ("synth400_w1", lambda: synth(400, 5, 4, 500), {"FGO_TASK_WORK": "1"}, "solve"),
    ("synth400_w200", lambda: synth(400, 5, 4, 500), {"FGO_TASK_WORK": "200"}, "solve"),
    ("synth650_w50", lambda: synth(650, 5, 4, 750), {"FGO_TASK_WORK": "50"}, "solve"),
    ("synth200_leaf", lambda: synth(200, 3, 1, 5), {}, "solve"),      # default task work: level 0 is a leaf level
    ("star200", lambda: memo("star200", lambda: star(200)), {}, "solve"),
    ("star3000", lambda: memo("star3000", lambda: star(3000)), {}, "solve"),
    ("complete70", lambda: memo("complete70", lambda: complete(70)), {}, "solve"),
    # with chain_work=0 (sets w1_2 / w1_3) every column is a task of its own: single-column tasks 69 .. 1 blocks high, beyond what the
    # one-wave k_chol_fact forms keep in registers (20 / 30 blocks: their overflow passes); otherwise chains of 16 columns
    ("complete70_w1_nopanels", lambda: memo("complete70", lambda: complete(70)), {"FGO_TASK_WORK": "1", "FGO_NO_PANELS": "1"}, "solve"),
    ("complete130_nopanels", lambda: memo("complete130", lambda: complete(130)), {"FGO_NO_PANELS": "1"}, "solve"),
    ("complete250_nopanels", lambda: complete(250), {"FGO_NO_PANELS": "1"}, "solve"),
    ("synth150_w1_nopanels", lambda: synth(150, 5, 4, 250), {"FGO_TASK_WORK": "1", "FGO_NO_PANELS": "1"}, "solve"),
    ("negdef_w1", negdef, {"FGO_TASK_WORK": "1"}, "negdef"),
    ("negdef_default", negdef, {}, "negdef"),
    ("negdef_nopanels", negdef, {"FGO_NO_PANELS": "1"}, "negdef"),
    ("negdef_star200", lambda: negated(memo("star200", lambda: star(200))), {}, "negdef"),       # single-column tasks at level 0
    ("negdef_star3000", lambda: negated(memo("star3000", lambda: star(3000))), {}, "negdef"),
    # 129 free poses in one chain of 16-column tasks leave a single-column task: the one-wave k_chol_fact forms
    ("negdef_complete70_w1_nopanels", lambda: negated(memo("complete70", lambda: complete(70))),
     {"FGO_TASK_WORK": "1", "FGO_NO_PANELS": "1"}, "negdef"),
    ("negdef_synth25", lambda: negated(synth(25, 3, 1, 5)), {}, "negdef"),      # one light sub-tree: a leaf level and nothing else
    ("negdef_complete130_nopanels", lambda: negated(memo("complete130", lambda: complete(130))), {"FGO_NO_PANELS": "1"}, "negdef"),
]
CTX_ENV = ("FGO_TASK_WORK", "FGO_NO_PANELS")


def make_gpu(g):
    gr = G.Graph()
    gr.add_poses(g["poses"], g["fixed"])
    gr.add_edges(g["ei"], g["ej"], g["meas"], g["info"])
    return gr


def run_graph(name, make, env, kind, out_dir, dense):
    t0 = time.time()
    for k in CTX_ENV:
        os.environ.pop(k, None)
    os.environ.update(env)
    gr = make_gpu(make())
    rec = dict(graph=name, kind=kind, status="ok")
    if kind == "negdef":
        for key, fn in (("raised_step", gr.solve_step), ("raised_fused", gr.solve_fused)):
            try:
                fn(0.0)
                rec[key] = False
            except G.FgoError as e:
                rec[key] = "not positive definite" in str(e)
                rec[key + "_message"] = str(e)
        rec["census_plain"] = gr.launch_census(fused=False)
        rec["census_fused"] = gr.launch_census(fused=True)
        rec["seconds"] = time.time() - t0
        return rec
    arrays = {}
    if dense:
        chi, H, b = gr.linearize(dense=True)
        i, j = np.nonzero(H)                                          # (row-major order; the parent rebuilds the dense matrix)
        arrays["H_i"] = i.astype(np.int32); arrays["H_j"] = j.astype(np.int32); arrays["H_v"] = H[i, j]
        arrays["b_dense"] = b
        del H
    Hblk, b_perm, chi = gr.read_system()
    nb = int(gr.stats().n_free)
    diag = Hblk[:36 * nb].reshape(nb, 6, 6)
    lam = 1e-5 * float(np.abs(np.einsum("kii->ki", diag)).max())     # 1e-5 * max |diag H|: the diagonal blocks come first
    rec["lam"] = lam
    rec["chi2"] = chi
    arrays["b_sorted"] = np.sort(b_perm)                              # (elimination order: compared as a multiset)
    rec["census_plain"] = gr.launch_census(fused=False)
    rec["census_fused"] = gr.launch_census(fused=True)
    arrays["d_step"] = gr.solve_step(lam)
    arrays["d_fused"] = gr.solve_fused(lam)
    path = os.path.join(out_dir, name + ".npz")
    np.savez(path, **arrays)
    rec["npz"] = path
    rec["n_levels"] = int(gr.stats().n_levels)
    rec["seconds"] = time.time() - t0
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--graphs", default="")
    a = ap.parse_args()
    want = [s for s in a.graphs.split(",") if s]
    os.makedirs(a.out, exist_ok=True)
    for name, make, env, kind in GRAPHS:
        if want and name not in want:
            continue
        try:
            rec = run_graph(name, make, env, kind, a.out, a.dense)
        except Exception as e:      # a refusal or a HIP error: reported, the parent fails the case
            rec = dict(graph=name, kind=kind, status="error: %s: %s" % (type(e).__name__, e))
        rec["maxrss_mb"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
        print("RECORD " + json.dumps(rec), flush=True)
        if rec["status"] != "ok" and "HIP" in rec["status"]:
            return 3                 # after a device error nothing more runs in this process
    return 0


if __name__ == "__main__":
    sys.exit(main())
