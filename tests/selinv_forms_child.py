"""Child runner of tests/test_gpu_selinv_forms.py: FGO_TUNE is read once per process, so each of the three sets (the launch
selection of the selected inversion's sweep left alone, forced to the 4-wave form, forced to the 16-wave form) runs in a fresh
process -- this script, by the protocol of tests/launch_forms_child.py.  Per graph it prints one JSON record and writes one .npz:
the census (fgo_debug_selinv_census), ids and cov of marginal_cov_all, per pairs call the requested ids (pa<k>, pb<k>), the output
of marginal_cov_pairs (pc<k>) and the fallback count behind it, and (with --dense) the dense H of linearize(dense=True) of the g2o
graphs, stored as its non-zero entries.  It computes no reference: the parent does.

usage: selinv_forms_child.py --out DIR [--dense] [--graphs a,b,...]"""
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
from graph_slam_amd import scenarios  # noqa: E402
from tests.launch_forms_child import synth, star, complete, from_pairs, random_truth, make_gpu, memo, CTX_ENV  # noqa: E402

N_HUBS, N_LEAVES = 42, 273
BA_SHAPE = (40, 600)


def chain(n):
    """a path 0 - 1 - ... - n-1 with vertex 0 fixed: n - 1 block columns, the last one without off-diagonal blocks.  (spread 0.3: at
    the default 3.0 the 85-pose chain's inverse is only good to 5e-10, tests/test_selinv_forms_reference_cpu.py)"""
    rng = np.random.default_rng(11)
    truth = random_truth(rng, n, spread=0.3)
    return from_pairs(rng, truth, [(k, k + 1) for k in range(n - 1)], fixed=[0])


def hub_leaves(n_hubs=N_HUBS, n_leaves=N_LEAVES):
    """n_hubs hubs forming a clique, n_leaves leaves each tied to every hub, the LAST leaf fixed: every free leaf is a column with
    n_hubs off-diagonal blocks and no other leaf in its pattern"""
    rng = np.random.default_rng(13)
    n = n_hubs + n_leaves
    truth = random_truth(rng, n, spread=1.0)
    pairs = [(a, b) for a in range(n_hubs) for b in range(a + 1, n_hubs)] + [(h, k) for k in range(n_hubs, n) for h in range(n_hubs)]
    return from_pairs(rng, truth, pairs, fixed=[n - 1])


# name -> (graph, environment of the context, pairs beyond the factors' endpoints: "all" / "random")
G2O_GRAPHS = [
    ("chain2", lambda: chain(2), {}, "all"),
    ("chain43", lambda: chain(43), {}, "all"),
    ("chain44", lambda: chain(44), {}, "all"),
    ("chain86", lambda: chain(86), {}, "all"),
    ("complete70", lambda: memo("complete70", lambda: complete(70)), {}, "all"),
    ("complete200", lambda: memo("complete200", lambda: complete(200)), {}, "all"),
    ("complete200_w1_nopanels", lambda: memo("complete200", lambda: complete(200)), {"FGO_TASK_WORK": "1", "FGO_NO_PANELS": "1"}, "all"),
    ("star600", lambda: star(600), {}, "random"),
    ("hub42x273", hub_leaves, {}, "random"),
    ("synth200_leaf", lambda: synth(200, 3, 1, 5), {}, "random"),
    ("synth400_w1", lambda: synth(400, 5, 4, 500), {"FGO_TASK_WORK": "1"}, "random"),
    ("synth650_w50", lambda: synth(650, 5, 4, 750), {"FGO_TASK_WORK": "50"}, "random"),
]
BA_GRAPH = "ba40x600"
GRAPH_NAMES = [g[0] for g in G2O_GRAPHS] + [BA_GRAPH]


def factor_pairs(ei, ej, free):
    """every factor's endpoints, both orders (each unordered pair once; fixed endpoints dropped)"""
    und = sorted({(min(int(i), int(j)), max(int(i), int(j))) for i, j in zip(ei, ej) if int(i) in free and int(j) in free and int(i) != int(j)})
    a = np.array([p[0] for p in und] + [p[1] for p in und], np.int64)
    b = np.array([p[1] for p in und] + [p[0] for p in und], np.int64)
    return a, b


def random_pairs(seed, cand, ei, ej, n=40):
    """n seeded pairs of distinct variables of cand that share no factor, the b's drawn from eight variables so that several pairs
    share one (the column solves of the fallback are grouped by b); then (a, a) of every variable that occurs"""
    rng = np.random.default_rng(seed)
    adj = {(int(i), int(j)) for i, j in zip(ei, ej)} | {(int(j), int(i)) for i, j in zip(ei, ej)}
    cand = np.asarray(cand, np.int64)
    bs = rng.choice(cand, 8, replace=False)
    out = []
    while len(out) < n:
        a, b = int(rng.choice(cand)), int(rng.choice(bs))
        if a != b and (a, b) not in adj and (a, b) not in out:
            out.append((a, b))
    used = sorted({v for p in out for v in p})
    return (np.array([p[0] for p in out] + used, np.int64), np.array([p[1] for p in out] + used, np.int64))


def pair_calls(name, mode, free_ids, ei, ej, random_from):
    fa, fb = factor_pairs(ei, ej, set(int(v) for v in free_ids))
    calls = [(fa, fb)]
    if mode == "all":
        a, b = np.meshgrid(free_ids, free_ids, indexing="ij")
        calls.append((a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64)))
    else:
        calls.append(random_pairs(1000 + GRAPH_NAMES.index(name), random_from, ei, ej))
    return calls


def run_graph(name, gr, mode, free_ids, ei, ej, random_from, out_dir, dense):
    t0 = time.time()
    rec = dict(graph=name, status="ok")
    arrays = {}
    if dense:
        chi, H, b = gr.linearize(dense=True)
        i, j = np.nonzero(H)                                          # (row-major order; the parent rebuilds the dense matrix)
        arrays["H_i"] = i.astype(np.int32); arrays["H_j"] = j.astype(np.int32); arrays["H_v"] = H[i, j]
        arrays["H_n"] = np.array([H.shape[0]], np.int64)
        del H
    ids, cov = gr.marginal_cov_all()
    arrays["ids"] = ids; arrays["cov"] = cov
    rec["census"] = gr.selinv_census()
    rec["fallback"] = []
    for k, (a, b) in enumerate(pair_calls(name, mode, free_ids, ei, ej, random_from)):
        arrays["pa%d" % k] = a; arrays["pb%d" % k] = b
        arrays["pc%d" % k] = gr.marginal_cov_pairs(a, b) if len(a) else np.zeros((0, 6, 6))
        rec["fallback"].append(int(gr.selinv_stats()["fallback_pairs"]) if len(a) else 0)
    st = gr.selinv_stats()
    rec["ms_prep"], rec["ms_sweep"] = float(st["ms_prep"]), float(st["ms_sweep"])
    path = os.path.join(out_dir, name + ".npz")
    np.savez(path, **arrays)
    rec["npz"] = path
    rec["seconds"] = time.time() - t0
    return rec


def run_g2o(name, make, env, mode, out_dir, dense):
    for k in CTX_ENV:
        os.environ.pop(k, None)
    os.environ.update(env)
    g = make()
    free_ids = np.flatnonzero(np.asarray(g["fixed"]) == 0).astype(np.int64)
    random_from = free_ids
    if name == "star600":
        random_from = free_ids[free_ids != 0]                         # leaf - leaf pairs
    elif name == "hub42x273":
        random_from = free_ids[free_ids >= N_HUBS]
    return run_graph(name, make_gpu(g), mode, free_ids, g["ei"], g["ej"], random_from, out_dir, dense)


def run_ba(out_dir):
    for k in CTX_ENV:
        os.environ.pop(k, None)
    p = scenarios.ba_problem(*BA_SHAPE)
    n_kf, n_pts = BA_SHAPE
    gr = scenarios.ba_graph(p)
    ei = np.concatenate([p["obs_kf"], np.arange(n_kf - 1)])
    ej = np.concatenate([n_kf + p["obs_pt"], np.arange(1, n_kf)])
    ids = np.arange(n_kf + n_pts, dtype=np.int64)
    return run_graph(BA_GRAPH, gr, "random", ids, ei, ej, ids, out_dir, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--graphs", default="")
    a = ap.parse_args()
    want = [s for s in a.graphs.split(",") if s]
    os.makedirs(a.out, exist_ok=True)
    jobs = [(name, lambda name=name, make=make, env=env, mode=mode: run_g2o(name, make, env, mode, a.out, a.dense)) for name, make, env, mode in G2O_GRAPHS]
    jobs.append((BA_GRAPH, lambda: run_ba(a.out)))
    for name, job in jobs:
        if want and name not in want:
            continue
        try:
            rec = job()
        except Exception as e:      # a refusal or a HIP error: reported, the parent fails the case
            rec = dict(graph=name, status="error: %s: %s" % (type(e).__name__, e))
        rec["maxrss_mb"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
        print("RECORD " + json.dumps(rec), flush=True)
        if rec["status"] != "ok" and "HIP" in rec["status"]:
            return 3                 # after a device error nothing more runs in this process
    return 0


if __name__ == "__main__":
    sys.exit(main())
