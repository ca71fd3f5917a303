"""Child runner of tests/test_gpu_isam_forms.py: FGO_TUNE is read once per process, so every override set runs in a fresh process --
this script.  It drives fgo_isam2_update over a fixed list of small GTSAM-semantics graphs and a fixed sequence of updates and prints
one JSON record per graph; the arrays (delta of every variable after every update, the values the priors were placed at, the
wildfire flags) go to an .npz next to it.  It computes no reference: the parent does.

modes: forms -- twin contexts, FGO_ISAM_PARTIAL=1 / 0 (read per call), relinearisation threshold 1e9 so that theta never moves;
       wild  -- three contexts with wildfire thresholds 0 / 5e-324 / 1e-3 on the same sequences;
       wave  -- twins through a relinearisation wave (threshold 0.1) on a growing graph;
       explore -- for choosing PICKS: a prior on every pose in turn, the ranges that each produces.

usage: isam_forms_child.py --out DIR [--mode forms|wild|wave|explore, or several joined by commas] [--graphs a,b,...]"""
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
from tests.util import info_ut, random_info  # noqa: E402
from tests.launch_forms_child import random_truth, from_pairs, CTX_ENV  # noqa: E402

SOFT_PRIOR = info_ut(np.diag([1e6] * 6))       # tests/test_gpu_isam2.py
WEAK_PRIOR = info_ut(np.eye(6))                # information 1
BIG = 1e9
EXTRA = 10                                     # poses held back for appending (one in the forms / wild sequences, ten in the wave)


def synth_part(n, lookback, n_loop, seed, first_id=0):
    """tests/test_gpu_gtsam.synth_gtsam with EXTRA more poses than n: the first n and the edges among them are the graph, the others
    are appended later with their look-back edges only (an edge from further back would rebuild the structure)"""
    from tests.test_gpu_gtsam import synth_gtsam
    g = synth_gtsam(n + EXTRA, lookback, n_loop, seed)
    newest, oldest = np.maximum(g["ei"], g["ej"]), np.minimum(g["ei"], g["ej"])
    keep = (newest < n) | (newest - oldest <= lookback)
    return dict(poses=g["poses"], ei=g["ei"][keep] + first_id, ej=g["ej"][keep] + first_id, meas=g["meas"][keep], info=g["info"][keep],
                n0=n, priors=[first_id])


def star_part(n):
    """the star of tests/launch_forms_child.py (hub 0, every third spoke pair joined) with random information matrices; the appended
    poses hang on their predecessor"""
    rng = np.random.default_rng(3)
    truth = random_truth(rng, n + EXTRA)
    pairs = [(0, k) for k in range(1, n)] + [(k, k + 1) for k in range(1, n - 1, 3)] + [(k - 1, k) for k in range(n, n + EXTRA)]
    g = from_pairs(rng, truth, pairs, fixed=[])
    return dict(poses=g["poses"], ei=g["ei"], ej=g["ej"], meas=g["meas"], info=g["info"], n0=n, priors=[0])


def two_components():
    """two disjoint synth-200 graphs, each with its own prior; the second one (ids 200 ...) is the one that grows"""
    a, b = synth_part(200, 3, 1, 5), synth_part(200, 3, 1, 6, first_id=200)
    ka = np.maximum(a["ei"], a["ej"]) < 200
    return dict(poses=np.concatenate([a["poses"][:200], b["poses"]]), ei=np.concatenate([a["ei"][ka], b["ei"]]),
                ej=np.concatenate([a["ej"][ka], b["ej"]]), meas=np.concatenate([a["meas"][ka], b["meas"]]),
                info=np.concatenate([a["info"][ka], b["info"]]), n0=400, priors=[0, 200])


# name -> (graph, environment of the context)
GRAPHS = [
    ("synth150_w1", lambda: synth_part(150, 5, 4, 250), {"FGO_TASK_WORK": "1"}),
    ("synth400_w1", lambda: synth_part(400, 5, 4, 500), {"FGO_TASK_WORK": "1"}),
    ("synth650_w50", lambda: synth_part(650, 5, 4, 750), {"FGO_TASK_WORK": "50"}),
    ("synth200_leaf", lambda: synth_part(200, 3, 1, 5), {}),
    ("synth150_w1_nopanels", lambda: synth_part(150, 5, 4, 250), {"FGO_TASK_WORK": "1", "FGO_NO_PANELS": "1"}),
    ("star200", lambda: star_part(200), {}),
    ("twocomp200", two_components, {}),
]
WAVE_GRAPHS = ["synth150_w1", "synth400_w1"]

# Poses that receive the weak priors of updates (b) .. (e), chosen from the output of --mode explore under the default set (the
# structure, and so the choice, does not depend on FGO_TUNE except for chain_work / no_leaf, where the same poses are kept):
#   b: the pose with the longest dirty path, c: a pose of a bottom-level task away from it, d: two poses of one level whose tasks lie
#   furthest apart, e: the pose with the shortest dirty path (its task is a root's; the root columns themselves are reserve slots).
# Each level's range under the default set is [task, task] on a single path and [first task, second task] of level 0 in (d).
PICKS = {
    "synth150_w1": dict(b=126, c=1, d=(127, 2), e=86),
    #   b: 16 dirty tasks from task 3 (level 0); c: task 5, 5 dirty; d: tasks 3 and 5 of level 0 (tasks 0..5); e: task 35, 1 dirty
    "synth400_w1": dict(b=388, c=64, d=(65, 389), e=251),
    #   b: 16 dirty tasks from task 9 (level 0); c: task 0, 6 dirty; d: tasks 0 and 9 of level 0 (tasks 0..11); e: task 55, 1 dirty
    "synth650_w50": dict(b=586, c=608, d=(565, 609), e=552),
    #   b: 13 dirty tasks from task 0 (level 0); c: task 23, 13 dirty; d: tasks 1 and 23 of level 0 (tasks 0..25); e: task 100, 1 dirty
    "synth200_leaf": dict(b=193, c=1, d=(199, 2), e=136),
    #   b: 14 dirty tasks from task 3 (level 0); c: task 6, 5 dirty; d: tasks 2 and 6 of level 0 (tasks 0..6); e: task 42, 1 dirty
    "synth150_w1_nopanels": dict(b=126, c=1, d=(127, 2), e=86),
    #   b: 16 dirty tasks from task 3 (level 0); c: task 5, 5 dirty; d: tasks 3 and 5 of level 0 (tasks 0..5); e: task 35, 1 dirty
    "star200": dict(b=199, c=61, d=(62, 198), e=1),
    #   b: 14 dirty tasks from task 132 (level 0); c: task 0, 2 dirty; d: tasks 0 and 133 of level 0 (tasks 0..135); e: task 20, 2 dirty
    "twocomp200": dict(b=336, c=176, d=(177, 386), e=66),
    #   b: 16 dirty tasks from task 14 (level 0); c: task 0, 3 dirty; d: tasks 0 and 15 of level 0 (tasks 0..18); e: task 41, 1 dirty
    #   (b lies in the second component, c and e in the first, d in both: updates (a) and (b) leave the first component clean)
}
UPDATES = ["first", "a", "b", "c", "d", "e", "f"]


def new_ctx(g, wildfire=None):
    gr = G.Graph()
    if wildfire is not None:
        gr.isam2_set_wildfire(wildfire)
    n0 = g["n0"]
    gr.add_poses(g["poses"][:n0])
    for p in g["priors"]:
        gr.add_prior(p, g["poses"][p], SOFT_PRIOR)
    m = np.maximum(g["ei"], g["ej"]) < n0
    gr.add_edges(g["ei"][m], g["ej"][m], g["meas"][m], g["info"][m], tangent_order=G.FGO_TANGENT_GTSAM)
    return gr


def append_pose(gr, g, k):
    gr.add_poses(g["poses"][k:k + 1], ids=[k])
    m = np.maximum(g["ei"], g["ej"]) == k
    gr.add_edges(g["ei"][m], g["ej"][m], g["meas"][m], g["info"][m], tangent_order=G.FGO_TANGENT_GTSAM)


def steps_of(name, g):
    """the updates after the first: (label, pose to append or None, poses that get a weak prior)"""
    pk = PICKS[name]
    return [("a", g["n0"], []), ("b", None, [pk["b"]]), ("c", None, [pk["c"]]), ("d", None, list(pk["d"])), ("e", None, [pk["e"]]),
            ("f", None, [])]


def census2(gr):
    try:
        return gr.launch_census(fused=2)
    except G.FgoError:
        return None


def last_summary(gr):
    la = gr.isam2_last()
    nl = len(la["level_lo"])
    dirty = np.bincount(la["task_level"][la["task_dirty"] != 0], minlength=nl)
    first = np.concatenate([[0], np.cumsum(la["level_ntask"])[:-1]])
    return la, dict(sweep=la["sweep"], cut=la["cut"], chain_low=la["chain_low"], lo=la["level_lo"].tolist(), hi=la["level_hi"].tolist(),
                    ntask=la["level_ntask"].tolist(), first=first.tolist(), dirty=dirty.tolist(), fwd=la["level_fwd"].tolist(),
                    fwtab=la["level_fwtab"].tolist())


def run_forms(name, g, out_dir):
    twins = {"f": new_ctx(g), "p": new_ctx(g)}                     # the full-sweep twin goes first: the priors sit at ITS values
    arrays, ups = {}, []
    for label, new_pose, prior_ids in [("first", None, [])] + steps_of(name, g):
        at = twins["f"].get_poses()[prior_ids] if prior_ids else np.zeros((0, 7))
        up = dict(label=label, new_pose=new_pose, prior_ids=[int(p) for p in prior_ids])
        for key in ("f", "p"):
            gr = twins[key]
            os.environ["FGO_ISAM_PARTIAL"] = "1" if key == "p" else "0"
            if new_pose is not None:
                append_pose(gr, g, new_pose)
            for p, val in zip(prior_ids, at):
                gr.add_prior(int(p), val, WEAK_PRIOR)
            st = gr.isam2_update(BIG)
            la, summary = last_summary(gr)
            up[key] = dict(r3=int(st.reserved[3]), r4=int(st.reserved[4]), rebuilt=int(st.structure_rebuilt), relin=int(st.reserved[1]),
                           n_tasks=int(st.n_tasks), last=summary, census2=census2(gr))
            arrays["delta_%s_%s" % (key, label)] = la["delta"]
        arrays["prior_at_%s" % label] = at
        ups.append(up)
    rec = dict(updates=ups, census_full=twins["f"].launch_census(fused=True), n_levels=int(twins["f"].stats().n_levels))
    return rec, arrays


WILD = [("exact", 0.0), ("tiny", 5e-324), ("gtsam", 1e-3)]


def run_wild(name, g, out_dir):
    os.environ["FGO_ISAM_PARTIAL"] = "1"
    ctx = {k: new_ctx(g, thr) for k, thr in WILD}
    arrays, ups = {}, []
    for label, new_pose, prior_ids in [("first", None, [])] + steps_of(name, g):
        at = ctx["exact"].get_poses()[prior_ids] if prior_ids else np.zeros((0, 7))
        up = dict(label=label, new_pose=new_pose, prior_ids=[int(p) for p in prior_ids])
        for key, _ in WILD:
            gr = ctx[key]
            if new_pose is not None:
                append_pose(gr, g, new_pose)
            for p, val in zip(prior_ids, at):
                gr.add_prior(int(p), val, WEAK_PRIOR)
            st = gr.isam2_update(BIG)
            la, summary = last_summary(gr)
            up[key] = dict(r3=int(st.reserved[3]), r4=int(st.reserved[4]), rebuilt=int(st.structure_rebuilt), cut=bool(la["cut"]),
                           chain_low=int(la["chain_low"]))
            arrays["delta_%s_%s" % (key, label)] = la["delta"]
            arrays["poses_%s_%s" % (key, label)] = gr.get_poses()
            if key != "exact":
                for f in ("task_run", "task_level", "var_task", "var_chg"):
                    arrays["%s_%s_%s" % (f, key, label)] = la[f]
        ups.append(up)
    return dict(updates=ups, census_full=ctx["exact"].launch_census(fused=True)), arrays


def run_wave(name, g, out_dir):
    n0 = g["n0"]
    g = dict(g)
    g["poses"] = g["poses"].copy()
    g["poses"][n0 - 30:n0, :3] += np.random.default_rng(1).normal(size=(30, 3)) * 0.12     # a stretch that crosses the 0.1 threshold
    arrays, rec = {}, {}
    for key in ("f", "p"):
        os.environ["FGO_ISAM_PARTIAL"] = "1" if key == "p" else "0"
        gr = new_ctx(g)
        stats = [gr.isam2_update(0.1)]
        for k in range(n0, n0 + EXTRA):
            append_pose(gr, g, k)
            stats.append(gr.isam2_update(0.1))
        n = n0 + EXTRA
        th = np.zeros((n, 7)); de = np.zeros((n, 6))
        for v in range(n):
            th[v], de[v] = gr.isam2_state(v)
        arrays["poses_" + key] = gr.get_poses(); arrays["theta_" + key] = th; arrays["delta_" + key] = de
        rec[key] = dict(relin=[int(s.reserved[1]) for s in stats], r3=[int(s.reserved[3]) for s in stats],
                        rebuilt=[int(s.structure_rebuilt) for s in stats])
    return rec, arrays


def run_explore(name, g, out_dir):
    os.environ["FGO_ISAM_PARTIAL"] = "1"
    gr = new_ctx(g)
    gr.isam2_update(BIG)
    append_pose(gr, g, g["n0"])
    st = gr.isam2_update(BIG)
    la, s0 = last_summary(gr)
    rows = []
    for p in range(g["n0"]):
        if p in g["priors"]:
            continue
        gr.add_prior(p, gr.get_poses()[p], WEAK_PRIOR)
        st = gr.isam2_update(BIG)
        la, s = last_summary(gr)
        rows.append(dict(p=p, r3=int(st.reserved[3]), rebuilt=int(st.structure_rebuilt), task=int(la["var_task"][p]),
                         level=int(la["task_level"][la["var_task"][p]]), lo=s["lo"], hi=s["hi"]))
    return dict(append=s0, ntask=s0["ntask"], first=s0["first"], rows=rows, census_full=gr.launch_census(fused=True)), {}


RUN = dict(forms=run_forms, wild=run_wild, wave=run_wave, explore=run_explore)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--mode", default="forms")                 # one of RUN, or several joined by commas
    ap.add_argument("--graphs", default="")
    a = ap.parse_args()
    want = [s for s in a.graphs.split(",") if s]
    os.makedirs(a.out, exist_ok=True)
    for mode in a.mode.split(","):
        for name, make, env in GRAPHS:
            if (want and name not in want) or (mode == "wave" and name not in WAVE_GRAPHS):
                continue
            t0 = time.time()
            for k in CTX_ENV:
                os.environ.pop(k, None)
            os.environ.update(env)
            key = "%s/%s" % (mode, name)                        # (the parent files the records by this)
            try:
                rec, arrays = RUN[mode](name, make(), a.out)
                rec.update(graph=key, status="ok")
                if arrays:
                    rec["npz"] = os.path.join(a.out, "%s_%s.npz" % (mode, name))
                    np.savez(rec["npz"], **arrays)
            except Exception as e:      # a refusal or a HIP error: reported, the parent fails the case
                rec = dict(graph=key, status="error: %s: %s" % (type(e).__name__, e))
            rec["seconds"] = time.time() - t0
            rec["maxrss_mb"] = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0
            print("RECORD " + json.dumps(rec), flush=True)
            if rec["status"] != "ok" and "HIP" in rec["status"]:
                return 3                 # after a device error nothing more runs in this process
    return 0


if __name__ == "__main__":
    sys.exit(main())
