"""Child runner of tests/test_gpu_ba_forms.py: FGO_TUNE (ba_schur_cam, ba_small of ba_tables) is read once per process, so every override
set runs in a fresh process -- this script.  It builds the cases of tests/ba_reference.py through the C-ABI with FGO_BA_MIN=1 (every
eligible landmark is eliminated, however few) and prints one JSON record per case; the arrays go to an .npz: the reduced system of
fgo_debug_read_reduced at every lambda of ba_reference.LAMS, read twice, chi2 at the start, and every variable after one
fgo_optimize_gtsam(1) from the same start.  With --generic the landmarks stay columns (FGO_BA_SCHUR=0) and the rows / columns of the
dense H of fgo_linearize that belong to the reduced system are stored instead.  It computes no reference: the parent does.

usage: ba_forms_child.py --out DIR [--generic] [--graphs a,b,...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import graph_slam_amd as G  # noqa: E402
from tests import ba_reference as R  # noqa: E402

UNDERDETERMINED_ITERS = 5


def build(c):
    K, L = c["K"], c["L"]
    gr = G.Graph()
    gr.add_poses(c["poses0"], c["fixed_pose"])
    if c["pose_prior"]:
        gr.add_prior(*c["pose_prior"])
    pts = np.ascontiguousarray(c["points0"])
    pid = np.arange(K, K + L, dtype=np.int64)
    gr._chk(G.lib.fgo_add_points3(gr._h, L, G._i64p(pid), G._dp(pts), 0.0))           # no prior: those follow one by one
    for j in np.nonzero(c["fixed_pt"])[0]:
        gr._chk(G.lib.fgo_set_fixed(gr._h, int(K + j), 1))
    for j, mean, s in zip(c["pp_pt"], c["pp_mean"], c["pp_sigma"]):
        gr.add_prior_point(int(K + j), mean, float(s))
    gr.set_calibration(c["calib"], c["bps"])
    if len(set(c["obs_sigma"])) == 1:
        uv = np.ascontiguousarray(c["obs_uv"])
        okf = np.ascontiguousarray(c["obs_kf"], np.int64); opt = np.ascontiguousarray(K + c["obs_pt"], np.int64)
        gr._chk(G.lib.fgo_add_reprojs(gr._h, len(uv), G._i64p(okf), G._i64p(opt), G._dp(uv), float(c["obs_sigma"][0])))
    else:
        for k, j, uv, s in zip(c["obs_kf"], c["obs_pt"], c["obs_uv"], c["obs_sigma"]):
            gr.add_reproj(int(k), int(K + j), uv, float(s))
    gr.add_edges(c["between_i"], c["between_j"], c["between_z"], np.tile(c["between_info"], (len(c["between_i"]), 1)),
                 tangent_order=G.FGO_TANGENT_GTSAM)
    return gr


def run_case(name, out_dir, generic):
    t0 = time.time()
    c = R.case(name)
    gr = build(c)
    rec = dict(graph=name, status="ok")
    arrays = {}
    if name == "underdetermined":
        rc, st = gr.optimize_gtsam(UNDERDETERMINED_ITERS)
    else:
        if generic:
            stay, _ = R.layout(c)
            free = np.nonzero(np.concatenate([c["fixed_pose"], c["fixed_pt"]]) == 0)[0]
            pos = np.full(c["K"] + c["L"], -1); pos[free] = np.arange(len(free))
            keep = (6 * pos[stay][:, None] + np.arange(6)[None, :]).ravel()
            chi, H, b = gr.linearize(dense=True)
            arrays["H_stay"] = H[np.ix_(keep, keep)]
            del H
        else:
            for i, lam in enumerate(R.LAMS):
                arrays["S%d" % i], arrays["g%d" % i] = gr.read_reduced(lam)
                arrays["S%d_again" % i], arrays["g%d_again" % i] = gr.read_reduced(lam)
        rec["chi2"] = gr.chi2()
        rc, st = gr.optimize_gtsam(1)
        arrays["values"] = gr.get_poses()
    tr = gr.trace()
    rec.update(rc=int(rc), iterations=int(st.iterations), trials=int(st.trials), n_free=int(st.n_free),
               trace_chi2=[float(v) for v in tr[0]], trace_lambda=[float(v) for v in tr[1]])
    path = os.path.join(out_dir, name + ".npz")
    np.savez(path, **arrays)
    rec["npz"] = path
    rec["seconds"] = time.time() - t0
    gr.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--generic", action="store_true")
    ap.add_argument("--graphs", default="")
    a = ap.parse_args()
    os.environ["FGO_BA_MIN"] = "1"
    os.environ["FGO_BA_SCHUR"] = "0" if a.generic else "1"
    want = [s for s in a.graphs.split(",") if s]
    os.makedirs(a.out, exist_ok=True)
    for name in R.CASE_NAMES + ["underdetermined"]:
        if want and name not in want:
            continue
        try:
            rec = run_case(name, a.out, a.generic)
        except Exception as e:      # a refusal or a HIP error: reported, the parent fails the case
            rec = dict(graph=name, status="error: %s: %s" % (type(e).__name__, e))
        print("RECORD " + json.dumps(rec), flush=True)
        if rec["status"] != "ok" and "HIP" in rec["status"]:
            return 3                 # after a device error nothing more runs in this process
    return 0


if __name__ == "__main__":
    sys.exit(main())
