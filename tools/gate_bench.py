"""Gating of candidate edges at config 2 (100k poses, vertex 0 fixed): one JSON line per request shape with the wall time of the
first gate call (it pays the undamped factorisation and the selected inversion), of a repeat call, the device time of the gate
kernel and of the column solves (HIP events), and -- measured in the same run -- the host route to the same numbers: three
marginal_cov_pairs requests (Sigma_aa, Sigma_bb, Sigma_ab) plus the edge Jacobians and the 6x6 algebra in numpy.
Shapes: `newest` = 64 random old poses against the newest pose; `scattered` = 64 candidates, all endpoints distinct and far apart.
    python tools/gate_bench.py [--poses 100000] [--candidates 64]
Plane mode: a VIO-shaped graph with plane hubs (the generator of config 4, graph_slam_amd.scenarios), `observations` plane
observations made at the newest key frame associated with EVERY plane of the map (fgo_associate_planes), against the host route:
three marginal_cov_pairs requests per (key frame, plane) pair plus the numpy reference of tests/plane_gate_reference.py.
    python tools/gate_bench.py --mode plane [--keyframes 5000] [--planes 50] [--observations 8]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graph_slam_amd as G  # noqa: E402
from tests import gate_reference as R  # noqa: E402
from tests import orc_binding as orc  # noqa: E402
from tests import plane_gate_reference as RP  # noqa: E402
from tests.util import info_full  # noqa: E402


def host_route(gr, poses, a, b, meas, info):
    Saa, Sbb, Sab = gr.marginal_cov_pairs(a, a), gr.marginal_cov_pairs(b, b), gr.marginal_cov_pairs(a, b)
    d2 = np.zeros(len(a))
    for k in range(len(a)):
        e, Ja, Jb = orc.edge_se3(poses[a[k]], poses[b[k]], meas[k])
        d2[k] = R.d2_direct(e, R.predicted_cov(Ja, Jb, Saa[k], Sab[k], Sbb[k]), info_full(info[k]))
    return d2


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def plane_host_route(gr, values, x, planes, z, S):
    xs = np.full(len(planes), x)
    Sxx, Spp, Sxp = gr.marginal_cov_pairs(xs, xs), gr.marginal_cov_pairs(planes, planes), gr.marginal_cov_pairs(xs, planes)
    D = np.zeros((len(z), len(planes)))
    for i in range(len(z)):
        for j, pid in enumerate(planes):
            D[i, j] = RP.gate_blocks(values, x, int(pid), z[i], S, Sxx[j], Sxp[j][:, :3], Spp[j][:3, :3])["d2"]
    return D


def plane_mode(args):
    from graph_slam_amd import scenarios as SC
    K, npl, k = args.keyframes, args.planes, args.observations
    p = SC.vio_problem(n_kf=K, n_planes=npl)
    gr, n_plane_factors = SC.vio_graph(p)
    gr.chi2()                                            # structure phase out of the way
    x, planes = K - 1, np.arange(3 * K, 3 * K + npl)
    ids = np.concatenate([[x], planes])
    V = gr.get_poses(ids=ids)
    values = {int(v): V[q] for q, v in enumerate(ids)}
    rng = np.random.default_rng(7)
    seen = rng.choice(npl, k, replace=k > npl)           # the observations: noisy views of k of the planes
    z = np.array([orc.plane_retract(orc.plane_transform(values[3 * K + int(j)][:4], values[x]), rng.normal(size=3) * 0.01) for j in seen])
    S6 = np.tile([1e-4, 0, 0, 1e-4, 0, 1e-4], (k, 1))
    (match, best2, D), first_ms = timed(lambda: gr.associate_planes(x, z, S6, planes, want_matrix=True))
    si = gr.selinv_stats()
    (match_b, _, Db), repeat_ms = timed(lambda: gr.associate_planes(x, z, S6, planes, want_matrix=True))
    st = gr.gate_stats()
    assert np.array_equal(D, Db) and np.array_equal(match, match_b)
    href, host_ms = timed(lambda: plane_host_route(gr, values, x, planes, z, 1e-4 * np.eye(3)))
    print(json.dumps(dict(
        shape="plane", keyframes=K, planes=npl, plane_factors=n_plane_factors, observations=k, candidates=k * npl,
        off_pattern=st["off_pattern"], column_groups=st["column_groups"], first_call_ms=round(first_ms, 3),
        factor_ms=round(si["ms_factor"], 3), selinv_ms=round(si["ms_prep"] + si["ms_sweep"], 3), repeat_call_ms=round(repeat_ms, 3),
        gate_kernel_ms=round(st["ms_kernel"], 4), column_solves_ms=round(st["ms_solves"], 3), host_route_ms=round(host_ms, 3),
        max_rel_diff_vs_host=float(np.abs(D / href - 1).max()), matched=int((match >= 0).sum()),
        matched_right=int((match == 3 * K + seen).sum()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["se3", "plane"], default="se3")
    ap.add_argument("--keyframes", type=int, default=5000)
    ap.add_argument("--planes", type=int, default=50)
    ap.add_argument("--observations", type=int, default=8)
    ap.add_argument("--poses", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--candidates", type=int, default=64)
    args = ap.parse_args()
    if args.mode == "plane":
        return plane_mode(args)
    n, m = args.poses, args.candidates
    g = G.synth_manhattan3d(n, 5, 4, seed=args.seed)
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    rng = np.random.default_rng(7)
    old = rng.choice(np.arange(1, n // 2), m, replace=False)
    spread = rng.permutation(np.arange(1, n - 1))[:2 * m]
    shapes = dict(newest=[(int(v), n - 1) for v in old], scattered=[(int(spread[2 * k]), int(spread[2 * k + 1])) for k in range(m)])
    for name, pairs in shapes.items():
        gr = G.Graph()                                   # a fresh context per shape: the first call pays factor + inversion
        gr.add_poses(g["poses"], fixed)
        gr.add_edges(g["ei"], g["ej"], g["meas"], g["info"])
        gr.chi2()                                        # structure phase out of the way
        a, b, meas, info = R.candidates(rng, g["poses"], pairs)
        (d2, chi2), first_ms = timed(lambda: gr.gate_edges(a, b, meas, info))
        si = gr.selinv_stats()
        (d2b, _), repeat_ms = timed(lambda: gr.gate_edges(a, b, meas, info))
        st = gr.gate_stats()
        assert np.array_equal(d2, d2b)
        href, host_ms = timed(lambda: host_route(gr, g["poses"], a, b, meas, info))
        print(json.dumps(dict(
            shape=name, poses=n, candidates=m, off_pattern=st["off_pattern"], column_groups=st["column_groups"],
            first_call_ms=round(first_ms, 3), factor_ms=round(si["ms_factor"], 3), selinv_ms=round(si["ms_prep"] + si["ms_sweep"], 3),
            repeat_call_ms=round(repeat_ms, 3), gate_kernel_ms=round(st["ms_kernel"], 4), column_solves_ms=round(st["ms_solves"], 3),
            host_route_ms=round(host_ms, 3), max_rel_diff_vs_host=float(np.abs(d2 / href - 1).max()),
            accepted_at_12_59=int((d2 < 12.59).sum()))))


if __name__ == "__main__":
    main()
