"""The batched IMU check of visual-odometry records (csrc/kernels_imu_check.hip, fgo_imu_check_vro_batch: one wave per record, all
records in one launch) against its numpy restatement (tests/imu_check_reference.py, itself pinned by
tests/test_imu_check_reference_cpu.py).  Reference: gtsam/test_vro_imu_graph.cpp:679-778.

ONE batch of 131 records over 7 preintegrations of 0, 1, 2, 3, 20, 40 and 200 samples, every preintegration named by at least two
records.  The extrinsic and the presence of a bias array belong to a call, not to a record, so the batch runs in two
configurations -- "plain" (no extrinsic, no bias array) and "full" (a random extrinsic; a bias array in which the records drawn
without a bias pass their preintegration's own bhat) -- once per mode (info, cov); the four results are shared by the tests.
  general (108)   the rotation the record reports is the preintegrated one turned by 1e-3, 0.05, 0.2, 0.3 (either side of the 0.25
                  series switch), 1.0 or 3.0 rad about a random axis, on every preintegration with samples, a third of them without
                  a bias of their own
  statuses (5)    the failed-VO sentinel, an indefinite information matrix, three records on the preintegration without samples,
                  in the middle of the batch
  near zero (18)  q_ij is the preintegration's dR to the bit, or that turned by 1e-12 or 1e-9 rad; checked in the plain configuration

Tolerances: the project's per-value tolerance, relative 1e-11, times the condition numbers the restatement
computes at run time.  dw: absolute 1e-11.  cov_dw: 1e-11 x its largest entry (x cond(info) in info mode).  d2: 1e-11 x cond(S) x d2
(x cond(info) in info mode).  d2_ref: 1e-11 x cond(Sigma15) x d2_ref.  Near zero: dw absolute 1e-11 and
d2 <= (|dw_ref| + sqrt(3) 1e-11)^2 / lambda_min(S_ref), the largest value a dw within the bound can give."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from tests import imu_check_reference as ref

TOL = 1e-11
SAMPLES = (0, 1, 2, 3, 20, 40, 200)
ANGLES = (1e-3, 0.05, 0.2, 0.3, 1.0, 3.0)
FIELDS = ("status", "reject", "d2", "d2_ref", "angle", "dw", "cov_dw")
CONFIGS = ("plain", "full")


def run(b, mode, q_uc=None, **kw):
    kw.setdefault("want_dw", True); kw.setdefault("want_cov", True)
    return G.imu_check_vro_batch(b["pose"], b["pres"], b["index"], bias_i=b["bias"], imu_q_cam=q_uc, **{mode: b[mode]}, **kw)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20260)
    pres = [ref.make_preint(rng, n, bias_hat=1e-2 * rng.normal(size=6)) for n in SAMPLES]
    q_uc = ref.random_unit(rng, 4)
    conf = {"plain": (None, False), "full": (q_uc, True)}
    both = tuple(conf.values())
    recs, group = [], []
    for k in range(1, 7):
        for a in ANGLES:
            for v in range(3):
                recs.append(ref.draw_record(rng, pres, k, a, v != 2, configs=both)); group.append("general")
    # the status records go in the middle of the batch
    st = [ref.draw_record(rng, pres, 4, 0.05, True, configs=both) for _ in range(2)]
    st[0]["info"] = ref.sentinel_info(st[0]["info"])                              # information (0, 0) == 10000: a failed VO record
    bad = np.diag([1.0, 1, 1, 1, 1, -1]); bad[0, 5] = bad[5, 0] = 0.5
    st[1]["info"] = ref.info_ut21(bad)                                           # indefinite: the last pivot is negative
    st += [ref.draw_record(rng, pres, 0, a, v == 0) for v, a in enumerate((0.05, 0.3, 1.0))]
    recs[50:50] = st; group[50:50] = ["sentinel", "indefinite", "empty", "empty", "empty"]
    for k in range(1, 7):
        for a in (0.0, 1e-12, 1e-9):
            r = ref.draw_record(rng, pres, k, a, False, configs=both)
            if a == 0.0:
                r["pose"] = np.concatenate([r["t"], pres[k][ref.DR]])             # the preintegration's dR to the bit
            recs.append(r); group.append("near")
    assert len(recs) == 131 and all(sum(r["k"] == k for r in recs) >= 2 for k in range(7))
    packs, want, got = {}, {}, {}
    for c, (q, ub) in conf.items():
        b = ref.pack(recs, pres, q, ub); b["pres"] = np.array(pres)
        packs[c] = b
        for m in ("cov", "info"):
            want[c, m] = [ref.check_record(**{m: r[m]}, **ref.record_args(r, pres, q, ub)) for r in recs]
            got[c, m] = run(b, m, q)
    return recs, np.array(group), conf, packs, want, got


def _rec(out, k):
    return {f: out[f][k] for f in FIELDS}


def _check_general(o, w, mode, tag):
    ci = w["cond_info"] if mode == "info" else 1.0
    assert o["status"] == w["status"] == G.FGO_IC_OK and o["reject"] == w["reject"], (tag, o["status"], o["reject"], w["reject"])
    err = dict(dw=np.abs(o["dw"] - w["dw"]).max() / TOL,
               cov_dw=np.abs(o["cov_dw"] - w["cov_dw"]).max() / (TOL * ci * np.abs(w["cov_dw"]).max()),
               d2=abs(o["d2"] - w["d2"]) / (TOL * ci * w["cond_S"] * w["d2"]),
               d2_ref=abs(o["d2_ref"] - w["d2_ref"]) / (TOL * w["cond_cov15"] * w["d2_ref"]),
               angle=abs(o["angle"] - w["angle"]) / TOL)
    for f, e in err.items():
        assert e <= 1.0, (tag, f, e, o[f], w[f], w["cond_S"], w["cond_info"], w["cond_cov15"])
    assert np.array_equal(o["cov_dw"], o["cov_dw"].T), tag
    return err


@pytest.mark.parametrize("mode", ["cov", "info"])
@pytest.mark.parametrize("config", CONFIGS)
def test_general_records_against_the_reference(config, mode):
    recs, group, conf, packs, want, got = cases()
    worst = {}
    idx = np.nonzero(group == "general")[0]
    for k in idx:
        err = _check_general(_rec(got[config, mode], k), want[config, mode][k], mode, (config, mode, k))
        worst = {f: max(e, worst.get(f, 0.0)) for f, e in err.items()}
    print("%s / %s, %d general records: largest error as a share of its bound: %s" % (
        config, mode, len(idx), ", ".join("%s %.1e" % fe for fe in worst.items())))
    rej = got[config, mode]["reject"][idx]
    for bit in (1, 2):                                                            # both bits occur set and clear
        assert ((rej & bit) != 0).any() and ((rej & bit) == 0).any(), (bit, np.bincount(rej, minlength=4))


@pytest.mark.parametrize("config", CONFIGS)
def test_the_generated_records_are_well_posed(config):
    """runs the restatement alone: no numerical failure in the general and near-zero groups, no reject bit near its gate"""
    recs, group, conf, packs, want, got = cases()
    for m in ("cov", "info"):
        for k in np.nonzero((group == "general") | (group == "near"))[0]:
            w = want[config, m][k]
            assert w["status"] == ref.IC_OK, (config, m, k)
            assert abs(w["d2"] - ref.D2_GATE) > 1e-6 * ref.D2_GATE and abs(w["d2_ref"] - ref.D2_REF_GATE) > 1e-6 * ref.D2_REF_GATE


@pytest.mark.parametrize("mode", ["cov", "info"])
def test_near_zero(mode):
    recs, group, conf, packs, want, got = cases()
    worst = 0.0
    for k in np.nonzero(group == "near")[0]:
        o, w = _rec(got["plain", mode], k), want["plain", mode][k]
        assert np.abs(o["dw"] - w["dw"]).max() <= TOL, (k, o["dw"], w["dw"])
        worst = max(worst, np.abs(o["dw"] - w["dw"]).max())
        assert o["status"] == G.FGO_IC_OK and o["reject"] == 0, k
        cap = (np.sqrt(w["dw"] @ w["dw"]) + np.sqrt(3.0) * TOL) ** 2 / np.linalg.eigvalsh(w["cov_dw"])[0]
        assert 0 <= o["d2"] <= cap, (k, o["d2"], cap)
        assert np.array_equal(o["cov_dw"], o["cov_dw"].T)
        assert np.abs(o["cov_dw"] - w["cov_dw"]).max() <= TOL * (w["cond_info"] if mode == "info" else 1.0) * np.abs(w["cov_dw"]).max()
    print("%s mode, near zero: largest |dw - dw_ref| %.2e" % (mode, worst))


@pytest.mark.parametrize("config", CONFIGS)
def test_statuses_and_zeroed_outputs(config):
    recs, group, conf, packs, want, got = cases()
    zero = lambda o: o["reject"] == 0 and o["d2"] == 0 and o["d2_ref"] == 0 and o["angle"] == 0 and not o["dw"].any() and not o["cov_dw"].any()
    s, = np.nonzero(group == "sentinel"); i, = np.nonzero(group == "indefinite")
    for m in ("cov", "info"):
        for k in np.nonzero(group == "empty")[0]:
            assert got[config, m]["status"][k] == want[config, m][k]["status"] == G.FGO_IC_NUM and zero(_rec(got[config, m], k)), (m, k)
    o = got[config, "info"]
    assert o["status"][s[0]] == want[config, "info"][s[0]]["status"] == G.FGO_IC_SKIPPED and zero(_rec(o, s[0]))
    assert o["status"][i[0]] == want[config, "info"][i[0]]["status"] == G.FGO_IC_NUM and zero(_rec(o, i[0]))
    for k in (s[0], i[0]):                                                        # in cov mode both are records like any other
        _check_general(_rec(got[config, "cov"], k), want[config, "cov"][k], "cov", (config, "cov", k))


@pytest.mark.parametrize("mode", ["cov", "info"])
def test_twice_reversed_and_without_the_status_records_are_bit_identical(mode):
    recs, group, conf, packs, want, got = cases()
    q, ub = conf["full"]
    b, g = packs["full"], got["full", mode]
    again = run(b, mode, q)
    for f in FIELDS:
        assert again[f].tobytes() == g[f].tobytes(), f
    rev = dict(b, **{f: b[f][::-1].copy() for f in ("pose", "info", "cov", "index", "bias")})
    back = run(rev, mode, q)
    for f in FIELDS:
        assert back[f][::-1].tobytes() == g[f].tobytes(), f
    # the status records' neighbours: the batch without them gives the same bits
    keep = np.nonzero(~np.isin(group, ("sentinel", "indefinite", "empty")))[0]
    sub = dict(b, **{f: b[f][keep].copy() for f in ("pose", "info", "cov", "index", "bias")})
    alone = run(sub, mode, q)
    for f in FIELDS:
        assert alone[f].tobytes() == g[f][keep].tobytes(), f


def test_batch_boundaries_and_optional_outputs():
    recs, group, conf, packs, want, got = cases()
    b, g = packs["plain"], got["plain", "info"]
    for k in (0, 77, 130):
        one = run(dict(b, **{f: b[f][k:k + 1].copy() for f in ("pose", "info", "cov", "index")}), "info")
        for f in FIELDS:
            assert one[f][0].tobytes() == g[f][k].tobytes(), (k, f)
    empty = run(dict(b, **{f: b[f][:0].copy() for f in ("pose", "info", "cov", "index")}), "info")          # FGO_OK: nothing raised
    assert all(len(empty[f]) == 0 for f in FIELDS)
    for kw in (dict(want_dw=False, want_cov=False), dict(want_dw=True, want_cov=False), dict(want_dw=False, want_cov=True)):
        o = run(b, "info", **kw)
        assert ("dw" in o, "cov_dw" in o) == (kw["want_dw"], kw["want_cov"])
        for f in o:
            assert o[f].tobytes() == g[f].tobytes(), (kw, f)


def test_gates_are_parameters():
    recs, group, conf, packs, want, got = cases()
    q, ub = conf["full"]
    keep = np.nonzero(group == "general")[0][::5]
    b = packs["full"]
    sub = dict(b, **{f: b[f][keep].copy() for f in ("pose", "info", "cov", "index", "bias")})
    gates = dict(d2_gate=0.5, d2_ref_gate=100.0)
    o = run(sub, "cov", q, params=G.imu_check_params(**gates))
    w = [ref.check_record(cov=recs[k]["cov"], **ref.record_args(recs[k], b["pres"], q, ub), **gates) for k in keep]
    assert all(min(abs(x["d2"] - 0.5) / 0.5, abs(x["d2_ref"] - 100.0) / 100.0) > 1e-6 for x in w)
    assert list(o["reject"]) == [x["reject"] for x in w]
    assert list(o["reject"]) != list(got["full", "cov"]["reject"][keep])          # the gates did move decisions
    assert o["d2"].tobytes() == got["full", "cov"]["d2"][keep].tobytes()
