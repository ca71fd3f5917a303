"""The batched plane check of visual-odometry records (csrc/kernels_plane_check.hip, fgo_plane_check_vro_batch: one wave per record,
all records in one launch) against its numpy restatement (tests/plane_check_reference.py, itself pinned by
tests/test_plane_check_reference_cpu.py).  Reference: gtsam/test_plane_check_vo.cpp computePlaneNodeDis :328-379, computePlaneDis
:383-445.

Tolerances: the project's per-edge tolerance, relative 1e-11, times the condition numbers the reference
computes at run time.  raw, pred_abcd, pred_cov and sdj: 1e-11 x their magnitude (of a vector or matrix: its largest entry).  d2 and
err in cov36 mode: 1e-11 x cond(S_e) x d2; in info mode cond(info) multiplies that.

Records: the generator the calibration test uses (consistent records, matched pairs within 5 deg and 0.1 m, every other pair at
least 20 deg or 0.4 m apart, so no match decision sits within rounding of a threshold).  257 records with ni, nj drawn from 0..9
(empty lists on either side, 1 x 1, a record count that is a multiple of nothing), then 8 x 8 (64 pairs), 5 x 13 (65) and 9 x 9 (81)
whose only match is the last pair, so it sits at the end of the first chunk / in the second chunk of 64, then two i matching one
j.  n_bad == 0 on every generated record is a condition the reference meets on these inputs.  Reference and GPU run once; the
tests share the results and leave them alone."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from tests import plane_check_reference as ref

TOL = 1e-11
I_LAST_88, I_LAST_513, I_LAST_99, I_TWO_ONE = 257, 258, 259, 260
PER_PLANE = ("match", "d2", "raw", "pred_abcd", "pred_cov", "sdj")
PER_RECORD = ("status", "n_matched", "n_bad", "best_i", "best_j", "err", "err_raw")


def _only_last(ni, nj):
    """ni x nj planes whose only common true plane is the last of either list"""
    return list(range(ni)), list(range(ni, ni + nj - 1)) + [ni - 1]


def run(b, mode, **kw):
    return G.plane_check_vro_batch(b["pose"], b["pi_ptr"], b["pi"], b["ci"], b["pj_ptr"], b["pj"], b["cj"],
                                   **{mode: b[mode]}, **kw)


def reference(r, mode, **kw):
    return ref.check_record(r["pose"], r["pi"], r["ci"], r["pj"], r["cj"], **{mode: r[mode]}, **kw)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20250)
    shapes = [(0, 0), (0, 3), (3, 0), (1, 1), (9, 9)] + [tuple(rng.integers(0, 10, 2)) for _ in range(252)]
    recs = [ref.draw_record(rng, *ref.random_sources(rng, int(ni), int(nj))) for ni, nj in shapes]
    recs += [ref.draw_record(rng, *_only_last(8, 8)), ref.draw_record(rng, *_only_last(5, 13)), ref.draw_record(rng, *_only_last(9, 9))]
    recs.append(ref.draw_record(rng, [0, 0, 1], [2, 0, 3]))
    b = ref.pack(recs)
    want = {m: [reference(r, m) for r in recs] for m in ("cov", "info")}
    got = {m: run(b, m) for m in ("cov", "info")}
    return recs, b, want, got


def _check(out, lo, w, mode, tag):
    """the slice of the batch's outputs that starts at plane lo against one record's reference; `out` holds per-record fields
    already reduced to this record"""
    ni = len(w["match"])
    sl = slice(lo, lo + ni)
    scale = TOL * (w["cond_info"] if mode == "info" else 1.0)
    for k in ("status", "n_matched", "n_bad", "best_i", "best_j"):
        assert out[k] == w[k], (tag, k, out[k], w[k])
    np.testing.assert_array_equal(out["match"][sl], w["match"], err_msg=str(tag))
    for i in range(ni):
        pa, pc = out["pred_abcd"][lo + i], out["pred_cov"][lo + i]
        assert np.abs(pa - w["pred_abcd"][i]).max() <= TOL * np.abs(w["pred_abcd"][i]).max(), (tag, i)
        assert np.abs(pc - w["pred_cov"][i]).max() <= TOL * np.abs(w["pred_cov"][i]).max(), (tag, i)
        assert np.array_equal(pc, pc.T), (tag, i)
        assert abs(out["sdj"][lo + i] - w["sdj"][i]) <= TOL * w["sdj"][i], (tag, i)
        if np.isinf(w["d2"][i]):
            assert np.isposinf(out["d2"][lo + i]) and np.isposinf(out["raw"][lo + i]), (tag, i)
            continue
        assert abs(out["raw"][lo + i] - w["raw"][i]) <= TOL * w["raw"][i], (tag, i, out["raw"][lo + i], w["raw"][i])
        assert abs(out["d2"][lo + i] - w["d2"][i]) <= scale * max(w["cond_e"][i], 1.0) * w["d2"][i], \
            (tag, i, out["d2"][lo + i], w["d2"][i], w["cond_e"][i], w["cond_info"])
    if w["best_i"] >= 0:
        assert out["err"] == out["d2"][lo + w["best_i"]] and out["err_raw"] == out["raw"][lo + w["best_i"]], tag
    else:
        assert out["err"] == 0 and out["err_raw"] == 0, tag


def _record(out, k):
    o = {f: out[f] for f in PER_PLANE}
    o.update({f: out[f][k] for f in PER_RECORD})
    return o


@pytest.mark.parametrize("mode", ["cov", "info"])
def test_batch_against_the_reference(mode):
    recs, b, want, got = cases()
    worst = 0.0
    for k, w in enumerate(want[mode]):
        assert w["status"] == ref.PC_OK and w["n_bad"] == 0, k                   # the cap: a condition on the generated records
        _check(_record(got[mode], k), int(b["pi_ptr"][k]), w, mode, (mode, k))
        lo = int(b["pi_ptr"][k])
        for i in np.nonzero(w["match"] >= 0)[0]:
            worst = max(worst, abs(got[mode]["d2"][lo + i] - w["d2"][i]) / (w["cond_e"][i] * w["d2"][i] * (w["cond_info"] if mode == "info" else 1)))
    n_matched = sum(w["n_matched"] for w in want[mode])
    print("%s mode: %d records, %d planes i, %d matched, largest d2 deviation / (cond x d2) %.2e" % (
        mode, len(recs), int(b["pi_ptr"][-1]), n_matched, worst))
    assert n_matched > 300                                                        # the generator did produce work


def test_the_only_match_in_the_last_chunk_and_two_i_on_one_j():
    recs, b, want, got = cases()
    for k, (ni, nj) in ((I_LAST_88, (8, 8)), (I_LAST_513, (5, 13)), (I_LAST_99, (9, 9))):
        w = want["cov"][k]
        assert (len(recs[k]["pi"]), len(recs[k]["pj"])) == (ni, nj)
        assert list(w["match"]) == [-1] * (ni - 1) + [nj - 1] and w["best_i"] == ni - 1       # what the generator was asked for
        assert got["cov"]["best_i"][k] == ni - 1 and got["cov"]["best_j"][k] == nj - 1 and got["cov"]["n_matched"][k] == 1
    w = want["cov"][I_TWO_ONE]
    assert list(w["match"]) == [1, 1, -1]
    lo = int(b["pi_ptr"][I_TWO_ONE])
    assert list(got["cov"]["match"][lo:lo + 3]) == [1, 1, -1] and got["cov"]["n_matched"][I_TWO_ONE] == 2


def test_info_mode_against_cov_mode_fed_the_inverse():
    recs, b, want, got = cases()
    inv = dict(b, cov=np.array([np.linalg.inv(ref.info_full(u)) for u in b["info"]]))
    out = run(inv, "cov")
    for f in ("status", "n_matched", "n_bad", "best_i", "best_j", "match"):
        np.testing.assert_array_equal(out[f], got["info"][f], err_msg=f)
    for k, w in enumerate(want["info"]):
        lo = int(b["pi_ptr"][k])
        for i in range(len(w["match"])):
            bound = 2 * TOL * w["cond_info"] * max(w["cond_e"][i], 1.0) * w["d2"][i]           # either side carries the bound once
            assert abs(out["d2"][lo + i] - got["info"]["d2"][lo + i]) <= bound, (k, i)


def _same_bits(a, b, fields):
    for f in fields:
        assert a[f].tobytes() == b[f].tobytes(), f


@pytest.mark.parametrize("mode", ["cov", "info"])
def test_alone_and_in_the_batch_and_twice_are_bit_identical(mode):
    recs, b, want, got = cases()
    _same_bits(run(b, mode), got[mode], PER_PLANE + PER_RECORD)
    for k in (4, 17, I_LAST_513, I_LAST_99, I_TWO_ONE):
        one = run(ref.pack([recs[k]]), mode)
        lo, hi = int(b["pi_ptr"][k]), int(b["pi_ptr"][k + 1])
        for f in PER_PLANE:
            assert one[f].tobytes() == got[mode][f][lo:hi].tobytes(), (k, f)
        for f in PER_RECORD:
            assert one[f][0].tobytes() == got[mode][f][k].tobytes(), (k, f)


def test_two_identical_planes_i_keep_the_first():
    rng = np.random.default_rng(77)
    r = ref.draw_record(rng, [0], [1, 0])
    r = dict(r, pi=np.repeat(r["pi"], 2, 0), ci=np.repeat(r["ci"], 2, 0))
    out = run(ref.pack([r]), "cov")
    w = reference(r, "cov")
    _check(_record(out, 0), 0, w, "cov", "identical")
    assert w["best_i"] == 0 and list(out["match"]) == [1, 1]
    assert out["d2"][0] == out["d2"][1] == out["err"][0] > 0 and out["best_i"][0] == 0 and out["best_j"][0] == 1


def test_sentinel_and_indefinite_information_leave_their_neighbours_alone():
    recs, b, want, got = cases()
    ks = [I_LAST_513, 10, I_LAST_99, 11, 12]
    batch = [dict(recs[k]) for k in ks]
    A = ref.info_full(batch[1]["info"]); A[0, 0] = 10000.0                       # information (0, 0) == 10000: a failed VO record
    batch[1]["info"] = ref.info_ut21(A)
    bad = np.diag([1.0, 1, 1, 1, 1, -1]); bad[0, 5] = bad[5, 0] = 0.5
    batch[3]["info"] = ref.info_ut21(bad)                                        # indefinite: the last pivot is negative
    out = run(ref.pack(batch), "info")
    assert list(out["status"]) == [G.FGO_PC_OK, G.FGO_PC_SKIPPED, G.FGO_PC_OK, G.FGO_PC_NUM, G.FGO_PC_OK]
    ptr = ref.pack(batch)["pi_ptr"]
    for q, k in enumerate(ks):
        lo, hi = int(ptr[q]), int(ptr[q + 1])
        if q in (1, 3):
            w = reference(batch[q], "info")
            assert w["status"] == out["status"][q]
            _check(_record(out, q), lo, w, "info", ("status", q))
            assert (out["err"][q], out["err_raw"][q], out["n_matched"][q], out["best_i"][q]) == (0, 0, 0, -1)
            assert (out["match"][lo:hi] == -1).all() and not out["d2"][lo:hi].any() and not out["pred_cov"][lo:hi].any()
            continue
        glo, ghi = int(b["pi_ptr"][k]), int(b["pi_ptr"][k + 1])
        for f in PER_PLANE:
            assert out[f][lo:hi].tobytes() == got["info"][f][glo:ghi].tobytes(), (k, f)
        for f in PER_RECORD:
            assert out[f][q].tobytes() == got["info"][f][k].tobytes(), (k, f)
    # the sentinel is a parameter: disabled, the record is checked like any other; and it does not apply to cov36 mode
    off = run(ref.pack(batch[1:2]), "info", params=G.plane_check_params(failed_info00=0.0))
    w = reference(batch[1], "info", failed_info00=0.0)
    assert off["status"][0] == G.FGO_PC_OK
    _check(_record(off, 0), 0, w, "info", "sentinel off")
    c = dict(batch[1], cov=np.diag([10000.0, 1e-4, 1e-4, 1e-4, 1e-4, 1e-4]))
    assert run(ref.pack([c]), "cov")["status"][0] == G.FGO_PC_OK


def test_all_covariances_zero_counts_a_bad_pair():
    z = np.zeros((1, 16))
    r = dict(pose=np.array([0.1, 0, 0, 0, 0, 0, 1.0]), cov=np.zeros((6, 6)), info=np.zeros(21), pi=np.array([[0, 0, 2.0, 1.0]]), ci=z,
             pj=np.array([[0.02, 0, 1.0, 1.01]]), cj=z)
    out = run(ref.pack([r]), "cov")
    assert (out["status"][0], out["n_matched"][0], out["n_bad"][0], out["err"][0], out["err_raw"][0], out["best_i"][0], out["best_j"][0]) == \
        (G.FGO_PC_OK, 1, 1, 0, 0, -1, -1)
    assert out["match"][0] == 0 and np.isposinf(out["d2"][0]) and np.isposinf(out["raw"][0])
    np.testing.assert_allclose(out["pred_abcd"][0], [0, 0, 1, 1], atol=1e-15)     # (a, b, c) normalised, d untouched
    assert not out["pred_cov"].any() and out["sdj"][0] == 0


def test_thresholds_are_parameters():
    recs, b, want, got = cases()
    ks = [I_LAST_99, 20, 21]
    batch = [recs[k] for k in ks]
    prm = dict(cos_min=float(np.cos(np.deg2rad(60.0))), d_max=1.5)               # decoys start to match: other pairs are selected
    out = run(ref.pack(batch), "cov", params=G.plane_check_params(**prm))
    ptr = ref.pack(batch)["pi_ptr"]
    changed = False
    for q, r in enumerate(batch):
        w = reference(r, "cov", **prm)
        np.testing.assert_array_equal(out["match"][int(ptr[q]):int(ptr[q + 1])], w["match"])
        assert (out["best_i"][q], out["best_j"][q], out["n_matched"][q]) == (w["best_i"], w["best_j"], w["n_matched"])
        changed = changed or list(w["match"]) != list(want["cov"][ks[q]]["match"])
    assert changed


def test_two_view_information_goes_straight_into_the_check():
    """the pipeline: fgo_two_view_ba_batch's pose and information for 8 records are handed on as they are; the planes of either
    frame are generated from the ground-truth pose of the bundle adjustment's own generator.  Every err is below 16.27, the
    99.9 % quantile of chi-square with 3 degrees of freedom."""
    from tests.test_gpu_two_view import make_pair, run_batch
    pairs = [make_pair(300 + k, 40 + 5 * k, 1.0) for k in range(8)]
    ba = run_batch(pairs)
    assert (ba["status"] == G.FGO_TV_OK).all()
    rng = np.random.default_rng(4)
    recs = []
    for k, p in enumerate(pairs):
        while True:
            pi, ci, pj, cj = ref.draw_planes(rng, p["truth_j"], [0, 1], [1, 0])
            if ref.well_separated(ba["pose_j"][k], pi, pj):
                break
        recs.append(dict(pose=ba["pose_j"][k], info=ba["info"][k], cov=ba["cov"][k], pi=pi, ci=ci, pj=pj, cj=cj))
    out = run(ref.pack(recs), "info")
    print("err of the 8 records:", np.array2string(out["err"], precision=3))
    assert (out["status"] == G.FGO_PC_OK).all() and (out["n_matched"] == 2).all() and (out["n_bad"] == 0).all()
    for k, r in enumerate(recs):
        assert list(out["match"][2 * k:2 * k + 2]) == [1, 0]
        w = reference(r, "info")
        assert abs(out["err"][k] - w["err"]) <= TOL * w["cond_info"] * w["cond_e"].max() * w["err"], (k, out["err"][k], w["err"])
    assert (out["err"] < 16.27).all() and (out["err"] > 0).all()
