"""Every form of the landmark-elimination kernels (csrc/kernels_ba.hip, ba_tables of csrc/structure_ba.cpp), pinned at small shapes to a dense
reference that shares no formula with the product (tests/ba_reference.py).

Three kernels fill the reduced camera system: k_ba_schur_cam<8,8> (a column camera with <= 80 row blocks, all of its blocks in one
workgroup), k_ba_schur<1> and k_ba_schur<4> (block by block: one wave up to tune("ba_small", 80) pairs, four waves above).  The cases of
ba_reference are built around their strides, batches and masks -- pair lists either side of 20 / 80 entries, cameras with 1 .. 513
observations, column cameras with every number of row blocks 1 .. 90, grids of 1, 7, 8, 9 workgroups through the XCD remap, and a graph
of oddities (a fixed camera, duplicated pairs, landmarks without or with two priors, ...) -- and run with FGO_BA_MIN=1 in four FGO_TUNE
sets.  No census exists for these launches: in the sets blocks / blocks_w1 / blocks_w4 one instantiation alone produces every landmark
term, which is the proof of which form ran.

Bounds, derived from the reference and not from the device (ba_reference.bounds; figures in profiles/NOTES.md "Landmark elimination at
small shapes"): every 6x6 block of S and every camera's part of g within 10 x the worst float64-vs-extended difference of the reference
itself over all cases and lambda, relative to the block's own scale |H_blk|max + sum_p max|W_a (H_pp + lambda I)^-1 W_b^T| (never below
2^-53, never above 1e-10); the variables after one LM iteration within 10 x |delta_float64 - delta_extended|_inf of the case (floor
1e-13 max(1, |delta|_inf), cap 1e-8) of retract(x0, delta) with delta from the extended reference: the direct check of k_ba_back.

FGO_TUNE is read once per process, so each set runs in a fresh child (tests/ba_forms_child.py), one after another, each under its own
timeout; after a child that ends with a signal, an abort, a device error or its timeout no further child is started and every remaining
case fails as "not run after <set>"."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import ba_reference as R
from tests import pose3_independent as p3
from tests.test_gpu_launch_forms import ROOT, _run_child, _stops

CHILD = os.path.join(ROOT, "tests", "ba_forms_child.py")

# (set, FGO_TUNE, child arguments, who fills the reduced system)
SETS = [
    ("default", "", [], "k_ba_schur_cam for cameras with <= 80 row blocks; clique90's ten widest block by block, one wave (12 pairs) and four (112)"),
    ("blocks", "ba_schur_cam=0", [], "k_ba_schur only: one wave up to 80 pairs, four waves above"),
    ("blocks_w1", "ba_schur_cam=0,ba_small=1e9", [], "k_ba_schur<1> alone, the 161- and 513-entry lists included"),
    ("blocks_w4", "ba_schur_cam=0,ba_small=0", [], "k_ba_schur<4> alone, lists of one entry included"),
    ("generic", "", ["--generic"], "no elimination: the landmarks are columns of the block system"),
]
SET_NAMES = [s[0] for s in SETS]
ELIMINATED = SET_NAMES[:4]
ALL_CASES = R.CASE_NAMES + ["underdetermined"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every set in a child of its own, one after another; stops starting children after trouble"""
    base = tmp_path_factory.mktemp("ba_forms")
    out, stopped, limit = {}, None, 300.0          # (the first child also pays the first use of the device)
    for name, tune, args, _ in SETS:
        if stopped:
            out[name] = dict(set=name, tune=tune, rc=None, records={}, seconds=0.0, stderr="", not_run_after=stopped)
            continue
        run = _run_child(name, tune, str(base / name), False, limit, child=CHILD, args=args)
        out[name] = run
        print("[ba forms] set %-10s rc %s  %.1f s" % (name, run["rc"], run["seconds"]))
        if _stops(run["rc"]):
            stopped = name
        if name == "default":
            limit = max(60.0, 10.0 * run["seconds"])                # sized from the measured time of the default set
    return out


def _record(runs, set_name, case):
    run = runs[set_name]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    rec = run["records"].get(case)
    assert rec is not None, "set %s (rc %s) left no record of %s: %s" % (set_name, run["rc"], case, run["stderr"])
    assert rec["status"] == "ok", rec["status"]
    return rec


@functools.lru_cache(maxsize=None)
def _arrays(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("set_name", SET_NAMES)
def test_child_ran_clean(runs, set_name):
    run = runs[set_name]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    assert run["rc"] == 0, (run["rc"], run["stderr"])
    assert sorted(run["records"]) == sorted(ALL_CASES)
    print("[ba forms] %s: child %.1f s; per case %s" % (set_name, run["seconds"],
          ", ".join("%s %.2f" % (g, run["records"][g].get("seconds", -1)) for g in ALL_CASES)))


def _blocks(M, n):
    return np.abs(M).reshape(n, 6, n, 6).max(axis=(1, 3))


@pytest.mark.parametrize("case", R.CASE_NAMES)
@pytest.mark.parametrize("set_name", ELIMINATED)
def test_reduced_system(runs, set_name, case):
    """S, g of fgo_debug_read_reduced at every lambda of ba_reference.LAMS and chi2 against the extended reference"""
    rec = _record(runs, set_name, case)
    a = _arrays(rec["npz"])
    ref, B = R.reference(case, True), R.bounds()
    Hgen = _arrays(_record(runs, "generic", case)["npz"])["H_stay"]
    n = len(ref["stay"])
    assert abs(rec["chi2"] - float(ref["chi2"])) <= 1e-12 * float(ref["chi2"]), (rec["chi2"], float(ref["chi2"]))
    untouched = ~ref["touched"]
    for i, lam in enumerate(R.LAMS):
        S, g = a["S%d" % i], a["g%d" % i]
        what = "%s %s lambda %g" % (set_name, case, lam)
        assert S.shape == (6 * n, 6 * n) and g.shape == (6 * n,), "%s: n_out %d, %d rows / columns stay" % (what, S.shape[0] // 6, n)
        assert np.all(np.isfinite(S)) and np.all(np.isfinite(g)), what
        Sref, gref = ref["S"][lam], ref["g"][lam]
        relS = R.block_rel(_blocks(np.asarray(S, np.longdouble) - Sref, n), ref["S_scale"][lam])
        relg = R.block_rel(np.abs(np.asarray(g, np.longdouble) - gref).reshape(n, 6).max(axis=1), ref["g_scale"][lam])
        wa, wb = np.unravel_index(np.argmax(relS), relS.shape)
        print("[ba forms] %-9s %-9s lambda %-6g S %.3e (bound %.3e, block %d,%d)  g %.3e (bound %.3e)" % (
            set_name, case, lam, relS.max(), B["S"], ref["stay"][wa], ref["stay"][wb], relg.max(), B["g"]))
        assert relS.max() <= B["S"], "%s: block (%d, %d) of S is off by %.3e of its scale, bound %.3e%s" % (
            what, ref["stay"][wa], ref["stay"][wb], relS.max(), B["S"], _marks(case, ref["stay"][wa], ref["stay"][wb]))
        wg = int(np.argmax(relg))
        assert relg.max() <= B["g"], "%s: g of variable %d is off by %.3e of its scale, bound %.3e" % (what, ref["stay"][wg], relg.max(), B["g"])
        # the bounds of tests/test_gpu_ba_oracle.py as well
        Sr64, gr64 = np.asarray(Sref, np.float64), np.asarray(gref, np.float64)
        np.testing.assert_allclose(S, Sr64, rtol=0, atol=1e-10 * np.abs(Sr64).max(), err_msg=what)
        np.testing.assert_allclose(g, gr64, rtol=0, atol=1e-10 * np.abs(gr64).max(), err_msg=what)
        # blocks without a landmark term are the linearised blocks themselves (k_copy_ba), whatever lambda
        S4, H4 = S.reshape(n, 6, n, 6), Hgen.reshape(n, 6, n, 6)
        for x, y in zip(*np.nonzero(untouched)):
            assert np.array_equal(S4[x, :, y, :], H4[x, :, y, :]), "%s: block (%d, %d) receives no landmark term and is not the linearised block" % (
                what, ref["stay"][x], ref["stay"][y])
        # symmetric to the bit where the product mirrors it: off the diagonal blocks, and in diagonal blocks nothing is subtracted from
        off = np.kron(~np.eye(n, dtype=bool) | np.diag(np.diag(untouched)), np.ones((6, 6), bool))
        assert np.array_equal(S[off], S.T[off]), what
        assert (R.block_rel(_blocks(S - S.T, n), ref["S_scale"][lam]) <= 2 * B["S"]).all(), what
        # fixed-order sums: a second call gives the same bits
        assert np.array_equal(S, a["S%d_again" % i]) and np.array_equal(g, a["g%d_again" % i]), what + ": two calls differ"


def _marks(case, va, vb):
    c = R.case(case)
    if not c["marks"]:
        return ""
    seen = [sorted(c["marks"][j] for j in set(c["obs_pt"][c["obs_kf"] == v])) for v in (va, vb) if v < c["K"]]
    return "; landmarks of these cameras: %s" % seen


@functools.lru_cache(maxsize=None)
def _expected_values(case):
    """every variable after one accepted trial at LAM0: retract(x0, delta) of the free poses, x0 + delta of the free landmarks"""
    c, ref = R.case(case), R.reference(case, True)
    K = c["K"]
    want = np.zeros((K + c["L"], 7)); want[:K] = c["poses0"]; want[K:, :3] = c["points0"]
    dc = np.asarray(ref["delta_stay"][R.LAM0], np.float64)
    dl = np.asarray(np.asarray(c["points0"], np.longdouble)[ref["elim"]] + ref["delta_lm"][R.LAM0], np.float64)
    for u, v in enumerate(ref["stay"]):
        if v < K:
            want[v] = p3.retract(c["poses0"][v], [float(x) for x in ref["delta_stay"][R.LAM0][u]])
        else:
            want[v, :3] = c["points0"][v - K] + dc[u, :3]
    want[K + ref["elim"], :3] = dl
    return want


@pytest.mark.parametrize("case", R.CASE_NAMES)
@pytest.mark.parametrize("set_name", SET_NAMES)
def test_one_lm_iteration(runs, set_name, case):
    """fgo_optimize_gtsam(1): one trial at GTSAM's initial lambda is accepted, and every variable lands where the extended reference's
    damped step puts it -- the cameras through the factor / solve kernels, the eliminated landmarks through k_ba_back (landmarks whose
    only camera is fixed included); with the same bounds in the generic form, which shows that they ask the eliminated form for no
    more than the generic one delivers"""
    rec = _record(runs, set_name, case)
    c, B = R.case(case), R.bounds()
    K = c["K"]
    assert rec["rc"] == 1 and rec["iterations"] == 1 and rec["trials"] == 1, rec
    assert rec["n_free"] == int((c["fixed_pose"] == 0).sum() + (c["fixed_pt"] == 0).sum())
    # the trace holds lambda AFTER the iteration: one accepted trial divides the initial 1e-5 by 10
    assert len(rec["trace_lambda"]) == 1 and rec["trace_lambda"][0] == R.LAM0 / 10.0, rec["trace_lambda"]
    got, want = _arrays(rec["npz"])["values"], _expected_values(case)
    bound = B["step"][case]
    sgn = np.sign(np.sum(got[:K, 3:] * want[:K, 3:], axis=1))[:, None]
    err_t = np.abs(got[:K, :3] - want[:K, :3]).max(axis=1)
    err_q = np.abs(got[:K, 3:] * sgn - want[:K, 3:]).max(axis=1)
    err_p = np.abs(got[K:, :3] - want[K:, :3]).max(axis=1)
    print("[ba forms] %-9s %-9s one LM iteration: cameras %.3e / %.3e  landmarks %.3e  (bound %.3e)" % (
        set_name, case, err_t.max(), err_q.max(), err_p.max(), bound))
    fixed = np.concatenate([c["fixed_pose"], c["fixed_pt"]]) == 1
    assert np.array_equal(got[fixed][:, :3], want[fixed][:, :3])           # fixed variables do not move
    assert err_t.max() <= bound and err_q.max() <= bound, "%s %s: camera %d is off by %.3e / %.3e, bound %.3e" % (
        set_name, case, int(np.argmax(np.maximum(err_t, err_q))), err_t.max(), err_q.max(), bound)
    j = int(np.argmax(err_p))
    assert err_p.max() <= bound, "%s %s: landmark %d%s is off by %.3e, bound %.3e" % (
        set_name, case, j, " (%s)" % c["marks"][j] if j in c["marks"] else "", err_p.max(), bound)


def test_underdetermined_landmark_takes_the_same_decisions_in_both_forms(runs):
    """grid7 plus a landmark without a prior that is seen once (H_pp of rank 2: k_ba_points raises fail_flag once lambda no longer
    covers the rounding of its pivots): fgo_optimize_gtsam(5) returns the same code, iterations, trials and lambda trajectory in the
    eliminated and in the generic form, and both take the oracle's decisions"""
    from tests.test_ba_reference_cpu import oracle_problem
    from tests.ba_forms_child import UNDERDETERMINED_ITERS
    po = oracle_problem(R.case("underdetermined"))
    ro, so = po.optimize_gtsam(UNDERDETERMINED_ITERS)
    to = po.trace()
    recs = [_record(runs, s, "underdetermined") for s in SET_NAMES]
    for s, rec in zip(SET_NAMES, recs):
        print("[ba forms] %-9s underdetermined: rc %d iterations %d trials %d lambda %s | oracle rc %d iterations %d trials %d lambda %s" % (
            s, rec["rc"], rec["iterations"], rec["trials"], rec["trace_lambda"], ro, so.iterations, so.trials, list(to[1])))
    for s, rec in zip(SET_NAMES, recs):
        assert (rec["rc"], rec["iterations"], rec["trials"]) == (ro, so.iterations, so.trials), (s, rec)
        np.testing.assert_allclose(rec["trace_lambda"], to[1], rtol=1e-12, err_msg=s)
        np.testing.assert_allclose(rec["trace_lambda"], recs[-1]["trace_lambda"], rtol=1e-12, err_msg=s)
        np.testing.assert_allclose(rec["trace_chi2"], to[0], rtol=1e-8, err_msg=s)
