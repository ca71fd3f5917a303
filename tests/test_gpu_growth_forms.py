"""The linearised system after the structure has been extended IN PLACE (refresh_factors, structure_grow.cpp), pinned at the H / b level.

Every case of tests/growth_forms.py grows a small graph step by step through one of the forms the extension has to get right -- a
duplicate group forming or gaining a member in either orientation, a duplicate on a pair with a fixed end, a variable crossing the
hub threshold (64 / 65 half-edges), a hub going from one slice to several (512 / 513, 1024 / 1025: k_hub_combine*), plane and point
hubs with their padding identity, planes / points / priors / plane and reprojection factors appended in place, the masked ISAM2
linearisation losing its precondition mid-run, the hub buffers overflowing (256 / 257 entries: one rebuild).  After every step:
  * fgo_debug_linearize_census against the ledger (tests/growth_forms.py ledger(), checked without a device by
    tests/test_growth_forms_cpu.py), exactly -- the proof that the form a case is named for really ran, and structure_rebuilt;
  * chi2, H, b of linearize(dense=True) at the values read back with get_poses(), every entry, against
      - g2o semantics: tests/se3_independent.py (4x4 matrices, forward-mode AD), H at 1e-9 max|H|, b at 1e-9 max(1, max|b|) (the
        figures of tests/test_gpu_independent.py), chi2 at 1e-11 (sums of up to 1 036 positive terms: 1036 x 1.1e-16 = 1.2e-13 from
        the order of summation, the rest is the residuals' own rounding, |e| ~ 0.05 from poses of size ~ 3: ~ 1e-14 relative);
      - GTSAM semantics: the oracle's dense_system() (tests.util.mixed_oracle), H and b at 1e-10 max|.|, chi2 at 1e-11;
      - both: a context with growth off holding the same graph and values from scratch, at 1e-12 max|.| (1 025 terms in another
        order differ by at most 1025 x 1.1e-16 = 1.2e-13 of the sum of magnitudes);
  * the last step: linearize() twice, bitwise.
Cases that need FGO_TUNE (hub_deg=2; the masked form's switch) run in fresh children (tests/growth_forms_child.py), one after another
under `timeout -k 10`, with the stop rule of tests/test_gpu_launch_forms.py: after a signal, abort, device error or timeout no further
child is started."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import growth_forms as GF
from tests import se3_independent as ind
from tests.growth_forms_child import unpack
from tests.test_gpu_launch_forms import ROOT, _run_child, _stops
from tests.util import mixed_oracle, SR4000_CALIB

import os

CHILD = os.path.join(ROOT, "tests", "growth_forms_child.py")
CASES = GF.all_cases()
INPROC = [f()["name"] for f in GF.INPROC_CASES]
HUB2 = [f()["name"] for f in GF.HUB2_CASES]
MASKED_PLAIN = "isam_lookahead=0,isam_masked=0"        # the switch of test_updates_without_lookahead_flags_and_masked_linearisation_give_the_same_states
CHILDREN = [("hub2", "hub_deg=2", HUB2), ("masked_fast", "", ["masked_then_not"]), ("masked_plain", MASKED_PLAIN, ["masked_then_not"])]
CHILD_SECONDS = 120


@pytest.fixture(scope="module")
def data():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = GF.realise(CASES[name])
        return cache[name]
    return get


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    base = tmp_path_factory.mktemp("growth_forms")
    out, stopped = {}, None
    for name, tune, cases in CHILDREN:
        if stopped:
            out[name] = dict(set=name, rc=None, records={}, stderr="", not_run_after=stopped)
            continue
        run = _run_child(name, tune, str(base / name), False, CHILD_SECONDS + 30, child=CHILD, args=("--cases", ",".join(cases)),
                         prefix=("timeout", "-k", "10", str(CHILD_SECONDS)))
        out[name] = run
        print("[growth forms] child %-12s rc %s  %.1f s  %s" % (name, run["rc"], run["seconds"],
              {g: round(r.get("seconds", -1), 2) for g, r in run["records"].items()}))
        if _stops(run["rc"]):
            stopped = name
    return out


def _child_records(children, child, case):
    run = children[child]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    rec = run["records"].get(case)
    assert rec is not None, "child %s (rc %s) left no record of %s: %s" % (child, run["rc"], case, run["stderr"])
    assert rec["status"] == "ok", rec["status"]
    return unpack(rec["steps"], rec["npz"])


# ---- references ----------------------------------------------------------------------------------------------------------------
def _close(a, ref, tol, scale, what):
    a, ref = np.asarray(a), np.asarray(ref)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    err = float(np.abs(a - ref).max()) if a.size else 0.0
    print("[growth forms] %s: max error %.3e (bound %.3e)" % (what, err, tol * scale))
    assert np.all(np.isfinite(a)) and err <= tol * scale, "%s: %.3e > %.3e" % (what, err, tol * scale)


class _G2oReference:
    """H, b, chi2 of tests/se3_independent.py, edge by edge: a step adds the terms of its own edges to the sums of the steps before
    (the values do not move in these cases -- checked -- and new free vertices take the last rows)"""

    def __init__(self, d):
        self.d, self.H, self.b, self.chi, self.E, self.values = d, np.zeros((0, 0)), np.zeros(0), 0.0, 0, None

    def upto(self, values, N, E):
        d = self.d
        if self.values is not None and not np.array_equal(values[:len(self.values)], self.values):
            self.H, self.b, self.chi, self.E = np.zeros((0, 0)), np.zeros(0), 0.0, 0
        sl = slice(self.E, E)
        Hn, bn, chin, free, _ = ind.dense_system(values, d["fixed"][:N], d["ei"][sl], d["ej"][sl], d["meas"][sl], d["info"][sl])
        m = len(self.b)
        Hn[:m, :m] += self.H; bn[:m] += self.b
        chi2 = ind.chi2(values, d["ei"][sl], d["ej"][sl], d["meas"][sl], d["info"][sl])
        assert abs(chi2 - chin) <= 1e-12 * max(chin, 1e-300)          # the two routes of the reference itself
        self.H, self.b, self.chi, self.E, self.values = Hn, bn, self.chi + chi2, E, values.copy()
        return self.H, self.b, self.chi


def _oracle(d, values, N, E, NP):
    vals = values.copy()
    vals[d["kinds"][:N] == GF.PLANE, 4:] = 0
    vals[d["kinds"][:N] == GF.POINT, 3:] = 0
    g = dict(values=vals, vkind=d["kinds"][:N], ei=d["ei"][:E], ej=d["ej"][:E], kind=d["fkind"][:E], meas=d["meas"][:E], info=d["info"][:E],
             prior_ids=d["prior_ids"][:NP], prior_mean=d["prior_mean"][:NP], prior_info=d["prior_info"][:NP], calib=SR4000_CALIB, bps=GF.BPS)
    po = mixed_oracle(g)
    H, b = po.dense_system()
    return H, b, po.chi2()


def check_case(case, d, recs):
    led = GF.ledger(case)
    gtsam = case["sem"] == "gtsam"
    assert len(recs) == len(led)
    ref_g2o = _G2oReference(d)
    for s, (rec, L) in enumerate(zip(recs, led)):
        tag = "%s step %d" % (case["name"], s)
        N, E, NP = GF.counts(case, s)
        cen = rec["census"]
        print("[growth forms] %s: census %s" % (tag, cen))
        assert {k: cen[k] for k in GF.CENSUS_KEYS} == {k: L[k] for k in GF.CENSUS_KEYS}, tag
        if "update" in rec:
            assert rec["update"]["rebuilt"] == L["structure_rebuilt"], tag
        if "H" not in rec:
            continue
        values = rec["values"]
        assert values.shape == (N, 7)
        nfree = int((d["fixed"][:N] == 0).sum())
        assert rec["H"].shape == (6 * nfree, 6 * nfree) and rec["b"].shape == (6 * nfree,)
        if gtsam:
            H, b, chi = _oracle(d, values, N, E, NP)
            tol_H = tol_b = 1e-10; scale_b = np.abs(b).max()
        else:
            H, b, chi = ref_g2o.upto(values, N, E)
            tol_H = tol_b = 1e-9; scale_b = max(1.0, np.abs(b).max())
        _close(rec["H"], H, tol_H, np.abs(H).max(), tag + " H vs reference")
        _close(rec["b"], b, tol_b, scale_b, tag + " b vs reference")
        _close(rec["chi2"], chi, 1e-11, abs(chi), tag + " chi2 vs reference")
        # the same graph and values in a context built from scratch, growth off
        Lt = GF.ledger(case, growth=False)[s]
        assert {k: rec["t_census"][k] for k in GF.CENSUS_KEYS} == {k: Lt[k] for k in GF.CENSUS_KEYS}, tag
        _close(rec["H"], rec["t_H"], 1e-12, np.abs(rec["t_H"]).max(), tag + " H vs rebuilt")
        _close(rec["b"], rec["t_b"], 1e-12, np.abs(rec["t_b"]).max(), tag + " b vs rebuilt")
        _close(rec["chi2"], rec["t_chi2"], 1e-12, abs(rec["t_chi2"]), tag + " chi2 vs rebuilt")
        print("[growth forms] %s: grown and rebuilt bit-identical: H %s, b %s, chi2 %s" % (
            tag, np.array_equal(rec["H"], rec["t_H"]), np.array_equal(rec["b"], rec["t_b"]), rec["chi2"] == rec["t_chi2"]))
        if gtsam:                                               # padding of the 3-dof variables: identity, exactly
            for v in np.nonzero(d["kinds"][:N] != GF.POSE)[0]:
                pad = np.r_[6 * v + 3:6 * v + 6]
                want = np.zeros((3, 6 * N)); want[np.arange(3), pad] = 1.0
                assert np.array_equal(rec["H"][pad], want) and np.array_equal(rec["H"][:, pad], want.T), (tag, v)
                assert np.array_equal(rec["b"][pad], np.zeros(3)), (tag, v)
    last = recs[-1]
    assert last["r_chi2"] == last["chi2"] and np.array_equal(last["r_H"], last["H"]) and np.array_equal(last["r_b"], last["b"])


# ---- the cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", INPROC)
def test_grown_in_place(data, name):
    case = CASES[name]
    check_case(case, data(name), GF.drive(case, data(name)))


@pytest.mark.parametrize("child", [c[0] for c in CHILDREN])
def test_child_ran_clean(children, child):
    run = children[child]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    assert run["rc"] == 0, (run["rc"], run["stderr"])
    assert sorted(run["records"]) == sorted(dict((c[0], c[2]) for c in CHILDREN)[child])


@pytest.mark.parametrize("name", HUB2)
def test_grown_in_place_with_every_variable_a_hub(children, data, name):
    """hub_deg = 2: all-hubs (built that way and grown that way) and the hub_cap overflow -- in place at 256 entries, one rebuild at
    the step the ledger predicts, H and b right on both sides of it"""
    check_case(CASES[name], data(name), _child_records(children, "hub2", name))


def test_plane_and_point_hub_forms_are_the_ones_named(data):
    """(what check_case proves from the census, spelt out for the two landmark hubs: one slice at 65, two slices -- k_hub_combine_gtsam
    -- at 513, the duplicate groups of kind FK_PLANE / FK_REPROJ, and the point's prior on the hub)"""
    for name, kind in (("plane_hub", GF.PLANEF), ("point_hub", GF.REPROJ)):
        led = GF.ledger(CASES[name])
        d = data(name)
        assert [(L["n_hubs"], L["n_hub_multi"]) for L in led] == [(0, 0), (0, 0), (1, 0), (1, 0), (2, 1)]
        assert all(d["fkind"][e] == kind for m in led[-1]["dup_groups"].values() for e in m) and led[-1]["n_dup_groups"] == 65
    assert 8 in data("point_hub")["prior_ids"] and 8 not in data("plane_hub")["prior_ids"]


def test_masked_then_not_equals_the_context_that_never_masks(children, data):
    """updates at threshold 0.02 with look-ahead flags and the masked linearisation, a duplicate between factor appended in place in
    the middle: the census says maskable before it and not after, and after EVERY update the estimate equals, bit for bit, that of a
    process that never takes the masked form; H, b, chi2 after the last update against the references"""
    case, d = CASES["masked_then_not"], data("masked_then_not")
    fast = _child_records(children, "masked_fast", "masked_then_not")
    plain = _child_records(children, "masked_plain", "masked_then_not")
    assert [r["census"]["maskable"] for r in fast] == [1, 1, 1, 1, 0, 0, 0] == [r["census"]["maskable"] for r in plain]
    assert [r["update"]["relin"] for r in fast] == [r["update"]["relin"] for r in plain] and sum(r["update"]["relin"] for r in fast[1:]) > 0
    for s, (a, b) in enumerate(zip(fast, plain)):
        np.testing.assert_array_equal(a["values"], b["values"], err_msg="estimate after update %d" % s)
        assert a["update"]["chi1"] == b["update"]["chi1"]
        # chi2 at the linearisation point: per variable (masked form) against per workgroup -- the same terms in another order
        np.testing.assert_allclose(a["update"]["chi0"], b["update"]["chi0"], rtol=1e-13)
    check_case(case, d, fast)
    check_case(case, d, plain)


def test_masked_case_blocks_vs_matrix_logarithm(children, data):
    """the pose-only case against tests/pose3_independent.py (40-digit matrix logarithm) at 1e-9, on 3 factors: the off-diagonal block of
    the pair (20, 21) that became a duplicate group in place (both members) and the block of the last factor appended in place"""
    from tests import pose3_independent as p3
    d = data("masked_then_not")
    rec = _child_records(children, "masked_fast", "masked_then_not")[-1]
    H, x = rec["H"], rec["values"]
    scale = np.abs(H).max()
    for a, b in ((20, 21), (38, 39)):
        es = [e for e in range(len(d["ei"])) if (d["ei"][e], d["ej"][e]) == (a, b)]
        assert len(es) == (2 if a == 20 else 1)
        blk = np.zeros((6, 6))
        for e in es:
            _, Ji, Jj = p3.between(x[a], x[b], d["meas"][e])
            blk += Ji.T @ ind.info_full(d["info"][e]) @ Jj
        _close(H[6 * a:6 * a + 6, 6 * b:6 * b + 6], blk, 1e-9, scale, "masked_then_not H[%d,%d] vs matrix logarithm" % (a, b))
        _close(H[6 * b:6 * b + 6, 6 * a:6 * a + 6], blk.T, 1e-9, scale, "masked_then_not H[%d,%d] vs matrix logarithm" % (b, a))
