"""Every instantiation that launch_factor / launch_fwd_level / launch_solve can select, pinned to a dense solve.

The launch selection (launch_select.cpp select_*) goes by thresholds on level width that were tuned on 100k- and 1M-pose graphs; graphs
small enough for a dense reference reach a handful of the forms on their own.  Here FGO_TUNE override sets move the thresholds so
that each form runs on small graphs whose panels have every width 1..16 and whose lists end in ragged remainders, the launch
census (fgo_debug_launch_census) proves that the form a set is named for really ran, and both the stand-alone solve
(fgo_solve_step) and the fused one (fgo_debug_solve_fused: the forward solve riding in the factor sweep, as an LM trial runs it)
are held to numpy.linalg.solve: forward error 1e-9 of the largest entry (the bound of test_damped_solve_matches_dense) and a
backward error within KAPPA of the reference's own.

FGO_TUNE is read once per process, so each set runs in a fresh child (tests/launch_forms_child.py), one after another; after a
child that ends with a signal, an abort, a device error or its timeout no further child is started and every remaining case fails
as "not run after <set>"."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "launch_forms_child.py")

SOLVE_GRAPHS = ["synth150_w1", "synth400_w1", "synth400_w200", "synth650_w50", "synth200_leaf", "star200", "star3000", "complete70",
                "complete70_w1_nopanels", "complete130_nopanels", "complete250_nopanels", "synth150_w1_nopanels"]
NEGDEF_GRAPHS = ["negdef_w1", "negdef_default", "negdef_nopanels", "negdef_star200", "negdef_star3000",
                 "negdef_complete70_w1_nopanels", "negdef_synth25", "negdef_complete130_nopanels"]

BIG = "1e9"
# (chain_work=0: no chains of columns in one task, so the complete graphs become single-column tasks of every height up to 249)
W1 = "chain_work=0,no_leaf=1,fact_h1_2=%s,fwd_h1=%s,bwd_h1=%s" % (BIG, BIG, BIG)
# (set, FGO_TUNE, instantiations the set is named for: each must appear in the census of at least one graph)
SETS = [
    ("default", "", ["k_chol_acc<8>", "k_panel_tri<16>", "k_bwd_chain", "k_bwd_fused", "k_chol_leaf<4>", "k_fwd_ext", "k_fwd_tri"]),
    ("acc4", "acc_narrow=0,acc_mid2=1e9", ["k_chol_acc<4>"]),
    ("acc2", "acc_narrow=0,acc_mid2=0,acc_wide2=1e9", ["k_chol_acc<2>"]),
    ("acc1", "acc_narrow=0,acc_mid2=0,acc_wide2=0", ["k_chol_acc<1>"]),
    ("acc2_wide", "acc_narrow=0,acc_mid2=0,acc_wide2=0,acc_wide_split=2", ["k_chol_acc<2>"]),
    ("g2_8", "acc2_min=0,acc2_narrow=1e9", ["k_chol_acc2<8>"]),
    ("g2_4", "acc2_min=0,acc2_narrow=0,acc2_mid=1e9", ["k_chol_acc2<4>"]),
    ("g2_1", "acc2_min=0,acc2_narrow=0,acc2_mid=0", ["k_chol_acc2<1>"]),
    # (no level of these graphs has the 8 000 groups that switch the column-group form on: the set must change nothing at all)
    ("g2_off", "acc_v1=1", ["k_chol_acc<8>"]),
    ("g2_1_plain", "acc2_min=0,acc2_narrow=0,acc2_mid=0,ride=0,acc_long=1e9", ["k_chol_acc2<1>"]),
    ("acc1_plain", "acc_v1=1,acc_narrow=0,acc_mid2=0,acc_wide2=0,ride=0,acc_long=1e9", ["k_chol_acc<1>"]),
    ("acc_long", "acc_long=4", ["k_chol_acc<8>"]),
    ("ride_off", "ride=0", ["k_panel_tri<16>"]),
    ("ride_all", "ride_min=1,ride_min2=1", ["k_panel_tri<16>"]),
    ("tri8", "tri_wide=0,tri1=0", ["k_panel_tri<8>"]),
    ("tri1", "tri_wide=0,tri1_min=0", ["k_panel_tri1"]),
    ("rows_plain", "rows_byc=0", ["k_panel_rows"]),
    ("rows_byc", "rows_byc=1e9", ["k_panel_rows_byc"]),
    ("no_leaf", "no_leaf=1", ["k_chol_fact<4,3>"]),
    ("fwd_split", "fwd_split=2", ["k_fwd_combine"]),
    ("bwd_ext", "bwd_chain=0,bwd_fused=0", ["k_bwd_ext", "k_bwd_tri"]),
    ("bwd_fused", "bwd_chain=0", ["k_bwd_fused"]),
    ("chain0", "bwd_chain_mode=0", ["k_bwd_chain"]),
    ("chain1", "bwd_chain_mode=1", ["k_bwd_chain"]),
    ("chain2", "bwd_chain_mode=2", ["k_bwd_chain"]),
    ("chain3", "bwd_chain_mode=3", ["k_bwd_chain"]),
    ("chain7", "bwd_chain_mode=7", ["k_bwd_chain"]),
    ("w1_2", W1, ["k_chol_fact<1,2>", "k_solve_fwd<1>", "k_solve_bwd<1>"]),
    ("w1_3", "chain_work=0,no_leaf=1,fact_h1_2=0,fact_h1_3=1e9,fwd_h1=1e9,bwd_h1=1e9", ["k_chol_fact<1,3>"]),
    ("w4", "no_leaf=1,fact_h1_2=0,fact_h1_3=0,fact_h4=1e9,fwd_h1=0,fwd_h4=1e9,bwd_h1=0,bwd_h4=1e9",
     ["k_chol_fact<4,3>", "k_solve_fwd<4>", "k_solve_bwd<4>"]),
    ("w8", "no_leaf=1,fact_h1_2=0,fact_h1_3=0,fact_h4=0,fact_h8=1e9,fwd_h1=0,fwd_h4=0,bwd_h1=0,bwd_h4=0",
     ["k_chol_fact<8,3>", "k_solve_fwd<16>", "k_solve_bwd<8>"]),
    ("w16", "no_leaf=1,fact_h1_2=0,fact_h1_3=0,fact_h4=0,fact_h8=0,fwd_h1=0,fwd_h4=0,bwd_h1=0,bwd_h4=0",
     ["k_chol_fact<16,2>", "k_solve_fwd<16>", "k_solve_bwd<8>"]),
]
SET_NAMES = [s[0] for s in SETS]
# sets whose results the code claims to be the same to the bit (fgo_internal.hpp: the column-group lists apply a target's updates in
# the order of the gather lists -- one wave per group against one wave per ten targets, no riders and no long-list role, which
# sum a list in pieces; kernels_factor.hip: the by-chunk rows table only moves the index loads; kernels_solve.hip: bwd_chain_mode only changes how the
# chain's workgroups wait for and publish x)
BIT_IDENTICAL = [
    ("g2_1_plain", "acc1_plain"),
    ("default", "g2_off"),
    ("rows_plain", "rows_byc"),
    ("default", "chain0"), ("default", "chain1"), ("default", "chain2"), ("default", "chain3"), ("default", "chain7"),
]
FACTOR_FORMS = ["k_panel_tri<16>", "k_panel_tri<8>", "k_panel_tri1", "k_chol_leaf<4>", "k_chol_fact<1,2>", "k_chol_fact<1,3>",
                "k_chol_fact<4,3>", "k_chol_fact<8,3>", "k_chol_fact<16,2>"]

# Backward error eta(d) = |(H + lambda I) d - b|_inf / (|H + lambda I|_inf |d|_inf + |b|_inf), residual in long double, is held to
# KAPPA * max(eta(numpy.linalg.solve), n eps), eps = 2^-53 (n eps: the backward-error scale of a Cholesky solve of dimension n).
# KAPPA = 8 x the largest ratio the DEFAULT set shows over all graphs (the margin covers the other summation orders of the split
# forms); one number for all sets.  Observed ratios and the choice: profiles/NOTES.md "Launch forms against a dense solve".
KAPPA = 8.0 * 1.113e-3
EPS = 2.0 ** -53


def _stops(rc):
    """the stop rule: after a child that ended with a signal, an abort, a segmentation fault, a device error or its timeout no further
    child is started"""
    return rc == "timeout" or rc < 0 or rc in (3, 124, 134, 137, 139)        # (124 / 137: ended by a `timeout -k` in front of the child)


def _run_child(name, tune, out_dir, dense, timeout, child=CHILD, args=(), prefix=()):
    env = dict(os.environ)
    if tune:
        env["FGO_TUNE"] = tune
    else:
        env.pop("FGO_TUNE", None)
    cmd = list(prefix) + [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [child, "--out", out_dir] + (["--dense"] if dense else []) + list(args)
    t0 = time.time()
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
        rc, out, err = r.returncode, r.stdout, r.stderr
    except subprocess.TimeoutExpired as e:
        rc, out, err = "timeout", (e.stdout or b"").decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or ""), ""
    recs = {}
    for line in out.splitlines():
        if line.startswith("RECORD "):
            rec = json.loads(line[7:])
            recs[rec["graph"]] = rec
    return dict(set=name, tune=tune, rc=rc, records=recs, seconds=time.time() - t0, stderr=err[-2000:], not_run_after=None)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every override set in a child of its own, one after another; stops starting children after trouble"""
    base = tmp_path_factory.mktemp("launch_forms")
    out, stopped, limit = {}, None, 600.0          # (the default set also pays the first use of the device)
    for name, tune, _ in SETS:
        if stopped:
            out[name] = dict(set=name, tune=tune, rc=None, records={}, seconds=0.0, stderr="", not_run_after=stopped)
            continue
        run = _run_child(name, tune, str(base / name), name == "default", limit)
        out[name] = run
        print("[launch forms] set %-10s rc %s  %.1f s" % (name, run["rc"], run["seconds"]))
        if _stops(run["rc"]):
            stopped = name
        if name == "default":
            limit = max(60.0, 10.0 * run["seconds"])                # sized from the measured time of the default set
    return out


def _arrays(rec):
    with np.load(rec["npz"]) as z:
        return {k: z[k] for k in z.files}


def _record(runs, set_name, graph):
    run = runs[set_name]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    rec = run["records"].get(graph)
    assert rec is not None, "set %s (rc %s) left no record of %s: %s" % (set_name, run["rc"], graph, run["stderr"])
    assert rec["status"] == "ok", rec["status"]
    return rec


class _Ref:
    """dense reference of one graph (from the default set's H, b): numpy solve, its backward error, and H + lambda I as long-double
    rows for the residuals"""

    def __init__(self, rec):
        a = _arrays(rec)
        self.b = a["b_dense"]
        self.b_sorted = a["b_sorted"]
        self.n = n = len(self.b)
        self.lam = rec["lam"]
        i, j, v = a["H_i"].astype(np.int64), a["H_j"].astype(np.int64), a["H_v"]
        A = np.zeros((n, n))
        A[i, j] = v
        assert self.lam == 1e-5 * np.abs(np.diag(A)).max()
        A[np.arange(n), np.arange(n)] += self.lam
        self.ref = np.linalg.solve(A, self.b)
        # rows of A in long double (every row has its diagonal entry): residuals by segment sums over the non-zeros
        d = A[np.arange(n), np.arange(n)]
        del A
        off = i != j
        ii = np.concatenate([i[off], np.arange(n)]); jj = np.concatenate([j[off], np.arange(n)]); vv = np.concatenate([v[off], d])
        order = np.lexsort((jj, ii))
        self.ii, self.jj, self.vv = ii[order], jj[order], vv[order].astype(np.longdouble)
        self.starts = np.searchsorted(self.ii, np.arange(n))
        self.norm_A = float(np.add.reduceat(np.abs(self.vv), self.starts).max())
        self.norm_b = float(np.abs(self.b).max())
        self.eta_ref = self.eta(self.ref)

    def eta(self, d):
        r = np.add.reduceat(self.vv * d.astype(np.longdouble)[self.jj], self.starts) - self.b.astype(np.longdouble)
        return float(np.abs(r).max()) / (self.norm_A * float(np.abs(d).max()) + self.norm_b)


@pytest.fixture(scope="module")
def refs(runs):
    cache = {}

    def get(graph):
        if graph not in cache:
            cache[graph] = _Ref(_record(runs, "default", graph))
        return cache[graph]
    return get


def _forms(rec):
    seen = {}
    for key in ("census_plain", "census_fused"):
        # (work items: for an accumulate form its targets / groups, not the forward-role or padding workgroups of its launch)
        for form, (launches, wgs, items) in rec[key]["forms"].items():
            if items > 0:
                assert launches > 0 and wgs >= ((items + 9) // 10 if form.startswith("k_chol_acc<") else items)
                seen[form] = seen.get(form, 0) + items
    return seen


@pytest.mark.parametrize("set_name", SET_NAMES)
def test_child_ran_clean(runs, set_name):
    run = runs[set_name]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    assert run["rc"] == 0, (run["rc"], run["stderr"])
    assert sorted(run["records"]) == sorted(SOLVE_GRAPHS + NEGDEF_GRAPHS)
    print("[launch forms] %s: child %.1f s; per graph %s" % (set_name, run["seconds"],
          ", ".join("%s %.2f" % (g, run["records"][g].get("seconds", -1)) for g in SOLVE_GRAPHS + NEGDEF_GRAPHS)))


@pytest.mark.parametrize("set_name,expect", [(s[0], s[2]) for s in SETS])
def test_the_form_ran(runs, set_name, expect):
    """the census holds the instantiation the set is named for, with workgroups, on at least one graph"""
    seen = {}
    for g in SOLVE_GRAPHS:
        for form, wgs in _forms(_record(runs, set_name, g)).items():
            seen.setdefault(form, []).append(g)
    print("[launch forms] %s: %s" % (set_name, {f: len(v) for f, v in sorted(seen.items())}))
    print("[launch forms] %s: %s" % (set_name, {f: seen.get(f) for f in expect}))
    for form in expect:
        assert form in seen, "set %s never launched %s (launched: %s)" % (set_name, form, sorted(seen))


def test_roles_ran(runs):
    """the long-list role of the accumulate and the rider work items: on where the sets say so, off where they say so"""
    def total(set_name, key):
        return sum(sum(_record(runs, set_name, g)["census_fused"][key]) for g in SOLVE_GRAPHS)
    assert total("acc_long", "level_long") > total("default", "level_long") >= 0
    assert total("acc_long", "level_long") > 0
    assert total("ride_off", "level_riders") == 0
    assert total("ride_all", "level_riders") > total("default", "level_riders")
    assert not any(_record(runs, "bwd_ext", g)["census_fused"]["chain_on"] for g in SOLVE_GRAPHS)
    assert any(_record(runs, "default", g)["census_fused"]["chain_on"] for g in SOLVE_GRAPHS)
    for k in (0, 1, 2, 3, 7):
        assert all(_record(runs, "chain%d" % k, g)["census_fused"]["chain_mode"] == k for g in SOLVE_GRAPHS)


@pytest.mark.parametrize("graph", SOLVE_GRAPHS)
@pytest.mark.parametrize("set_name", SET_NAMES)
def test_solves_match_dense(runs, refs, set_name, graph):
    """stand-alone and fused delta against numpy.linalg.solve(H + lambda I, b): forward error 1e-9 of the largest entry, backward
    error within KAPPA of the reference's"""
    rec = _record(runs, set_name, graph)
    ref = refs(graph)
    a = _arrays(rec)
    assert rec["lam"] == ref.lam                                    # the same system as the reference's: linearisation does not
    np.testing.assert_array_equal(a["b_sorted"], ref.b_sorted)      # depend on the launch selection
    bound = KAPPA * max(ref.eta_ref, ref.n * EPS)
    for key in ("d_step", "d_fused"):
        d = a[key]
        assert np.all(np.isfinite(d))
        fwd = float(np.abs(d - ref.ref).max() / np.abs(ref.ref).max())
        eta = ref.eta(d)
        print("[launch forms] %s %s %s: forward %.3e  eta %.3e  eta_ref %.3e  n eps %.3e  ratio %.3f" % (
            set_name, graph, key, fwd, eta, ref.eta_ref, ref.n * EPS, eta / max(ref.eta_ref, ref.n * EPS)))
        np.testing.assert_allclose(d, ref.ref, rtol=0, atol=1e-9 * np.abs(ref.ref).max())
        assert eta <= bound, "%s %s %s: backward error %.3e > %.3e" % (set_name, graph, key, eta, bound)


@pytest.mark.parametrize("a,b", BIT_IDENTICAL)
def test_bit_identity_where_the_code_claims_it(runs, a, b):
    for g in SOLVE_GRAPHS:
        xa, xb = _arrays(_record(runs, a, g)), _arrays(_record(runs, b, g))
        for key in ("d_step", "d_fused"):
            diff = int(np.count_nonzero(xa[key] != xb[key]))
            assert diff == 0, "%s vs %s, %s %s: %d entries differ (largest %.3e)" % (a, b, g, key, diff, np.abs(xa[key] - xb[key]).max())
    if a.startswith("g2_"):        # the comparison is between the two forms: one side ran the column groups, the other none
        fa = [f for g in SOLVE_GRAPHS for f in _forms(_record(runs, a, g))]
        fb = [f for g in SOLVE_GRAPHS for f in _forms(_record(runs, b, g))]
        assert any(f.startswith("k_chol_acc2") for f in fa) and not any(f.startswith("k_chol_acc2") for f in fb)


@pytest.mark.parametrize("set_name", SET_NAMES)
def test_not_positive_definite_is_reported_from_every_form(runs, set_name):
    """the negative-definite graph of test_not_positive_definite_is_reported raises whatever forms factor it"""
    for g in NEGDEF_GRAPHS:
        rec = _record(runs, set_name, g)
        assert rec["raised_step"] and rec["raised_fused"], (set_name, g, rec)


# a (set, graph) per factor form in which it is the ONLY form that factors: on a wholly negated graph the first level reports and
# the NaNs it leaves make every later form report too, so a form proves that it raises the flag itself only where it is alone
SOLE_FACTOR_FORM = [
    ("k_panel_tri<16>", "default", "negdef_w1"), ("k_panel_tri<8>", "tri8", "negdef_w1"), ("k_panel_tri1", "tri1", "negdef_w1"),
    ("k_chol_leaf<4>", "default", "negdef_synth25"),
    ("k_chol_fact<1,2>", "w1_2", "negdef_complete70_w1_nopanels"), ("k_chol_fact<1,3>", "w1_3", "negdef_complete70_w1_nopanels"),
    ("k_chol_fact<4,3>", "w4", "negdef_nopanels"), ("k_chol_fact<8,3>", "w8", "negdef_nopanels"),
    ("k_chol_fact<16,2>", "w16", "negdef_nopanels"),
]


@pytest.mark.parametrize("form,set_name,graph", SOLE_FACTOR_FORM)
def test_failure_is_reported_by_the_form_itself(runs, form, set_name, graph):
    rec = _record(runs, set_name, graph)
    assert sorted(f for f in _forms(rec) if f in FACTOR_FORMS) == [form]
    assert rec["raised_step"] and rec["raised_fused"], rec


def test_every_factor_form_is_covered():
    assert sorted(f for f, _, _ in SOLE_FACTOR_FORM) == sorted(FACTOR_FORMS)


def test_every_selectable_instantiation_was_seen(runs):
    """the enumeration comes from the census itself: an instantiation added to the launchers fails here until a set reaches it"""
    names = list(_record(runs, "default", SOLVE_GRAPHS[0])["census_fused"]["forms"])
    assert len(names) >= 31                                        # (LF_COUNT when this test was written)
    seen = set()
    for name in SET_NAMES:
        for g in SOLVE_GRAPHS:
            seen.update(_forms(_record(runs, name, g)))
    assert [f for f in names if f not in seen] == []
    import resource
    print("[launch forms] peak resident memory: parent %.0f MB, children %s" % (
        resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0,
        {n: "%.0f MB" % max(r.get("maxrss_mb", 0) for r in runs[n]["records"].values()) for n in ("default", "acc4")}))
