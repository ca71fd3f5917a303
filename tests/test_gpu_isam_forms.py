"""Partial re-factorisation and wildfire back-substitution (fgo_isam2_update) in every launch form.

tests/test_gpu_launch_forms.py holds every kernel form that launch_factor / launch_solve can select to a dense solve -- for the full
sweep.  The same launchers run in two more modes (DESIGN.md "Three sweep modes"): masked (DevPlan::task_dirty set, full grids whose
workgroups look their flag up) and ranged (PartialSweep: per level only the index ranges that cover the dirty tasks), and the backward
kernels run under the wildfire mask.  Here the override sets of the launch-forms module put each form on small graphs, an update
sequence dirties the tree at its newest end, deep inside, inside a bottom-level sub-tree, at two places of one level, at a root only,
and not at all; the census of the LAST update (fgo_debug_launch_census, fused = 2: launch_factor walked with the update's own ranges)
proves that the named form ran on a part of its work items, and the result is held to the full sweep bit for bit and to
numpy.linalg.solve.  The wildfire cut is held to the exact back-substitution (threshold 5e-324) and, at 1e-3, to its own rule, flag by
flag.

FGO_TUNE is read once per process, so each set runs in a fresh child (tests/isam_forms_child.py), one after another, by the protocol
of the launch-forms module (imported: SETS, _run_child, _stops, KAPPA)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import orc_binding as orc  # noqa: E402
from tests.test_gpu_launch_forms import SETS, KAPPA, EPS, ROOT, _run_child, _stops, _Ref, _arrays  # noqa: E402
from tests import isam_forms_child as child  # noqa: E402

CHILD = os.path.join(ROOT, "tests", "isam_forms_child.py")
GRAPH_NAMES = [g[0] for g in child.GRAPHS]
LATER = child.UPDATES[1:]
KEEP_PARTIAL = "isam_full_frac=1e9"            # a 150-pose graph stays in partial mode however much of its tree is dirty

# the forms launch_factor selects: what a partial sweep can run on a part of its items
FACTOR_SIDE = ("k_chol_acc", "k_fwd_combine", "k_panel_tri", "k_panel_rows", "k_chol_leaf", "k_chol_fact", "k_solve_fwd")
NOT_THIS_PATH = ("bwd_ext", "bwd_fused", "chain0", "chain1", "chain2", "chain3", "chain7")     # backward forms only


def _join(*parts):
    return ",".join(p for p in parts if p)


# (set, FGO_TUNE, child modes, factor-side instantiations the set is named for)
FORM_SETS = [(n, _join(t, KEEP_PARTIAL), "forms", [f for f in forms if f.startswith(FACTOR_SIDE)]) for n, t, forms in SETS if n not in NOT_THIS_PATH]
FORM_SETS.append(("ranges_off", _join("isam_ranges=0", KEEP_PARTIAL), "forms", []))
# the relinearisation wave: the default set and three that differ in the accumulate and the triangle form
WAVE_SETS = ["default", "acc1", "g2_8", "tri1"]
FORM_SETS = [(n, t, "forms,wave" if n in WAVE_SETS else m, f) for n, t, m, f in FORM_SETS]
# wildfire: the backward chain stays on (the cut needs it); one set per form select_bwd can pick below the chain
WILD_SETS = [
    ("wf_fused", KEEP_PARTIAL, "wild", ["k_bwd_fused"]),
    ("wf_ext", _join("bwd_fused=0", KEEP_PARTIAL), "wild", ["k_bwd_ext", "k_bwd_tri"]),
    ("wf_bwd1", _join("chain_work=0,no_leaf=1,bwd_h1=1e9", KEEP_PARTIAL), "wild", ["k_solve_bwd<1>"]),
    ("wf_bwd4", _join("no_leaf=1,bwd_h1=0,bwd_h4=1e9", KEEP_PARTIAL), "wild", ["k_solve_bwd<4>"]),
    ("wf_bwd8", _join("no_leaf=1,bwd_h1=0,bwd_h4=0", KEEP_PARTIAL), "wild", ["k_solve_bwd<8>"]),
]
ALL_SETS = FORM_SETS + WILD_SETS
FORM_NAMES = [s[0] for s in FORM_SETS]
WILD_NAMES = [s[0] for s in WILD_SETS]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every override set in a child of its own, one after another; stops starting children after trouble"""
    base = tmp_path_factory.mktemp("isam_forms")
    out, stopped, limit, total = {}, None, 600.0, 0.0      # (the default set also pays the first use of the device)
    for name, tune, modes, _ in ALL_SETS:
        if stopped:
            out[name] = dict(set=name, tune=tune, rc=None, records={}, seconds=0.0, stderr="", not_run_after=stopped)
            continue
        run = _run_child(name, tune, str(base / name), False, limit, child=CHILD, args=["--mode", modes])
        out[name] = run
        total += run["seconds"]
        print("[isam forms] set %-10s rc %s  %.1f s" % (name, run["rc"], run["seconds"]))
        if _stops(run["rc"]):
            stopped = name
        if name == "default":
            limit = max(60.0, 10.0 * run["seconds"])                # sized from the measured time of the default set
    print("[isam forms] %d children, %.1f s" % (len(ALL_SETS), total))
    return out


def _record(runs, set_name, graph, mode="forms"):
    run = runs[set_name]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    rec = run["records"].get("%s/%s" % (mode, graph))
    assert rec is not None, "set %s (rc %s) left no %s record of %s: %s" % (set_name, run["rc"], mode, graph, run["stderr"])
    assert rec["status"] == "ok", rec["status"]
    return rec


def _updates(rec):
    ups = {u["label"]: u for u in rec["updates"]}
    assert list(ups) == child.UPDATES
    return ups


# ---- 1. the child ran clean

@pytest.mark.parametrize("set_name,modes", [(s[0], s[2]) for s in ALL_SETS])
def test_child_ran_clean(runs, set_name, modes):
    """every update after the first is partial on the partial twin and a full sweep on the other; nothing rebuilds the structure after
    the first update has built it"""
    run = runs[set_name]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    assert run["rc"] == 0, (run["rc"], run["stderr"])
    want = ["%s/%s" % (m, g) for m in modes.split(",") for g in (child.WAVE_GRAPHS if m == "wave" else GRAPH_NAMES)]
    assert sorted(run["records"]) == sorted(want)
    print("[isam forms] %s: child %.1f s; %s" % (set_name, run["seconds"], ", ".join("%s %.2f" % (k, run["records"][k].get("seconds", -1)) for k in want)))
    for key in want:
        mode, g = key.split("/")
        rec = _record(runs, set_name, g, mode)
        if mode == "wave":
            assert all(r == 0 for r in rec["p"]["rebuilt"][1:] + rec["f"]["rebuilt"][1:]), (key, rec)
            continue
        for label, up in _updates(rec).items():
            if label == "first":
                continue
            twins = ("f", "p") if mode == "forms" else tuple(k for k, _ in child.WILD)
            assert all(up[k]["rebuilt"] == 0 for k in twins), (key, label, up)
            if mode == "forms":
                assert up["p"]["r3"] >= 0 and up["f"]["r3"] == -1, (key, label, up["p"]["r3"], up["f"]["r3"])
                assert up["p"]["census2"] is not None and up["f"]["census2"] is None       # (FGO_ESTATE after a full sweep)
                assert up["p"]["last"]["sweep"] == (1 if set_name == "ranges_off" else 2) and up["f"]["last"]["sweep"] == 0
            else:
                assert all(up[k]["r3"] >= 0 for k in twins), (key, label, up)


# ---- 2. the form ran partially

def _partial_items(runs, set_name, count):
    """[(graph, update, items in the census of the update, items in the full fused census)] with 0 < items < full"""
    hits = []
    for g in GRAPH_NAMES:
        rec = _record(runs, set_name, g)
        full = count(rec["census_full"])
        for label, up in _updates(rec).items():
            if label != "first" and up["p"]["census2"] is not None:
                part = count(up["p"]["census2"])
                if 0 < part < full:
                    hits.append((g, label, part, full))
    return hits


FORM_CASES = [(s[0], f) for s in FORM_SETS for f in s[3]] + [("acc_long", "long targets"), ("default", "k_panel_rows"), ("default", "k_panel_rows_byc")]
# a form that no update of these graphs can run on a PART of its items, and why (checked: it must indeed not be reached)
NOT_PARTIAL = {
    # launch_factor gives k_fwd_combine the level's whole split table whenever the level has a dirty task (its workgroups go by
    # tcol_task, there is no range for it), and the rows that fwd_split=2 splits sit in levels that every dirty path of these
    # graphs crosses: the form runs under the mask on ALL of its items or, in update (f), on none
    ("fwd_split", "k_fwd_combine"): "not ranged",
}


@pytest.mark.parametrize("set_name,form", FORM_CASES)
def test_the_form_ran_partially(runs, set_name, form):
    """on at least one (graph, update) the census of the update holds the named instantiation with work items > 0 and strictly fewer
    than the full fused census of the same graph.  Accumulate forms count their targets (gather form: short + long) or column groups,
    the long-list role counts on its own, the row kernels count their chunks (+ riders)."""
    if form == "long targets":
        hits = _partial_items(runs, set_name, lambda cz: sum(cz["level_long"]))
    else:
        hits = _partial_items(runs, set_name, lambda cz: cz["forms"][form][2])
    print("[isam forms] %s %s: %s" % (set_name, form, hits[:12]))
    if (set_name, form) in NOT_PARTIAL:
        assert not hits, "NOT_PARTIAL is out of date: %s" % hits[:3]
        whole = [(g, u["label"]) for g in GRAPH_NAMES for rec in [_record(runs, set_name, g)] for u in rec["updates"][1:]
                 if sum(u["p"]["last"]["dirty"]) > 0 and u["p"]["census2"]["forms"][form][2] == rec["census_full"]["forms"][form][2] > 0]
        assert whole, "set %s never ran %s in a partial update at all" % (set_name, form)
    else:
        assert hits, "set %s never ran %s on a part of its work items" % (set_name, form)


# ---- 3. the edge patterns ran

PATTERNS = ["lo_after_first", "hi_before_last", "clean_inside", "riders_only", "fwd_table", "f_nothing_dirty"]
# (set, pattern) that these graphs cannot reach, and why; checked both ways
masked = "the masked sweep launches full grids: there are no ranges"
PATTERN_EXCEPT = {("ranges_off", p): masked for p in ("lo_after_first", "hi_before_last", "clean_inside", "riders_only")}
# (structure_upload.cpp: a panel level's forward work items come from the table only where a row is split, i.e. has >= fwd_split = 32
#  chunks of external entries; no row of these graphs is that long, so the table is reached by the set that lowers fwd_split alone)
PATTERN_EXCEPT.update({(s[0], "fwd_table"): "no row is long enough to be split at the default fwd_split" for s in FORM_SETS if s[0] != "fwd_split"})


def _patterns(runs, set_name):
    seen = {p: [] for p in PATTERNS}
    for g in GRAPH_NAMES:
        rec = _record(runs, set_name, g)
        for label, up in _updates(rec).items():
            if label == "first":
                continue
            la, cz = up["p"]["last"], up["p"]["census2"]
            if label == "f" and up["p"]["r3"] == 0 and sum(la["dirty"]) == 0:
                seen["f_nothing_dirty"].append(g)
            for l, (lo, hi, first, n, dirty) in enumerate(zip(la["lo"], la["hi"], la["first"], la["ntask"], la["dirty"])):
                at = (g, label, l)
                if la["sweep"] == 2 and dirty > 0:
                    assert first <= lo <= hi <= first + n - 1 and dirty <= hi - lo + 1, (at, lo, hi, first, n, dirty)
                    if lo > first: seen["lo_after_first"].append(at)
                    if hi < first + n - 1: seen["hi_before_last"].append(at)
                    if hi - lo + 1 > dirty: seen["clean_inside"].append(at)
                if la["sweep"] == 2 and dirty == 0:
                    assert hi < lo, (at, lo, hi)
                    if cz["level_riders"][l] > 0: seen["riders_only"].append(at)
                if dirty > 0 and la["fwtab"][l] and la["fwd"][l] > 0: seen["fwd_table"].append(at)
    return seen


@pytest.mark.parametrize("set_name", FORM_NAMES)
def test_edge_patterns_ran(runs, set_name):
    """per set, over all graphs: a range that starts after the level's first task, one that ends before its last, one that holds clean
    tasks between dirty ones, a level with no dirty task whose launches still carry riders, a dirty level whose forward work items
    come from the work-item table, and update (f) with nothing dirty"""
    seen = _patterns(runs, set_name)
    print("[isam forms] %s: %s" % (set_name, {p: len(v) for p, v in seen.items()}))
    has_riders = any(sum(_record(runs, set_name, g)["census_full"]["level_riders"]) > 0 for g in GRAPH_NAMES)
    for p in PATTERNS:
        excepted = (set_name, p) in PATTERN_EXCEPT or (p == "riders_only" and not has_riders)
        assert bool(seen[p]) == (not excepted), "set %s, pattern %s: reached at %s, PATTERN_EXCEPT says %s" % (
            set_name, p, seen[p][:3], PATTERN_EXCEPT.get((set_name, p)))


# ---- 4. bit identity

@pytest.mark.parametrize("graph", GRAPH_NAMES)
@pytest.mark.parametrize("set_name", FORM_NAMES)
def test_partial_equals_full_bitwise(runs, set_name, graph):
    """delta of the partial twin equals delta of the full-sweep twin in every entry after every update; after update (f), which adds
    nothing, delta equals the previous update's"""
    a = _arrays(_record(runs, set_name, graph))
    for label in child.UPDATES:
        dp, df = a["delta_p_" + label], a["delta_f_" + label]
        assert np.all(np.isfinite(df))
        diff = int(np.count_nonzero(dp != df))
        assert diff == 0, "%s %s update %s: %d entries differ (largest %.3e)" % (set_name, graph, label, diff, np.abs(dp - df).max())
    for key in ("p", "f"):
        np.testing.assert_array_equal(a["delta_%s_f" % key], a["delta_%s_e" % key])


@pytest.mark.parametrize("graph", GRAPH_NAMES)
def test_masked_sweep_equals_ranged_sweep_bitwise(runs, graph):
    a, b = _arrays(_record(runs, "default", graph)), _arrays(_record(runs, "ranges_off", graph))
    for label in child.UPDATES:
        np.testing.assert_array_equal(a["delta_p_" + label], b["delta_p_" + label], err_msg=label)


# ---- 5. dense reference

class _DenseRef(_Ref):
    """_Ref of the launch-forms module from a dense (H, b): numpy solve, its backward error, the rows of H in long double"""

    def __init__(self, H, b):
        self.b, self.n, self.lam = b, len(b), 0.0
        n = self.n
        self.ref = np.linalg.solve(H, b)
        i, j = np.nonzero(H)
        v = H[i, j]
        d = H[np.arange(n), np.arange(n)]
        off = i != j
        ii = np.concatenate([i[off], np.arange(n)]); jj = np.concatenate([j[off], np.arange(n)]); vv = np.concatenate([v[off], d])
        order = np.lexsort((jj, ii))
        self.ii, self.jj, self.vv = ii[order], jj[order], vv[order].astype(np.longdouble)
        self.starts = np.searchsorted(self.ii, np.arange(n))
        self.norm_A = float(np.add.reduceat(np.abs(self.vv), self.starts).max())
        self.norm_b = float(np.abs(b).max())
        self.eta_ref = self.eta(self.ref)


@pytest.fixture(scope="module")
def refs(runs):
    """per (graph, update): H and b of the oracle at theta with the factors added so far (the relinearisation threshold is 1e9, so theta
    is the initial value of every variable, for every set), solved by numpy; built once, from the default child's prior values"""
    cache = {}

    def get(graph, label):
        if (graph, label) in cache:
            return cache[(graph, label)]
        g = dict((n, m) for n, m, _ in child.GRAPHS)[graph]()
        a = _arrays(_record(runs, "default", graph))
        n = g["n0"]
        ids, means, infos = list(g["priors"]), [g["poses"][p] for p in g["priors"]], [child.SOFT_PRIOR] * len(g["priors"])
        for lab, new_pose, prior_ids in [("first", None, [])] + child.steps_of(graph, g):
            if new_pose is not None:
                n = new_pose + 1
            ids += list(prior_ids); means += list(a["prior_at_" + lab]); infos += [child.WEAK_PRIOR] * len(prior_ids)
            if lab == label:
                break
        m = np.maximum(g["ei"], g["ej"]) < n
        po = orc.Problem(g["poses"][:n], np.zeros(n, np.uint8), g["ei"][m], g["ej"][m], g["meas"][m], g["info"][m])
        po.set_gtsam()
        po.add_priors(np.array(ids, np.int32), np.array(means), np.array(infos))
        H, b = po.dense_system()
        cache[(graph, label)] = _DenseRef(np.asarray(H), np.asarray(b))
        return cache[(graph, label)]
    if runs["default"]["rc"] == 0 and all(runs["default"]["records"].get("forms/" + g, {}).get("status") == "ok" for g in GRAPH_NAMES):
        for g in GRAPH_NAMES:                                  # (built here, so that no case pays for a reference)
            for label in child.UPDATES:
                get(g, label)
    return get


@pytest.mark.parametrize("graph", GRAPH_NAMES)
@pytest.mark.parametrize("set_name", FORM_NAMES)
def test_updates_match_dense(runs, refs, set_name, graph):
    """delta after every update against numpy.linalg.solve(H, b): forward error 1e-9 of the largest entry, backward error within KAPPA
    of the reference's own (tests/test_gpu_launch_forms.py)"""
    a = _arrays(_record(runs, set_name, graph))
    for label in child.UPDATES:
        ref = refs(graph, label)
        bound = KAPPA * max(ref.eta_ref, ref.n * EPS)
        for key in ("p", "f"):
            d = a["delta_%s_%s" % (key, label)].ravel()
            assert len(d) == ref.n and np.all(np.isfinite(d))
            fwd = float(np.abs(d - ref.ref).max() / np.abs(ref.ref).max())
            eta = ref.eta(d)
            print("[isam forms] %s %s %s %s: forward %.3e  eta %.3e  eta_ref %.3e  n eps %.3e  ratio %.3e" % (
                set_name, graph, label, key, fwd, eta, ref.eta_ref, ref.n * EPS, eta / max(ref.eta_ref, ref.n * EPS)))
            np.testing.assert_allclose(d, ref.ref, rtol=0, atol=1e-9 * np.abs(ref.ref).max())
            assert eta <= bound, "%s %s %s %s: backward error %.3e > %.3e" % (set_name, graph, label, key, eta, bound)


# ---- 6. a relinearisation wave

@pytest.mark.parametrize("graph", child.WAVE_GRAPHS)
@pytest.mark.parametrize("set_name", WAVE_SETS)
def test_relinearisation_wave_partial_equals_full_bitwise(runs, set_name, graph):
    """a stretch of 30 poses displaced by 0.12 m, threshold 0.1, ten appended poses: same relinearisation decisions, and poses, theta
    and delta of the partial twin equal the full-sweep twin's bit for bit"""
    rec = _record(runs, set_name, graph, "wave")
    a = _arrays(rec)
    assert rec["p"]["relin"] == rec["f"]["relin"] and sum(rec["p"]["relin"]) > 0, rec
    assert all(r == -1 for r in rec["f"]["r3"]) and all(r >= 0 for r in rec["p"]["r3"][1:]), rec
    for key in ("poses", "theta", "delta"):
        np.testing.assert_array_equal(a[key + "_p"], a[key + "_f"], err_msg=key)


# ---- 7. wildfire

# a backward form that no graph of the list runs below a backward chain, and why (checked: it must indeed not be reached)
BACKWARD_UNREACHED = {
    # k_solve_bwd<1> needs a non-panel level of single-column tasks.  Below panel levels a non-panel level holds light sub-trees of
    # several columns each (the leaf level of the 200-pose graphs; chain_work=0 does not split sub-trees), and the graph whose tasks
    # are single columns has no panels, hence no backward chain and no cut: select_bwd sends wf_bwd1's bottom level to
    # k_solve_bwd<8> as it does for wf_bwd8.  The form under the wildfire mask stays open.
    ("wf_bwd1", "k_solve_bwd<1>"): "no single-column non-panel level below a chain",
}


def _has_chain(rec):
    return bool(rec["census_full"]["chain_on"])


@pytest.mark.parametrize("set_name,forms", [(s[0], s[3]) for s in WILD_SETS])
def test_wildfire_set_runs_its_backward_form_below_the_chain(runs, set_name, forms):
    seen = {}
    for g in GRAPH_NAMES:
        rec = _record(runs, set_name, g, "wild")
        if _has_chain(rec):
            for form, (launches, wgs, items) in rec["census_full"]["forms"].items():
                if items > 0:
                    seen.setdefault(form, []).append(g)
    print("[isam forms] %s: %s" % (set_name, {f: seen.get(f) for f in forms}))
    for form in forms:
        assert (form in seen) == ((set_name, form) not in BACKWARD_UNREACHED), "set %s, %s next to a backward chain: launched %s" % (
            set_name, form, sorted(seen))


@pytest.mark.parametrize("graph", GRAPH_NAMES)
@pytest.mark.parametrize("set_name", WILD_NAMES)
def test_wildfire_smallest_threshold_equals_exact_bitwise(runs, set_name, graph):
    """threshold 5e-324: every change counts, a task left out would have reproduced its old values -- every later update cuts
    (reserved[4] == 1; a graph without panels has no backward chain and never cuts) and poses and delta equal the threshold-0 context"""
    rec = _record(runs, set_name, graph, "wild")
    a = _arrays(rec)
    for label, up in _updates(rec).items():
        want = 1 if (label != "first" and _has_chain(rec)) else 0
        assert up["tiny"]["r4"] == want and up["gtsam"]["r4"] == want and up["exact"]["r4"] == 0, (label, up)
        for key in ("delta", "poses"):
            np.testing.assert_array_equal(a["%s_tiny_%s" % (key, label)], a["%s_exact_%s" % (key, label)], err_msg="%s %s" % (key, label))


def _cut_rule(rec, a, thr_key, thr):
    """per cut update: (label, tasks left out, variables of tasks left out) after asserting the rule of the cut exactly"""
    out, prev = [], None
    for label, up in _updates(rec).items():
        delta = a["delta_%s_%s" % (thr_key, label)]
        if up[thr_key]["r4"]:
            run, task, chg = (a["%s_%s_%s" % (f, thr_key, label)] for f in ("task_run", "var_task", "var_chg"))
            before = np.zeros_like(delta)
            before[:len(prev)] = prev                             # (a variable added by this update had delta 0)
            assert np.all(task >= 0)
            ran = run[task] != 0
            np.testing.assert_array_equal(delta[~ran], before[~ran], err_msg="update %s: a task that was left out moved" % label)
            moved = ran & (np.abs(delta - before) >= thr).any(axis=1)
            np.testing.assert_array_equal(chg != 0, moved, err_msg="update %s: chg" % label)
            out.append((label, run, task, a["task_level_%s_%s" % (thr_key, label)], up[thr_key]["chain_low"]))
        prev = delta
    return out


@pytest.mark.parametrize("graph", GRAPH_NAMES)
@pytest.mark.parametrize("set_name", WILD_NAMES)
def test_wildfire_cut_follows_its_rule_exactly(runs, set_name, graph):
    """threshold 1e-3, no tolerance: the variables of a task with run == 0 keep the previous update's delta bit for bit; chg of a
    variable is 1 exactly when its task ran and a component of its delta moved by >= 1e-3; some task is left out on some update.
    Two components: an update that touches only the second leaves out every task of the first below the backward chain (the levels
    of the chain are always solved)."""
    rec = _record(runs, set_name, graph, "wild")
    a = _arrays(rec)
    cuts = _cut_rule(rec, a, "gtsam", 1e-3)
    _cut_rule(rec, a, "tiny", 5e-324)
    if not _has_chain(rec):
        assert not cuts
        return
    assert [c[0] for c in cuts] == LATER
    left_out = {label: int(np.count_nonzero(run == 0)) for label, run, _, _, _ in cuts}
    print("[isam forms] %s %s: tasks left out per update %s" % (set_name, graph, left_out))
    assert max(left_out.values()) > 0
    if graph == "twocomp200":
        ups, checked = _updates(rec), 0
        for label, run, task, level, chain_low in cuts:
            touched = ups[label]["prior_ids"] + ([ups[label]["new_pose"]] if ups[label]["new_pose"] is not None else [])
            if touched and min(touched) >= 200:
                first = np.unique(task[:200])
                assert not np.intersect1d(first, task[200:]).size              # (no task holds variables of both components)
                below = first[level[first] < chain_low]
                assert below.size > 0 and not run[below].any(), (label, below[run[below] != 0])
                checked += 1
        assert checked >= 2
