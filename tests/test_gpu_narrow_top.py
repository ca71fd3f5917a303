"""The kernels of the narrow top of the elimination tree -- k_bwd_chain, k_bwd_fused, k_panel_tri<16>, k_panel_tri<8> -- at the
shapes where their code takes another path, pinned to a dense solve the way tests/test_gpu_launch_forms.py does it.

The graphs (tests/narrow_top_child.py) are small complete graphs with FGO_TASK_WORK=1: N free poses are eliminated as one chain of
columns, cut from the bottom into P = ceil(N / 16) panels of m = 16 columns, one panel per level, the root panel taking the
remaining m = N - 16 (P - 1) columns.  Panel p (p = 0 at the bottom) has N - 16 (p + 1) off-triangle block rows, the root none.
Levels 1 .. P - 1 form the backward chain (k_bwd_chain), level 0 runs k_bwd_fused; with bwd_chain=0 every level runs k_bwd_fused.

  complete209  N = 208  m 16 x 13            rows 192, 176, 160, 144, ... 16, 0   (160: the 16 waves x 10 rows of ONE chunk round are
                                              exactly full; 176 / 192: a second round for waves 0 / 0..3)
  complete210  N = 209  m 16 x 13, root 1    rows 193, 177, 161, 145, ... 17, 1, 0   (161: one row in the second round; 1: one lane group)
  complete35   N = 34   m 16, 16, root 2     rows 18, 2, 0
  complete36   N = 35   m 16, 16, root 3     rows 19, 3, 0
  complete40   N = 39   m 16, 16, root 7     rows 23, 7, 0
  complete41   N = 40   m 16, 16, root 8     rows 24, 8, 0     (6 m = 48: exactly three 16-wide tiles; 6, 12, 18, 42: a padded last tile)
  synth150_w1  (of test_gpu_launch_forms) panels of every width 1 .. 16 with rows below them: the complete graphs have their short
               panel at the root, where the row phase has nothing to do

The root panels (0 rows) and the panels with 1, 2, 3, 7, 8 rows use one lane-group chunk of wave 0 only.  The structure is asserted,
not assumed: the number of levels and the census items of the backward kernels must be P, P - 1 and 1.

Checks per override set (a fresh child each, under its own time limit; after a child that ends abnormally none is started):
stand-alone and fused delta against numpy.linalg.solve(H + lambda I, b) with the bounds of test_gpu_launch_forms (forward 1e-9 of
the largest entry, backward error within its KAPPA); bit identity of the default with bwd_chain=0 and bwd_chain_mode=0 / 7; the
census proves which kernels ran."""
import os

import numpy as np
import pytest

from tests.test_gpu_launch_forms import KAPPA, EPS, ROOT, _run_child, _stops, _Ref, _arrays, _forms
from tests.narrow_top_child import COMPLETE

pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "narrow_top_child.py")
CHILD_SECONDS = 180            # (the first child also pays the first use of the device; a child takes 2-3 s)

GRAPHS = ["complete%d" % n for n in COMPLETE] + ["synth150_w1"]
SETS = [
    ("default", ""),
    ("bwd_fused", "bwd_chain=0"),
    ("chain0", "bwd_chain_mode=0"),
    ("chain7", "bwd_chain_mode=7"),
    ("tri8", "tri_wide=0,tri1=0"),
]
SET_NAMES = [s[0] for s in SETS]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("narrow_top")
    out, stopped = {}, None
    for name, tune in SETS:
        if stopped:
            out[name] = dict(set=name, tune=tune, rc=None, records={}, seconds=0.0, stderr="", not_run_after=stopped)
            continue
        run = _run_child(name, tune, str(base / name), name == "default", CHILD_SECONDS + 30, child=CHILD,
                         prefix=("timeout", "-k", "10", str(CHILD_SECONDS)))
        out[name] = run
        print("[narrow top] set %-10s rc %s  %.1f s" % (name, run["rc"], run["seconds"]))
        if _stops(run["rc"]):
            stopped = name
    return out


def _record(runs, set_name, graph):
    run = runs[set_name]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    rec = run["records"].get(graph)
    assert rec is not None, "set %s (rc %s) left no record of %s: %s" % (set_name, run["rc"], graph, run["stderr"])
    assert rec["status"] == "ok", rec["status"]
    return rec


@pytest.fixture(scope="module")
def refs(runs):
    cache = {}

    def get(graph):
        if graph not in cache:
            cache[graph] = _Ref(_record(runs, "default", graph))
        return cache[graph]
    return get


@pytest.mark.parametrize("set_name", SET_NAMES)
def test_child_ran_clean(runs, set_name):
    run = runs[set_name]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    assert run["rc"] == 0, (run["rc"], run["stderr"])
    assert sorted(run["records"]) == sorted(GRAPHS)
    print("[narrow top] %s: child %.1f s; per graph %s" % (set_name, run["seconds"],
          ", ".join("%s %.2f" % (g, run["records"][g].get("seconds", -1)) for g in GRAPHS)))


def _items(rec, key, form):
    return rec[key]["forms"][form][2]


@pytest.mark.parametrize("n", COMPLETE)
def test_the_graphs_have_the_panels_the_docstring_states(runs, n):
    """one panel per level, P = ceil(N / 16) of them; the chain holds levels 1 .. P - 1, level 0 is a k_bwd_fused launch"""
    g, P = "complete%d" % n, (n - 1 + 15) // 16
    for set_name in SET_NAMES:
        rec = _record(runs, set_name, g)
        assert rec["n_levels"] == P, (set_name, g, rec["n_levels"])
        for key in ("census_plain", "census_fused"):
            chain, fused = _items(rec, key, "k_bwd_chain"), _items(rec, key, "k_bwd_fused")
            assert (chain, fused) == ((0, P) if set_name == "bwd_fused" else (P - 1, 1)), (set_name, g, key, chain, fused)
            assert rec[key]["chain_on"] == (set_name != "bwd_fused")
            tri16, tri8 = _items(rec, key, "k_panel_tri<16>"), _items(rec, key, "k_panel_tri<8>")
            assert (tri16 == 0 and tri8 == P) if set_name == "tri8" else (tri16 >= P and tri8 == 0), (set_name, g, key, tri16, tri8)
            assert _items(rec, key, "k_panel_tri1") == 0 and _items(rec, key, "k_chol_leaf<4>") == 0
    assert _record(runs, "chain0", g)["census_fused"]["chain_mode"] == 0 and _record(runs, "chain7", g)["census_fused"]["chain_mode"] == 7


def test_the_forms_ran(runs):
    for set_name, forms in (("default", ["k_bwd_chain", "k_bwd_fused", "k_panel_tri<16>"]), ("bwd_fused", ["k_bwd_fused"]),
                            ("chain0", ["k_bwd_chain"]), ("chain7", ["k_bwd_chain"]), ("tri8", ["k_panel_tri<8>", "k_bwd_chain"])):
        for g in GRAPHS:
            seen = _forms(_record(runs, set_name, g))
            for form in forms:
                assert form in seen, "set %s, %s never launched %s (launched: %s)" % (set_name, g, form, sorted(seen))


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("set_name", SET_NAMES)
def test_solves_match_dense(runs, refs, set_name, graph):
    """stand-alone and fused delta against numpy.linalg.solve(H + lambda I, b): forward error 1e-9 of the largest entry, backward
    error within KAPPA of the reference's (the bounds of test_gpu_launch_forms)"""
    rec = _record(runs, set_name, graph)
    ref = refs(graph)
    a = _arrays(rec)
    assert rec["lam"] == ref.lam
    np.testing.assert_array_equal(a["b_sorted"], ref.b_sorted)
    bound = KAPPA * max(ref.eta_ref, ref.n * EPS)
    for key in ("d_step", "d_fused"):
        d = a[key]
        assert np.all(np.isfinite(d))
        fwd = float(np.abs(d - ref.ref).max() / np.abs(ref.ref).max())
        eta = ref.eta(d)
        print("[narrow top] %s %s %s: forward %.3e  eta %.3e  eta_ref %.3e  n eps %.3e  ratio %.3f" % (
            set_name, graph, key, fwd, eta, ref.eta_ref, ref.n * EPS, eta / max(ref.eta_ref, ref.n * EPS)))
        np.testing.assert_allclose(d, ref.ref, rtol=0, atol=1e-9 * np.abs(ref.ref).max())
        assert eta <= bound, "%s %s %s: backward error %.3e > %.3e" % (set_name, graph, key, eta, bound)


@pytest.mark.parametrize("other", ["bwd_fused", "chain0", "chain7"])
def test_bit_identity_of_the_backward_forms(runs, other):
    """k_bwd_chain in its wait / publish modes and k_bwd_fused share their arithmetic: the same delta to the bit"""
    for g in GRAPHS:
        xa, xb = _arrays(_record(runs, "default", g)), _arrays(_record(runs, other, g))
        for key in ("d_step", "d_fused"):
            diff = int(np.count_nonzero(xa[key] != xb[key]))
            assert diff == 0, "default vs %s, %s %s: %d entries differ (largest %.3e)" % (other, g, key, diff, np.abs(xa[key] - xb[key]).max())
