"""k_panel_tri1 (one wave per panel, two waves per SIMD) as the ONLY triangle form, on panels of every width, pinned to a dense solve
the way tests/test_gpu_launch_forms.py does it.

The child (tests/tri1_two_waves_child.py) runs with FGO_TUNE="tri_wide=0,tri1_min=0" and FGO_TASK_WORK=1: no leaf level, every level a
panel level, every panel through k_panel_tri1.  The census (fgo_debug_launch_census) must show as many k_panel_tri1 work items as the
graph has panels and none of k_panel_tri<16> / k_panel_tri<8>.

Graphs.  Panel widths m of the two synthetic graphs, as `tools/symstats <poses> 5 4 64 1 1000000000` prints them with
FGO_SYNTH_SEED=<seed> (all levels; counts for m = 1 .. 16):

  synth300_w1  synth_manhattan3d(300, 5, 4, seed 3)  21 panels, 5 levels   0 0 0 1 0 1 0 0 1 0 0 1 1 0 1 15
  synth500_w1  synth_manhattan3d(500, 5, 4, seed 6)  43 panels, 7 levels   1 2 3 0 3 1 4 1 0 1 1 1 1 1 0 23
  together                                                                 1 2 3 1 3 2 4 1 1 1 1 2 2 1 1 38

so every width 1 .. 16 occurs with block rows below the panel (test_the_graphs_hold_every_panel_width re-derives the histograms on
the CPU).  What the widths reach in the kernel: m = 1 no MFMA at all; 6 m no multiple of 16 (all but m = 8, 16) a padded last tile
row; m >= 11 rows 64 .. 95 on lanes 0 .. 31; m = 16 no padding; every m >= 3 a diagonal block that straddles two tile columns
(block column 2: scalar columns 12 .. 17).  The complete graphs of tests/test_gpu_narrow_top.py (one chain of 16-column panels, one
panel per level) add root panels of 16, 1, 2, 3, 7 and 8 columns without rows and panels with up to 193 rows below them.

Checks: stand-alone (fgo_solve_step) and fused (the step of an LM trial) delta of a damped solve, lambda = 1e-5 max|diag H|, against
numpy.linalg.solve(H + lambda I, b): forward error within 1e-9 of the largest entry, backward error within KAPPA of the reference's
own (both bounds are those of test_gpu_launch_forms); the wholly negated graph raises with k_panel_tri1 as the only factor form; a
second child gives the same steps to the bit.  One child at a time under its own time limit; after a child that ends with a signal,
a device error or its timeout none is started."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_launch_forms import KAPPA, EPS, ROOT, FACTOR_FORMS, _run_child, _stops, _Ref, _arrays, _forms
from tests.tri1_two_waves_child import COMPLETE, SYNTH
from tests.util import build_symstats

gpu = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "tri1_two_waves_child.py")
CHILD_SECONDS = 180            # (the first child also pays the first use of the device; a child takes a few seconds)
TUNE = "tri_wide=0,tri1_min=0"

WIDTHS = {"synth300_w1": [0, 0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 1, 0, 1, 15],
          "synth500_w1": [1, 2, 3, 0, 3, 1, 4, 1, 0, 1, 1, 1, 1, 1, 0, 23]}
PANELS = {g: sum(h) for g, h in WIDTHS.items()}
PANELS.update({"complete%d" % n: (n - 1 + 15) // 16 for n in COMPLETE})
GRAPHS = list(WIDTHS) + ["complete%d" % n for n in COMPLETE]
RUNS = ["first", "second"]


def test_the_graphs_hold_every_panel_width():
    """CPU: the structure phase of the two synthetic graphs (tools/symstats, task work 1) has the panel widths the docstring states"""
    exe = build_symstats()
    total = [0] * 16
    for g, (n, lookback, loops, seed) in SYNTH.items():
        out = subprocess.run([exe, str(n), str(lookback), str(loops), "64", "1", "1000000000"], capture_output=True, text=True,
                             env=dict(os.environ, FGO_SYNTH_SEED=str(seed)), timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = [[int(v) for v in l.split(":")[1].split()] for l in out.stdout.splitlines() if "panel widths:" in l]
        summary = [l for l in out.stdout.splitlines() if l.startswith("panels ")][0]
        n_panels, n_levels = int(summary.split()[1].rstrip(",")), int(summary.split("panel levels")[1].split()[0])
        assert len(rows) == n_levels and int(summary.split(" of ")[1].split(",")[0]) == n_levels      # every level is listed, and is a panel level
        hist = [sum(r[m] for r in rows) for m in range(16)]
        print("[tri1 two waves] %s: %d panels, %d levels, widths %s" % (g, n_panels, n_levels, hist))
        assert hist == WIDTHS[g] and sum(hist) == n_panels
        total = [a + b for a, b in zip(total, hist)]
    assert all(total), total


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("tri1_two_waves")
    out, stopped = {}, None
    for name in RUNS:
        if stopped:
            out[name] = dict(set=name, tune=TUNE, rc=None, records={}, seconds=0.0, stderr="", not_run_after=stopped)
            continue
        run = _run_child(name, TUNE, str(base / name), name == "first", CHILD_SECONDS + 30, child=CHILD,
                         prefix=("timeout", "-k", "10", str(CHILD_SECONDS)))
        out[name] = run
        print("[tri1 two waves] child %-6s rc %s  %.1f s" % (name, run["rc"], run["seconds"]))
        if _stops(run["rc"]):
            stopped = name
    return out


def _record(runs, name, graph):
    run = runs[name]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    rec = run["records"].get(graph)
    assert rec is not None, "child %s (rc %s) left no record of %s: %s" % (name, run["rc"], graph, run["stderr"])
    assert rec["status"] == "ok", rec["status"]
    return rec


@pytest.fixture(scope="module")
def refs(runs):
    cache = {}

    def get(graph):
        if graph not in cache:
            cache[graph] = _Ref(_record(runs, "first", graph))
        return cache[graph]
    return get


@gpu
@pytest.mark.parametrize("name", RUNS)
def test_child_ran_clean(runs, name):
    run = runs[name]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    assert run["rc"] == 0, (run["rc"], run["stderr"])
    assert sorted(run["records"]) == sorted(GRAPHS + ["negdef_w1"])
    print("[tri1 two waves] %s: child %.1f s; per graph %s" % (name, run["seconds"],
          ", ".join("%s %.2f" % (g, r.get("seconds", -1)) for g, r in run["records"].items())))


@gpu
@pytest.mark.parametrize("graph", GRAPHS)
def test_every_panel_went_through_tri1(runs, graph):
    """k_panel_tri1 has one work item per panel of the graph, in the stand-alone and in the fused sweep, and is the only factor form"""
    for name in RUNS:
        rec = _record(runs, name, graph)
        for key in ("census_plain", "census_fused"):
            forms = rec[key]["forms"]
            assert forms["k_panel_tri1"][2] == PANELS[graph], (name, graph, key, forms["k_panel_tri1"])
            assert forms["k_panel_tri<16>"][2] == 0 and forms["k_panel_tri<8>"][2] == 0
        assert sorted(f for f in _forms(rec) if f in FACTOR_FORMS) == ["k_panel_tri1"]
        if graph.startswith("complete"):
            assert rec["n_levels"] == PANELS[graph]                 # one panel per level


@gpu
@pytest.mark.parametrize("graph", GRAPHS)
def test_solves_match_dense(runs, refs, graph):
    rec = _record(runs, "first", graph)
    ref = refs(graph)
    a = _arrays(rec)
    bound = KAPPA * max(ref.eta_ref, ref.n * EPS)
    for key in ("d_step", "d_fused"):
        d = a[key]
        assert np.all(np.isfinite(d))
        fwd = float(np.abs(d - ref.ref).max() / np.abs(ref.ref).max())
        eta = ref.eta(d)
        print("[tri1 two waves] %s %s: forward %.3e  eta %.3e  eta_ref %.3e  n eps %.3e  ratio %.3f" % (
            graph, key, fwd, eta, ref.eta_ref, ref.n * EPS, eta / max(ref.eta_ref, ref.n * EPS)))
        np.testing.assert_allclose(d, ref.ref, rtol=0, atol=1e-9 * np.abs(ref.ref).max())
        assert eta <= bound, "%s %s: backward error %.3e > %.3e" % (graph, key, eta, bound)


@gpu
def test_not_positive_definite_is_reported_by_tri1_alone(runs):
    for name in RUNS:
        rec = _record(runs, name, "negdef_w1")
        assert sorted(f for f in _forms(rec) if f in FACTOR_FORMS) == ["k_panel_tri1"]
        assert rec["raised_step"] and rec["raised_fused"], rec


@gpu
@pytest.mark.parametrize("graph", GRAPHS)
def test_two_runs_give_the_same_bits(runs, graph):
    xa, xb = _arrays(_record(runs, "first", graph)), _arrays(_record(runs, "second", graph))
    for key in ("d_step", "d_fused"):
        diff = int(np.count_nonzero(xa[key] != xb[key]))
        assert diff == 0, "%s %s: %d entries differ (largest %.3e)" % (graph, key, diff, np.abs(xa[key] - xb[key]).max())
