"""Host structure phase (ordering.cpp + symbolic.cpp and their phase files) on several host threads: the elimination order, the update
lists and the task / panel schedule must be the same for every thread count (the parallel top of the nested dissection --
ordering_tree.cpp order_all -- emits in post-order, the update lists are generated per target column with no shared cursors).  CPU
only: builds the developer tool tools/symstats.cpp, which links the two drivers without the device part."""
import os
import subprocess

import pytest

from tests.util import build_symstats


@pytest.fixture(scope="module")
def symstats():
    return build_symstats()


def run(exe, n, threads, leaf=64):
    env = dict(os.environ, FGO_HOST_THREADS=str(threads))
    out = subprocess.run([exe, str(n), "5", "4", str(leaf), "5000", "1000000000"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    keep = [l for l in out.stdout.splitlines() if l.startswith(("nnzL", "panels", "ops:", "level 0:", "structure checksum", "critical-path"))]
    assert any(l.startswith("structure checksum") for l in keep)
    return keep


@pytest.mark.parametrize("n", [600, 20000])
def test_structure_does_not_depend_on_the_thread_count(symstats, n):
    ref = run(symstats, n, 1)
    for threads in (2, 5, 16):
        assert run(symstats, n, threads) == ref


def test_small_leaf_size_exercises_the_parallel_top_tree(symstats):
    # leaf 8: the top tree is expanded even on a small graph (regions > 8 * leaf are bisected concurrently)
    assert run(symstats, 3000, 8, leaf=8) == run(symstats, 3000, 1, leaf=8)


def test_ordering_quality_on_the_benchmark_graph(symstats):
    """cfg 2 (100k poses / 1M edges): the level-synchronous sweeps pay ~70 us per level, so the depth of the schedule is
    the quantity the separator selection is tuned for (69 levels with raw level sizes from one end, 35 now).
    Bounds with some slack: a change that costs levels or fill should be a decision, not an accident."""
    import re
    line = [l for l in run(symstats, 100000, 4) if l.startswith("nnzL")][0]
    nnz = int(re.search(r"nnzL blocks (\d+)", line).group(1))
    nops = int(re.search(r"nops (\d+)", line).group(1))
    height = int(re.search(r"etree_height (\d+)", line).group(1))
    levels = int(re.search(r"levels (\d+)", line).group(1))
    assert levels <= 40 and height <= 460
    assert nnz <= 2.45e6 and nops <= 34.0e6


def test_fgo_tune_overrides_a_schedule_constant(symstats):
    """The tuning constants are overridden through ONE variable, FGO_TUNE="key=value,..." (csrc/fgo_internal.hpp tune()):
    merge_multi=0 restores round 1's panel rule (a panel does not continue across a separator boundary), which costs levels;
    an unknown key is ignored."""
    import re

    def levels(tune):
        env = dict(os.environ, FGO_HOST_THREADS="4")
        if tune is not None:
            env["FGO_TUNE"] = tune
        out = subprocess.run([symstats, "20000", "5", "4", "64", "5000", "1000000000"], capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        return int(re.search(r"levels (\d+)", [l for l in out.stdout.splitlines() if l.startswith("nnzL")][0]).group(1))
    base = levels(None)
    assert levels("no_such_key=3") == base
    assert levels("merge_multi=0,no_such_key=1") > base


def _levels(exe, n, lookback, loops, extra_env):
    env = dict(os.environ, **extra_env)
    out = subprocess.run([exe, str(n), str(lookback), str(loops), "64", "5000", "1152921504606846976"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("nnzL blocks")][0].split()
    return int(line[line.index("levels") + 1]), int(line[2]), int(line[line.index("nops") + 1])


@pytest.mark.parametrize("n", [6000, 30000])
def test_time_dissection_under_recovered_labels(symstats, n):
    """VERDICT r5 next #4a: a band graph (predecessor + look-back edges, no loop closures) whose vertex ids are NOT creation order -- a .g2o
    file need not number its vertices in time -- gets the index-cut dissection too: one Cuthill-McKee pass recovers the order (ordering.cpp
    cuthill_mckee_labels), the same band test decides, and the structure comes out as that of the creation-order graph (levels within one,
    fill and block updates within 1 %); with the recovery switched off the relabelled graph falls back to the level structures."""
    lv0, nnz0, ops0 = _levels(symstats, n, 10, 0, {})
    for seed in ("1", "2"):
        lv, nnz, ops = _levels(symstats, n, 10, 0, {"FGO_SHUFFLE": seed})
        assert abs(lv - lv0) <= 1, (lv, lv0)
        assert abs(nnz - nnz0) <= 0.01 * nnz0 and abs(ops - ops0) <= 0.01 * ops0, (nnz, nnz0, ops, ops0)
    # the switch really is what does it: without the recovery the relabelled graph takes another path (a different structure)
    lvx, nnzx, opsx = _levels(symstats, n, 10, 0, {"FGO_SHUFFLE": "1", "FGO_TUNE": "nd_time_recover=0"})
    assert (lvx, nnzx, opsx) != (lv0, nnz0, ops0)


def test_recovered_labels_do_not_hijack_a_graph_with_loop_closures(symstats):
    """cfg-2-like graph (4 closures per pose) relabelled at random: the Cuthill-McKee order passes the band test for 64 % of the edges only
    (breadth-first fronts fold over each other at every closure) -- forcing the index cuts on it was measured (41 levels against 30, twice
    the block updates): it must keep the level-structure dissection, i.e. the structure it had before round 6"""
    a = _levels(symstats, 20000, 5, 4, {"FGO_SHUFFLE": "1"})
    b = _levels(symstats, 20000, 5, 4, {"FGO_SHUFFLE": "1", "FGO_TUNE": "nd_time_recover=0"})
    assert a == b
