"""Both forms of the selected inversion's sweep (kernels_sinv.hip: k_sinv_sweep<16>, 160 lane groups per column, and
k_sinv_sweep<4>, 40), the wrap of their target loops and the 42-column packing of k_sinv_prep, pinned to a dense inverse.

launch_sinv_sweep gives a level with fewer tasks than the device has compute units the 16-wave form, so graphs small enough for
a dense reference reach the 4-wave form only where a level is hundreds of tasks wide.  Three sets -- the selection left alone,
FGO_TUNE=sinv_wide=0 (every level 4-wave) and sinv_wide=1e9 (every level 16-wave) -- run the graphs of
tests/selinv_forms_child.py; the census (fgo_debug_selinv_census, which asks the launcher's own helper) proves that a case
reached what it is named for, and every diagonal block of marginal_cov_all and every requested pair block, on the factor's
pattern and off it, is held to R = numpy.linalg.inv(H):

    max|D - R_blk| / max|R_blk|  <=  16 * max(d_ref, n * 2**-53)   and   <= 1e-8 (tests/test_gpu_marginals_all.py)

d_ref: the largest blockwise distance of R from a second double-precision inverse (Cholesky), the reference's own attainable
error on this matrix; 16: a margin over two backward-stable dense inverses for a recursion that accumulates along the
elimination tree and sums in another order.  Neither is measured on the device (tests/test_selinv_forms_reference_cpu.py;
observed ratios: profiles/NOTES.md "Selected inversion forms against a dense inverse").

FGO_TUNE is read once per process, so each set runs in fresh children, one after another; FGO_TUNE is the only thing that
differs between the sets.  A set has two children: FGO_TASK_WORK=1 and FGO_NO_PANELS=1 alone leave the complete graph's columns
in chains of 16 per task (the chains are bounded by the FGO_TUNE key chain_work, process-wide like every key), so
complete200_w1_nopanels -- single-column tasks of every height -- runs in a second child whose FGO_TUNE is the set's plus
chain_work=0, which no selection of the selected inversion reads.  After a child that ends with a signal, an abort, a device
error or its timeout no further child is started and every remaining case fails as "not run after <set>"."""
import os

import numpy as np
import pytest

from tests import selinv_forms_child as child
from tests.test_gpu_launch_forms import _run_child, _stops
from tests.test_selinv_forms_reference_cpu import Reference, ba_dense

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "selinv_forms_child.py")

SETS = [("default", ""), ("wide4", "sinv_wide=0"), ("wide16", "sinv_wide=1e9")]
SET_NAMES = [s[0] for s in SETS]
SINGLE = "complete200_w1_nopanels"
GRAPHS = child.GRAPH_NAMES
MAIN_GRAPHS = [g for g in GRAPHS if g != SINGLE]
# (vertices, fixed vertex) of the g2o graphs; the bundle-adjustment graph has a prior instead of a fixed vertex
VERTICES = {"chain2": (2, 0), "chain43": (43, 0), "chain44": (44, 0), "chain86": (86, 0), "complete70": (70, 0), "complete200": (200, 0),
            SINGLE: (200, 0), "star600": (600, 1), "hub42x273": (child.N_HUBS + child.N_LEAVES, child.N_HUBS + child.N_LEAVES - 1),
            "synth200_leaf": (200, 0), "synth400_w1": (400, 0), "synth650_w50": (650, 0)}
MULTI_COLUMN = ["complete70", "complete200", "synth200_leaf", "synth400_w1", "synth650_w50"]
FORMS = (("w16", 160), ("w4", 40))


@pytest.fixture(scope="module")
def sruns(tmp_path_factory):
    """every set in children of its own, one after another; stops starting children after trouble"""
    base = tmp_path_factory.mktemp("selinv_forms")
    out, stopped, limit = {}, None, 600.0          # (the first child also pays the first use of the device)
    for name, tune in SETS:
        run = dict(set=name, records={}, children=[], not_run_after=stopped)
        out[name] = run
        parts = (("main", tune, MAIN_GRAPHS), ("single", (tune + "," if tune else "") + "chain_work=0", [SINGLE]))
        for part, part_tune, graphs in parts:
            if stopped:
                run["not_run_after"] = run["not_run_after"] or stopped
                continue
            r = _run_child(name, part_tune, str(base / name), name == "default", limit, child=CHILD, args=("--graphs", ",".join(graphs)))
            run["children"].append(r)
            run["records"].update(r["records"])
            print("[selinv forms] set %-8s %-6s rc %s  %.1f s" % (name, part, r["rc"], r["seconds"]))
            if _stops(r["rc"]):
                stopped = name
            if len(out) == 1 and part == "main":
                limit = max(60.0, 10.0 * r["seconds"])              # sized from the measured time of the first child
    return out


def _arrays(rec):
    with np.load(rec["npz"]) as z:
        return {k: z[k] for k in z.files}


def _record(sruns, set_name, graph):
    run = sruns[set_name]
    rec = run["records"].get(graph)
    if rec is None and run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    assert rec is not None, "set %s left no record of %s: %s" % (set_name, graph, [(c["rc"], c["stderr"]) for c in run["children"]])
    assert rec["status"] == "ok", rec["status"]
    return rec


@pytest.fixture(scope="module")
def srefs(sruns):
    """the dense reference of a graph, computed once and shared among the sets: from the default child's dense H for the g2o
    graphs, from the independent oracle for the bundle-adjustment graph"""
    cache = {}

    def get(graph):
        if graph not in cache:
            if graph == child.BA_GRAPH:
                cache[graph] = Reference(*ba_dense())
            else:
                a = _arrays(_record(sruns, "default", graph))
                n = int(a["H_n"][0])
                H = np.zeros((n, n))
                H[a["H_i"].astype(np.int64), a["H_j"].astype(np.int64)] = a["H_v"]
                cache[graph] = Reference(H)
        return cache[graph]
    return get


def _free_ids(graph):
    if graph == child.BA_GRAPH:
        return np.arange(sum(child.BA_SHAPE), dtype=np.int64)
    n, fixed = VERTICES[graph]
    return np.array([v for v in range(n) if v != fixed], np.int64)


@pytest.mark.parametrize("set_name", SET_NAMES)
def test_child_ran_clean(sruns, set_name):
    run = sruns[set_name]
    if run["not_run_after"]:
        pytest.fail("not run after %s" % run["not_run_after"])
    assert [c["rc"] for c in run["children"]] == [0, 0], [(c["rc"], c["stderr"]) for c in run["children"]]
    assert sorted(run["records"]) == sorted(GRAPHS)
    print("[selinv forms] %s: children %s s; per graph %s" % (set_name, ", ".join("%.1f" % c["seconds"] for c in run["children"]),
          ", ".join("%s %.2f" % (g, run["records"][g].get("seconds", -1)) for g in GRAPHS)))


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("set_name", SET_NAMES)
def test_blocks_match_dense_inverse(sruns, srefs, set_name, graph):
    """ids, every diagonal block, every pair block and the diagonal blocks' asymmetry within the bound; what the gather serves
    from one stored block equal to the bit"""
    rec = _record(sruns, set_name, graph)
    ref = srefs(graph)
    a = _arrays(rec)
    free = _free_ids(graph)
    np.testing.assert_array_equal(a["ids"], free)                   # the free ids, ascending
    assert ref.n == 6 * len(free)
    pos = np.full(int(free.max()) + 1, -1, np.int64)
    pos[free] = np.arange(len(free))
    cov = a["cov"]
    assert cov.shape == (len(free), 6, 6) and np.all(np.isfinite(cov))
    k = np.arange(len(free))
    worst = {}
    worst["diag"], pad = ref.errors(cov, k, k)
    worst["asym"] = float((np.abs(cov - cov.transpose(0, 2, 1)).max(axis=(1, 2)) / ref.rmax[k, k]).max())     # the kernel does not symmetrise
    n_pairs = 0
    for c in range(len(rec["fallback"])):
        pa, pb, pc = a["pa%d" % c], a["pb%d" % c], a["pc%d" % c]
        if len(pa) == 0:
            continue
        assert np.all(np.isfinite(pc))
        n_pairs += len(pa)
        rel, p = ref.errors(pc, pos[pa], pos[pb])
        worst["pairs%d" % c] = rel
        pad = max(pad, p)
        same = pa == pb                                             # pairs(a, a): the block of marginal_cov_all
        assert np.array_equal(pc[same], cov[pos[pa[same]]])
        assert same.any() or c == 0
    print("[selinv forms] %s %s: n %d  d_ref %.3e  bound %.3e  blocks %d + %d pairs (fallback %s)  ratio to bound: %s  padding %.1e" % (
        set_name, graph, ref.n, ref.d_ref, ref.bound, len(free), n_pairs, rec["fallback"],
        "  ".join("%s %.4f" % (key, v / ref.bound) for key, v in worst.items()), pad))
    # the factors' endpoints in both orders are on the pattern: one stored block, gathered as it is and transposed
    assert rec["fallback"][0] == 0
    pc0 = a["pc0"]
    h = len(pc0) // 2
    assert np.array_equal(a["pa0"][:h], a["pb0"][h:]) and np.array_equal(a["pb0"][:h], a["pa0"][h:])
    assert np.array_equal(pc0[h:], pc0[:h].transpose(0, 2, 1))
    if graph in ("star600", "hub42x273"):
        assert rec["fallback"][1] >= 1                              # leaf - leaf pairs: column solves, grouped by b
    if graph.startswith("complete"):
        assert rec["fallback"][1] == 0                              # every pair of a complete graph shares a factor
        pa, pb, pc = a["pa1"], a["pb1"], a["pc1"]
        nf = len(free)
        assert np.array_equal(pa.reshape(nf, nf), pb.reshape(nf, nf).T)
        off = ~np.eye(nf, dtype=bool)                                # (a diagonal block is not symmetrised: held to the bound above)
        assert np.array_equal(pc.reshape(nf, nf, 6, 6)[off], pc.reshape(nf, nf, 6, 6).transpose(1, 0, 3, 2)[off])
    for key, v in worst.items():
        assert v <= ref.bound, "%s %s %s: %.3e > %.3e (d_ref %.3e, n %d)" % (set_name, graph, key, v, ref.bound, ref.d_ref, ref.n)
    assert pad <= ref.bound


def _census(sruns, set_name, graph):
    return _record(sruns, set_name, graph)["census"]


@pytest.mark.parametrize("set_name", SET_NAMES)
def test_census_is_consistent(sruns, set_name):
    for g in GRAPHS:
        cz = _census(sruns, set_name, g)
        print("[selinv forms] census %s %s: %s" % (set_name, g, cz))
        assert cz["nb"] == len(_free_ids(g))
        assert cz["w16"]["columns"] + cz["w4"]["columns"] == cz["nb"]
        assert cz["prep_workgroups"] == (cz["nb"] + 41) // 42
        for form, groups in FORMS:
            f = cz[form]
            assert f["launches"] <= f["workgroups"] <= f["columns"]
            assert (f["wrap_cols"] > 0) == (f["max_m"] > groups)
            assert (f["columns"] > 0) == (f["workgroups"] > 0) == (f["max_task_cols"] > 0)


def test_forced_sets_ran_one_form_and_wrapped(sruns):
    for g in GRAPHS:
        assert _census(sruns, "wide4", g)["w16"]["workgroups"] == 0 and _census(sruns, "wide4", g)["w4"]["workgroups"] > 0
        assert _census(sruns, "wide16", g)["w4"]["workgroups"] == 0 and _census(sruns, "wide16", g)["w16"]["workgroups"] > 0
    for g in ("complete200", SINGLE):
        w4, w16 = _census(sruns, "wide4", g)["w4"], _census(sruns, "wide16", g)["w16"]
        assert w4["wrap_cols"] > 0 and w4["max_m"] >= 161           # more than four rounds of 40 targets
        assert w16["wrap_cols"] >= 1 and w16["max_m"] > 160


def test_default_set_reaches_the_four_wave_form_on_the_real_threshold(sruns):
    """with no override a level at least as wide as the device's compute units takes the 4-wave form: the star's leaf level
    (399 tasks), and the hub graph's (272 tasks of one column with 42 off-diagonal blocks: the wrap past 40 lane groups)"""
    cz = {g: _census(sruns, "default", g) for g in GRAPHS}
    launched = [g for g in GRAPHS if cz[g]["w4"]["launches"] > 0]
    wrapped = [g for g in GRAPHS if cz[g]["w4"]["wrap_cols"] > 0]
    print("[selinv forms] default: 4-wave launches on %s, 4-wave columns with m > 40 on %s (compute units %d)" % (launched, wrapped, cz["star600"]["cus"]))
    assert launched and wrapped
    if cz["star600"]["cus"] <= 272:                                 # (the widest level of the hub graph)
        assert "star600" in launched and "hub42x273" in wrapped
        assert cz["hub42x273"]["w4"]["wrap_cols"] == 272 and cz["hub42x273"]["w4"]["max_m"] == 42
    assert any(cz[g]["w16"]["launches"] > 0 for g in GRAPHS)


def test_named_shapes_were_reached(sruns):
    for s in SET_NAMES:
        cz = _census(sruns, s, "chain2")
        assert cz["nb"] == 1 and cz["empty_cols"] == 1              # a single free column, m = 0
        for g, nb, wgs in (("chain43", 42, 1), ("chain44", 43, 2), ("chain86", 85, 3)):
            cz = _census(sruns, s, g)
            assert (cz["nb"], cz["prep_workgroups"]) == (nb, wgs)
        for g in MULTI_COLUMN:
            cz = _census(sruns, s, g)
            assert max(cz["w16"]["max_task_cols"], cz["w4"]["max_task_cols"]) > 1
        cz = _census(sruns, s, SINGLE)
        assert max(cz["w16"]["max_task_cols"], cz["w4"]["max_task_cols"]) == 1
        assert cz["w16"]["workgroups"] + cz["w4"]["workgroups"] == cz["nb"] == 199
        assert max(cz["w16"]["max_m"], cz["w4"]["max_m"]) == 198    # single-column tasks of every height 0 .. 198


def test_forms_agree_to_the_bit_where_no_column_wraps(sruns):
    """Both forms compute an off-diagonal target with one lane group, in ascending q, and with at most 40 off-diagonal blocks in
    every column each lane group of either form holds at most one term of a diagonal sum, the empty groups adding zeros: for the
    graphs whose census shows a largest m <= 40 the three sets give the same bits in every output"""
    graphs = [g for g in GRAPHS if max(_census(sruns, "default", g)[f]["max_m"] for f, _ in FORMS) <= 40]
    print("[selinv forms] largest m <= 40: %s" % graphs)
    assert len(graphs) >= 4 and "star600" in graphs
    for g in graphs:
        base = _arrays(_record(sruns, "default", g))
        for s in ("wide4", "wide16"):
            other = _arrays(_record(sruns, s, g))
            for key in sorted(other):
                diff = int(np.count_nonzero(base[key] != other[key]))
                assert diff == 0, "default vs %s, %s %s: %d entries differ (largest %.3e)" % (s, g, key, diff, np.abs(base[key] - other[key]).max())
