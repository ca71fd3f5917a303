"""The numpy restatement of the descriptor matching (tests/feature_match_reference.py) pinned on the CPU: against plain double loops on
tiny inputs, the tie rules, d2 = d1 on a tied minimum, the one-candidate rule, and the conditions the generated GPU cases must meet
(no undecided gate, every reason and every planted case present)."""
import math

import numpy as np
import pytest

from tests import feature_match_reference as ref


def _loops(fj, fi, pose7=None, **params):
    """the semantics of include/fgo.h, one (a, b) at a time"""
    P = dict(ref.DEFAULTS, **params)
    dj, di = fj["desc"].astype(int), fi["desc"].astype(int)
    nj, ni = len(dj), len(di)
    ok = lambda p: all(math.isfinite(c) for c in p) and p[2] > 0
    if pose7 is not None:
        R, t = ref.quat_matrix(pose7[3:]), pose7[:3]
    D = [[-1] * ni for _ in range(nj)]
    for a in range(nj):
        for b in range(ni):
            if not ok(fj["xyz"][a]) or not ok(fi["xyz"][b]):
                continue
            if pose7 is not None:
                p = R.T @ (fi["xyz"][b] - t)
                if not p[2] > 0:
                    continue
                u = P["fx"] * p[0] / p[2] + P["cx"]; v = P["fy"] * p[1] / p[2] + P["cy"]
                if (u - fj["uv"][a][0]) ** 2 + (v - fj["uv"][a][1]) ** 2 > P["radius_px"] ** 2:
                    continue
                if P["max_dist_3d"] > 0 and sum((p - fj["xyz"][a]) ** 2) > P["max_dist_3d"] ** 2:
                    continue
            D[a][b] = sum((int(x) - int(y)) ** 2 for x, y in zip(dj[a], di[b]))
    best, d1, d2, reason = [-1] * nj, [-1] * nj, [-1] * nj, [0] * nj
    for a in range(nj):
        if not ok(fj["xyz"][a]):
            reason[a] = 1
            continue
        cand = [(D[a][b], b) for b in range(ni) if D[a][b] >= 0]
        if not cand:
            reason[a] = 2
            continue
        cand.sort()
        d1[a], best[a] = cand[0]
        if len(cand) > 1:
            d2[a] = cand[1][0]
        if P["ratio_test"] and len(cand) > 1 and not (float(d1[a]) < P["ratio"] * P["ratio"] * float(d2[a])):
            reason[a] = 3
        elif d1[a] > P["max_desc_dist2"]:
            reason[a] = 4
        elif P["cross_check"]:
            col = sorted((D[q][best[a]], q) for q in range(nj) if D[q][best[a]] >= 0)
            if col[0][1] != a:
                reason[a] = 5
    return np.array(D, np.int64).reshape(nj, ni), best, d1, d2, reason


def _tiny(rng, nj, ni, spread=3):
    """descriptors from a small alphabet, so that ties happen; a few points without depth; pixels around the projections"""
    mk = lambda n: dict(desc=rng.integers(0, spread, (n, ref.DIM)).astype(np.uint8) * 40,
                        xyz=np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(1, 4, n)], 1))
    fj, fi = mk(nj), mk(ni)
    for f in (fj, fi):
        f["uv"] = ref.project(f["xyz"]) + rng.uniform(-3, 3, (len(f["xyz"]), 2))
        if len(f["xyz"]) > 3:
            f["xyz"][1] = [0.1, 0.2, 0.0]; f["xyz"][3, 0] = np.nan
    return fj, fi


@pytest.mark.parametrize("params", ref.CONFIGS + (dict(ratio=1.0), dict(max_desc_dist2=150000), dict(radius_px=60.0, max_dist_3d=0.8)))
def test_restatement_equals_plain_loops(params):
    rng = np.random.default_rng(11)
    for nj, ni in ((0, 3), (3, 0), (1, 1), (5, 7), (9, 4), (12, 12)):
        fj, fi = _tiny(rng, nj, ni)
        if nj > 6 and ni > 6:
            fi["desc"][6] = fi["desc"][2]; fj["desc"][5] = fj["desc"][0]          # ties among the trains and among the queries
        for pose in (None, np.array([0.05, -0.02, 0.03, 0.01, -0.02, 0.015, 1.0])):
            p = dict(params, radius_px=max(params.get("radius_px", 0), 80.0)) if pose is not None else params
            D, best, d1, d2, reason = _loops(fj, fi, pose, **p)
            r = ref.match_pair(fj, fi, pose, **p)
            assert np.array_equal(r["dist"], D), (nj, ni)
            assert (list(r["best"]), list(r["d1"]), list(r["d2"]), list(r["reason"])) == (best, d1, d2, reason), (nj, ni, params)
            kept = [a for a in range(nj) if reason[a] == 0]
            assert list(r["a"]) == kept and list(r["b"]) == [best[a] for a in kept]
            assert r["n_matches"] == len(kept) and r["status"] == (ref.FM_TOO_FEW if len(kept) < 12 else ref.FM_OK)


def _frame(desc, xyz=None):
    desc = np.asarray(desc, np.uint8)
    xyz = np.tile([0.0, 0.0, 2.0], (len(desc), 1)) if xyz is None else np.asarray(xyz, float)
    return dict(desc=desc, xyz=xyz, uv=ref.project(xyz))


def test_tie_rules_second_equals_best_and_one_candidate():
    z = np.zeros(ref.DIM, np.uint8)
    e = lambda k, v=10: np.where(np.arange(ref.DIM) == k, v, 0).astype(np.uint8)
    # trains 1 and 3 are the same descriptor: the lowest index wins and the second distance equals the first
    r = ref.match_pair(_frame([e(0)]), _frame([e(5), e(0), e(7), e(0)]), ratio_test=0)
    assert (r["best"][0], r["d1"][0], r["d2"][0], r["reason"][0]) == (1, 0, 0, 0)
    r = ref.match_pair(_frame([e(0)]), _frame([e(5), e(0), e(7), e(0)]))
    assert r["reason"][0] == 3                                   # 0 < 0.25 * 0 is false
    # two queries with the same best train at the same distance: the cross-check keeps the lowest a
    r = ref.match_pair(_frame([e(1), e(0), e(0)]), _frame([e(0), e(9, 200)]), min_matches=0)
    assert list(r["best"]) == [0, 0, 0] and list(r["reason"]) == [5, 0, 5] and list(r["a"]) == [1] and r["n_cross"] == 2
    r = ref.match_pair(_frame([e(1), e(0), e(0)]), _frame([e(0), e(9, 200)]), cross_check=0)
    assert list(r["reason"]) == [0, 0, 0] and list(r["b"]) == [0, 0, 0]          # several queries keep one train
    # exactly one candidate: d2 = -1, the ratio test passes whatever the distance
    r = ref.match_pair(_frame([np.full(ref.DIM, 255)]), _frame([z]))
    assert (r["best"][0], r["d1"][0], r["d2"][0], r["reason"][0]) == (0, 128 * 255 ** 2, -1, 0)
    assert r["d1"][0] == 8323200
    # no candidate, and a feature that is not usable
    r = ref.match_pair(_frame([z, z], [[0, 0, 2.0], [0, 0, -1.0]]), _frame([z], [[0, 0, np.inf]]))
    assert list(r["reason"]) == [2, 1] and list(r["best"]) == [-1, -1] and (r["n_query"], r["n_train"]) == (1, 0)
    # the ratio is compared squared, strictly: d1 = 100, d2 = 400, ratio 0.5 -> 100 < 0.25 * 400 is false
    r = ref.match_pair(_frame([z]), _frame([e(0, 10), e(1, 20)]))
    assert (r["d1"][0], r["d2"][0], r["reason"][0]) == (100, 400, 3)
    r = ref.match_pair(_frame([z]), _frame([e(0, 10), e(1, 21)]))
    assert (r["d1"][0], r["d2"][0], r["reason"][0]) == (100, 441, 0)
    # the cap
    assert ref.match_pair(_frame([z]), _frame([e(0, 10)]), max_desc_dist2=99)["reason"][0] == 4
    assert ref.match_pair(_frame([z]), _frame([e(0, 10)]), max_desc_dist2=100)["reason"][0] == 0


def test_the_gate_belongs_to_the_pair_and_reports_its_margins():
    P = ref.DEFAULTS
    xyz_i = np.array([[0.0, 0.0, 2.0], [0.5, 0.0, 2.0]])
    pose = np.array([0.1, 0, 0, 0, 0, 0, 1.0])                   # p_j = p_i - (0.1, 0, 0)
    pj = xyz_i - pose[:3]
    uv_j = ref.project(pj) + [[9.0, 0.0], [0.0, 10.5]]           # 9 px: inside; 10.5 px: outside
    inside, und = ref.gate(pj, uv_j, xyz_i, pose, P)
    assert inside.tolist() == [[True, False], [False, False]] and not und.any()
    uv_j = ref.project(pj) + [[10.0 * (1 + 1e-8), 0.0], [0.0, 3.0]]
    inside, und = ref.gate(pj, uv_j, xyz_i, pose, P)
    assert und[0, 0] and not und[1, 1] and inside[1, 1]          # a gate on its threshold is reported
    inside, _ = ref.gate(pj, ref.project(pj), xyz_i, pose, dict(P, max_dist_3d=0.01))
    assert inside.tolist() == [[True, False], [False, True]]
    inside, _ = ref.gate(pj + [0, 0, 0.02], ref.project(pj), xyz_i, pose, dict(P, max_dist_3d=0.01))
    assert not inside.any()
    behind = np.array([0, 0, 0, 0, 1.0, 0, 0])
    assert not ref.gate(pj, uv_j, xyz_i, behind, P)[0].any()


@pytest.mark.parametrize("cfg", range(len(ref.CONFIGS)))
def test_generated_gpu_cases_are_decided_and_hold_every_planted_case(cfg):
    frames, pairs, planted = ref.gpu_cases()
    params = ref.CONFIGS[cfg]
    seen, sizes = np.zeros(6, int), set()
    res = []
    for fj, fi, pose in pairs:
        r = ref.match_pair(frames[fj], frames[fi], pose, **params)
        assert r["undecided"] == 0, (fj, fi)
        seen += np.bincount(r["reason"], minlength=6)
        sizes.add((len(frames[fj]["desc"]), len(frames[fi]["desc"])))
        res.append(r)
    assert max(len(f["desc"]) for f in frames) <= ref.MAX_FEATURES
    assert {n for s in sizes for n in s} >= set(ref.SIZES) and sum(a != b for a, b in sizes) > len(sizes) // 2
    assert max(r["dist"].max() for r in res if r["dist"].size) == 8323200
    if cfg == 0:
        assert (seen[[0, 1, 2, 3, 5]] > 0).all(), seen
        k = {(j, i, p is not None): n for n, (j, i, p) in enumerate(pairs)}
        free, guided = res[k[15, 14, False]], res[k[15, 14, True]]
        for a, b in planted:                                     # the gate excludes the global nearest neighbour
            assert free["best"][a] == b and free["d1"][a] == 0 and guided["best"][a] != b and guided["reason"][a] == 0
        assert guided["n_matches"] > free["n_matches"] > 50      # and tells the look-alikes apart
        assert res[k[13, 12, True]]["n_matches"] == 0 and (res[k[13, 12, True]]["dist"] == -1).all()
        assert (res[k[11, 10, True]]["dist"] == -1).all() and set(res[k[11, 10, True]]["reason"]) <= {1, 2}
        same = res[k[9, 9, False]]
        ok = ref.usable(frames[9]["xyz"])
        assert (same["d1"][ok] == 0).all() and (np.diag(same["dist"])[ok] == 0).all()
        assert any((r["d2"] == r["d1"]).any() and (r["d1"] >= 0).any() for r in res)
        st = [r["status"] for r in res]
        assert ref.FM_OK in st and ref.FM_TOO_FEW in st
    if cfg == 4:
        assert seen[4] > 0 and seen[0] > 0, seen
    print("config %d: reasons 0..5 over the batch: %s" % (cfg, seen))


def test_end_to_end_cases_have_wrong_matches_and_look_alikes():
    frames, planted = ref.e2e_cases()
    for p in range(len(planted)):
        fi, fj = frames[2 * p], frames[2 * p + 1]
        r = ref.match_pair(fj, fi)
        wrong = fj["ids"][r["a"]] != fi["ids"][r["b"]]
        assert r["n_matches"] >= 60 and 0.1 < wrong.mean() < 0.5, (r["n_matches"], wrong.mean())
        assert r["n_ratio"] >= 60                                # the look-alikes the unguided ratio test rejects
