"""The ledger of tests/growth_forms.py, without a device: that every case of tests/test_gpu_growth_forms.py sits on the edge it is
named for (hub threshold 64 / 65, slice boundaries 512 / 513 and 1024 / 1025, hub buffers 256 / 257 entries), that every factor
appended after the build lies on a pair the structure already has or in the band of a reserve slot (so that only what a case
names can force a rebuild), and the ledger's own arithmetic against a second, brute-force count."""
import numpy as np
import pytest

from tests import growth_forms as GF

CASES = GF.all_cases()


def _brute(case, upto):
    """half-edge degrees and duplicate groups of the graph after step `upto`, counted the slow way"""
    kinds = [k for st in case["steps"][:upto + 1] for k, _ in st["vars"]]
    fixed = [f for st in case["steps"][:upto + 1] for _, f in st["vars"]]
    fac = [f for st in case["steps"][:upto + 1] for f in st["factors"]]
    deg = [sum((i == v) + (j == v) for i, j, _ in fac) for v in range(len(kinds))]
    pairs = [frozenset((i, j)) for i, j, _ in fac if i != j and not fixed[i] and not fixed[j]]
    groups = {p: pairs.count(p) for p in set(pairs) if pairs.count(p) > 1}
    return np.array(deg), groups


@pytest.mark.parametrize("name", sorted(CASES))
def test_ledger_counts_every_step(name):
    case = CASES[name]
    led = GF.ledger(case)
    assert len(led) == len(case["steps"])
    for s, L in enumerate(led):
        if len(case["steps"][s]["factors"]) > 600 and s + 1 < len(led):       # (the brute count is quadratic: the long steps' ends only)
            continue
        deg, groups = _brute(case, s)
        np.testing.assert_array_equal(L["deg"], deg)
        T = L["hub_deg"]
        want = [0 if d <= T else min(64, int(np.ceil(d / 512))) for d in deg]
        np.testing.assert_array_equal(L["entries"], want)
        assert L["n_hubs"] == sum(want) and L["n_hub_vars"] == sum(w > 0 for w in want) and L["n_hub_multi"] == sum(w > 1 for w in want)
        assert {frozenset(p): len(m) for p, m in L["dup_groups"].items()} == groups
        assert L["n_dup_groups"] == len(groups) and L["n_dup_members"] == sum(groups.values())
        assert L["n_priors"] == GF.counts(case, s)[2]
        assert 0 <= L["n_phantom"] <= case["growth"][0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_appended_pair_exists_or_lies_in_the_band(name):
    case = CASES[name]
    for s, L in enumerate(GF.ledger(case)):
        assert L["structure_rebuilt"] == (s == 0) or L["why"] == "hub_cap", (s, L["why"])
        assert all(L["in_band"]), (s, L["in_band"])
        if s > 0:
            assert len(L["in_band"]) == len(case["steps"][s]["factors"])


def test_growth_off_builds_every_step():
    for case in CASES.values():
        led = GF.ledger(case, growth=False)
        assert all(L["structure_rebuilt"] == 1 and L["n_phantom"] == 0 for L in led)
        assert all(L["hub_cap"] == L["n_hubs"] for L in led)


def _rebuilt(name):
    return [L["structure_rebuilt"] for L in GF.ledger(CASES[name])]


def test_dup_in_place_forms_the_groups_it_names():
    led = GF.ledger(CASES["dup_in_place"])
    assert [L["n_dup_groups"] for L in led] == [0, 1, 1, 1, 2]
    assert [L["n_dup_members"] for L in led] == [0, 2, 3, 3, 5]
    assert led[2]["dup_groups"][(3, 4)] == [5, 21, 22] and CASES["dup_in_place"]["steps"][2]["factors"] == [(4, 3, GF.SE3)]     # the reversed member
    assert CASES["dup_in_place"]["steps"][3]["factors"] == [(0, 1, GF.SE3)] and CASES["dup_in_place"]["steps"][0]["vars"][0][1]  # fixed end: no group
    assert (5, 7) in led[4]["dup_groups"] and _rebuilt("dup_in_place") == [1, 0, 0, 0, 0]
    tw = GF.ledger(CASES["dup_twin"])
    assert [L["n_dup_groups"] for L in tw] == [1, 1] and [L["n_dup_members"] for L in tw] == [2, 3] and _rebuilt("dup_twin") == [1, 0]
    assert all(L["n_hubs"] == 0 and L["hub_deg"] == 64 for L in led + tw)


def test_hub_by_new_vertices_crosses_64_65():
    led = GF.ledger(CASES["hub_by_new_vertices"])
    assert [int(L["deg"][7]) for L in led] == [1, 64, 65]
    assert [L["n_hubs"] for L in led] == [0, 0, 1] and [L["n_hub_multi"] for L in led] == [0, 0, 0]
    assert led[2]["entries"][7] == 1 and led[2]["hub_deg"] == 64 and led[2]["hub_cap"] == 256
    assert _rebuilt("hub_by_new_vertices") == [1, 0, 0] and [L["n_phantom"] for L in led] == [80, 18, 17]


def test_slices_by_duplicates_crosses_every_slice_boundary():
    led = GF.ledger(CASES["slices_by_duplicates"])
    assert [int(L["deg"][0]) for L in led] == [8, 64, 65, 512, 513, 1024, 1025]
    assert [int(L["entries"][0]) for L in led] == [0, 0, 1, 1, 2, 2, 3]
    assert [L["n_hub_multi"] for L in led] == [0, 0, 0, 0, 1, 1, 1]
    assert _rebuilt("slices_by_duplicates") == [1, 0, 0, 0, 0, 0, 0]
    last = led[-1]
    assert last["n_dup_groups"] == 7 and max(len(m) for m in last["dup_groups"].values()) >= 128        # pose 1 is fixed: its spoke has no group
    # the orientation alternates on every spoke
    fac = [f for st in CASES["slices_by_duplicates"]["steps"] for f in st["factors"]]
    for p, members in last["dup_groups"].items():
        fwd = sum(fac[e][0] == 0 for e in members)
        assert abs(2 * fwd - len(members)) <= 2, (p, fwd, len(members))
    # the spoke poses become one-slice hubs on the way (64 / 65 of their own)
    assert last["n_hubs"] == 3 + 8 and all(int(d) > 64 for d in last["deg"])


def test_all_hubs_cases_make_every_variable_above_degree_two_a_hub():
    for name in ("dup_in_place_hub2", "dup_twin_hub2", "chain_hub2"):
        led = GF.ledger(CASES[name])
        for L in led:
            assert L["hub_deg"] == 2 and L["n_hub_multi"] == 0 and L["n_hubs"] == int((L["deg"] > 2).sum()) > 0.8 * len(L["deg"])
        assert _rebuilt(name) == [1] + [0] * (len(led) - 1)


def test_hub_cap_overflows_at_257_entries():
    led = GF.ledger(CASES["hub_cap_overflow"])
    assert [L["n_hubs"] for L in led] == [0, 256, 298] and led[1]["hub_cap"] == 256 == led[1]["n_hubs"]
    assert _rebuilt("hub_cap_overflow") == [1, 0, 1] and led[2]["why"] == "hub_cap" and led[2]["hub_cap"] == 298 + 256
    assert len(CASES["hub_cap_overflow"]["steps"][1]["factors"]) == 255
    one = GF.ledger(CASES["hub_cap_257"])
    assert [L["n_hubs"] for L in one] == [0, 256, 257, 298] and _rebuilt("hub_cap_257") == [1, 0, 1, 0] and one[2]["why"] == "hub_cap"
    assert one[3]["hub_cap"] == 257 + 256 and one[3]["n_phantom"] == 8


def test_landmark_hubs_cross_64_65_and_512_513():
    for name, lm_pri in (("plane_hub", 0), ("point_hub", 1)):
        led = GF.ledger(CASES[name])
        assert [int(L["deg"][8]) for L in led] == [8, 64, 65, 512, 513]
        assert [int(L["entries"][8]) for L in led] == [0, 0, 1, 1, 2] and [L["n_hubs"] for L in led] == [0, 0, 1, 1, 2]
        assert [L["n_dup_groups"] for L in led] == [0, 0, 0, 65, 65] and _rebuilt(name) == [1, 0, 0, 0, 0]
        assert [L["n_priors"] for L in led] == [1 + lm_pri] * 5 and [L["maskable"] for L in led] == [1, 1, 0, 0, 0]


def test_mixed_in_place_claims_slots_of_every_kind_and_adds_priors_alone():
    case = CASES["mixed_in_place"]
    led = GF.ledger(case)
    assert _rebuilt("mixed_in_place") == [1, 0, 0, 0, 0]
    assert [L["n_phantom"] for L in led] == [12, 10, 8, 8, 7] and [L["n_priors"] for L in led] == [1, 1, 1, 3, 3]
    assert [k for k, _ in case["steps"][2]["vars"]] == [GF.PLANE, GF.POINT] and case["steps"][3]["factors"] == [] and case["steps"][3]["vars"] == []
    assert all(L["maskable"] == 1 and L["n_hubs"] == 0 and L["n_dup_groups"] == 0 for L in led)


def test_masked_then_not_loses_the_precondition_at_the_duplicate():
    led = GF.ledger(CASES["masked_then_not"])
    assert [L["maskable"] for L in led] == [1, 1, 1, 1, 0, 0, 0] and [L["n_dup_groups"] for L in led] == [0, 0, 0, 0, 1, 1, 1]
    assert _rebuilt("masked_then_not") == [1] + [0] * 6 and len(led[-1]["deg"]) == 40


def test_measurements_are_reproducible_and_keep_the_landmarks_in_view():
    for name in ("dup_in_place", "mixed_in_place", "point_hub"):
        a, b = GF.realise(CASES[name]), GF.realise(CASES[name])
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])
    d = GF.realise(CASES["point_hub"])
    uv = d["meas"][d["fkind"] == GF.REPROJ, :2]
    assert np.all(np.isfinite(uv)) and np.abs(uv[:, 0] - 90).max() < 150 and np.abs(uv[:, 1] - 70).max() < 120
