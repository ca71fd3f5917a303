"""Dense depth alignment (csrc/kernels_depth_align.hip: fgo_depth_align_batch) against its numpy restatement
(tests/depth_align_reference.py, itself pinned to a per-pixel brute force by tests/test_depth_align_reference_cpu.py).  An ICP is
not in the reference tree: the restatement is the yardstick.

Scenes: depth frames of a three-wall corner by analytic ray-plane intersection, 176 x 144 ("big") and 40 x 30 ("small": image
borders within reach of every sample, normal_step at the edge, a partial wave on every level), 8 pairs each.  The CPU test has shown
that the restatement keeps every sample of these pairs more than 1e-6 away from every gate at every evaluation: the kernel then
associates the same samples, so COUNTS, ITERATIONS, CONVERGED AND STATUS ARE COMPARED FOR EQUALITY.  Where a test evaluates at a pose
or with parameters the CPU test did not cover, it asserts the same margins itself before it compares.

Tolerances.  The per-sample numbers of the two sides carry the same bits (the same operations in the same order, every one rounded
on its own); what differs is the order of the sums and the C library's sin and cos in the retraction.  The yardstick is the
restatement's own f64-against-longdouble difference over the 16 pairs, norm-wise (max |difference| / max |value| of a block; the
pose absolutely), recorded in depth_align_reference.YARDSTICK -- H 4.2e-16, g 5.5e-15, chi2 3.3e-15 at the first evaluation, pose
2.8e-16 and info 2.4e-16 after the full run -- and the kernel is allowed 16 x that: H 6.7e-15, g 8.8e-14, chi2 5.3e-14, pose 4.5e-15,
info 3.8e-15.  Every test prints what it measured before it asserts.
Ground truth: the recovered pose against the camera motion the frames were rendered with, within twice the restatement's own error
on the same frames (depth quantisation and nothing else; depth_align_reference.truth_bound).
Measured on 1 x MI355X at this commit, the kernel against the f64 restatement, largest over the 16 pairs: first evaluation H 2.0e-16,
g 4.3e-16, chi2 2.1e-16; full run pose 3.8e-16, info 2.6e-16, chi2 1.1e-14, rmse 6.5e-15; the truth within 0.115 mm and 0.07 mrad
at 176 x 144 (bound 0.23 mm, 0.14 mrad) and 3.2 cm and 5.4 mrad at 40 x 30 (bound 6.4 cm, 11 mrad).  The same figures are in DESIGN.md,
"Dense depth alignment"."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from graph_slam_amd import dense as D
from tests import depth_align_reference as ref

TOL = {k: ref.YARDSTICK_FACTOR * v for k, v in ref.YARDSTICK.items()}
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])
GIVEN = np.array([0.01, -0.005, 0.008, 0.0025, 0.0025, 0.0025, 1.0])         # about 1.4 cm and 0.5 degrees; normalised by the call


@functools.lru_cache(maxsize=None)
def gpu_run(kind, form=0):
    """the full run of the 8 pairs of a scene from the identity, once per kernel form"""
    S = ref.scene(kind)
    assert G.lib.fgo_debug_depth_align_form(form) == form
    try:
        return D.depth_align_batch(S["depth"], S["frame_i"], S["frame_j"], None, ref.params_struct(S["P"]), want_normal_eq=True)
    finally:
        G.lib.fgo_debug_depth_align_form(0)


def assert_clear(margins):
    for k, m in margins.items():
        assert m > (ref.MARGIN_REL if k.endswith("_rel") else ref.MARGIN), (k, m)


def assert_same_bits(a, b, keys=None):
    for k in keys or a:
        assert np.array_equal(a[k], b[k]), k


def full(info):
    M = np.zeros((6, 6))
    for r in range(6):
        for c in range(r, 6):
            M[r, c] = M[c, r] = info[ref.ut6(r, c)]
    return M


# ---- the first evaluation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["big", "small"])
def test_first_evaluation_from_the_identity(kind):
    out = gpu_run(kind)
    for p in range(8):
        want, got = ref.scene_run(kind, p)["normal_eq"], out["normal_eq"][p]
        m = {"H": ref.rel_diff(got[:21], want[:21]), "g": ref.rel_diff(got[21:27], want[21:27]), "chi2": ref.rel_diff(got[27:], want[27:])}
        print(kind, p, {k: "%.2e" % v for k, v in m.items()})
        for k, v in m.items():
            assert v <= TOL[k], (p, k, v)


@pytest.mark.parametrize("kind,n_pairs", [("big", 1), ("big", 8), ("small", 1), ("small", 3), ("small", 8)])
def test_first_evaluation_from_a_given_pose_with_its_count(kind, n_pairs):
    """iters = {0}: the result's evaluation IS the first one, so n_pairs_used is its count and info its H"""
    S = ref.scene(kind)
    P = dict(S["P"], n_levels=1, iters=(0, 0, 0))
    out = D.depth_align_batch(S["depth"], S["frame_i"][:n_pairs], S["frame_j"][:n_pairs], np.tile(GIVEN, (n_pairs, 1)), ref.params_struct(P),
                              want_normal_eq=True)
    for p in range(n_pairs):
        want = ref.align(S["depth"][S["frame_i"][p]], S["depth"][S["frame_j"][p]], GIVEN, P)
        assert_clear(want["margins"])
        assert want["status"] == ref.OK and want["evaluations"] == 1
        assert (out["status"][p], out["iterations"][p], out["converged"][p]) == (D.FGO_DA_OK, 0, 0)
        assert out["n_pairs_used"][p] == want["n_pairs_used"]
        assert np.array_equal(out["pose_ij"][p], want["pose_ij"])                     # the given pose, normalised
        got = out["normal_eq"][p]
        assert np.array_equal(out["info"][p], got[:21]) and out["chi2"][p] == got[27]
        m = {"H": ref.rel_diff(got[:21], want["normal_eq"][:21]), "g": ref.rel_diff(got[21:27], want["normal_eq"][21:27]),
             "chi2": ref.rel_diff(got[27:], want["normal_eq"][27:])}
        print(kind, p, want["n_pairs_used"], {k: "%.2e" % v for k, v in m.items()})
        for k, v in m.items():
            assert v <= TOL[k], (p, k, v)
        assert abs(out["rmse"][p] - want["rmse"]) <= TOL["chi2"] * want["rmse"]
        assert abs(out["min_pivot"][p] - want["min_pivot"]) <= 1e-12


def test_a_frame_too_large_for_lds_takes_the_global_form_by_itself():
    """200 x 160 words are 64 000 bytes, more than the lds form stages: the default form has to switch, and count the same"""
    P = ref.default_params(normal_jump=0.0505, n_levels=1, iters=(0, 0, 0), skip=(3, 1, 1))
    depth = np.stack([ref.render(ref.camera(), P, 200, 160), ref.render(ref.nearby_camera(4), P, 200, 160)])
    want = ref.align(depth[0], depth[1], GIVEN, P)
    assert_clear(want["margins"])
    out = D.depth_align_batch(depth, [0], [1], [GIVEN], ref.params_struct(P), want_normal_eq=True)
    assert out["status"][0] == D.FGO_DA_OK and out["n_pairs_used"][0] == want["n_pairs_used"] > 2000
    assert ref.rel_diff(out["normal_eq"][0][:21], want["normal_eq"][:21]) <= TOL["H"]
    assert ref.rel_diff(out["normal_eq"][0][21:27], want["normal_eq"][21:27]) <= TOL["g"]


# ---- the full run ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["big", "small"])
def test_full_run_against_the_restatement_and_the_ground_truth(kind):
    S, out = ref.scene(kind), gpu_run(kind)
    bt, br = ref.truth_bound(kind)
    for p in range(8):
        want = ref.scene_run(kind, p)
        for k in ("status", "iterations", "converged", "n_pairs_used"):                # exact
            assert out[k][p] == want[k], (p, k, out[k][p], want[k])
        m = {"pose": float(np.max(np.abs(out["pose_ij"][p] - want["pose_ij"]))), "info": ref.rel_diff(out["info"][p], want["info"]),
             "chi2": ref.rel_diff(out["chi2"][p], want["chi2"]), "rmse": ref.rel_diff(out["rmse"][p], want["rmse"])}
        dt, dr = ref.pose_error(out["pose_ij"][p], S["truth"][p])
        print(kind, p, {k: "%.2e" % v for k, v in m.items()}, "truth %.2e m %.2e rad of %.2e %.2e" % (dt, dr, bt, br))
        assert m["pose"] <= TOL["pose"] and m["info"] <= TOL["info"] and m["chi2"] <= TOL["chi2"] and m["rmse"] <= TOL["chi2"], (p, m)
        assert dt <= bt and dr <= br, (p, dt, dr)
        assert out["pose_ij"][p][6] > 0 and abs(np.linalg.norm(out["pose_ij"][p][3:]) - 1) < 1e-15
        cov = out["cov"][p]
        assert np.array_equal(cov, cov.T) and np.allclose(cov @ full(out["info"][p]), np.eye(6), atol=1e-9)
        assert np.linalg.eigvalsh(full(out["info"][p])).min() > 0
        assert abs(out["min_pivot"][p] - want["min_pivot"]) <= 1e-12 and out["min_pivot"][p] > S["P"]["min_pivot"]


@pytest.mark.parametrize("n_levels", [1, 2, 3])
def test_every_number_of_levels_runs(n_levels):
    S = ref.scene("small")
    P = dict(S["P"], n_levels=n_levels)
    out = D.depth_align_batch(S["depth"], S["frame_i"][:2], S["frame_j"][:2], None, ref.params_struct(P))
    for p in range(2):
        want = ref.align(S["depth"][S["frame_i"][p]], S["depth"][S["frame_j"][p]], None, P)
        assert_clear(want["margins"])
        for k in ("status", "iterations", "converged", "n_pairs_used"):
            assert out[k][p] == want[k], (p, k, out[k][p], want[k])
        assert want["status"] == ref.OK and want["iterations"] >= n_levels
        assert float(np.max(np.abs(out["pose_ij"][p] - want["pose_ij"]))) <= TOL["pose"]
        assert ref.rel_diff(out["info"][p], want["info"]) <= TOL["info"]


# ---- failure statuses ---------------------------------------------------------------------------------------------------------
def test_failure_statuses_and_the_void_record():
    S = ref.scene("small")
    wall = np.full((30, 40), 2000, np.uint16)             # fronto-parallel at an exact depth word: every normal is (0, 0, -1)
    depth = np.stack([wall, np.zeros((30, 40), np.uint16), np.full((30, 40), 6000, np.uint16), S["depth"][0]])
    out = D.depth_align_batch(depth, [0, 1, 2, 3], [0, 1, 2, 3], None, ref.params_struct(S["P"]))
    assert out["status"].tolist() == [D.FGO_DA_DEGENERATE, D.FGO_DA_TOO_FEW, D.FGO_DA_TOO_FEW, D.FGO_DA_OK]
    void = np.zeros(21); void[[ref.ut6(r, r) for r in range(6)]] = 10000.0
    for p in range(3):
        assert np.array_equal(out["pose_ij"][p], ref.align(depth[p], depth[p], None, S["P"])["pose_ij"])
        assert np.array_equal(out["pose_ij"][p], IDENTITY) and np.array_equal(out["info"][p], void) and not out["cov"][p].any()
        assert (out["iterations"][p], out["converged"][p], out["rmse"][p], out["chi2"][p]) == (0, 0, 0.0, 0.0)
    # the wall: J = (-y, x, 0, 0, 0, -1) for every sample, H has three zero rows exactly
    assert out["min_pivot"][0] == 0.0 < S["P"]["min_pivot"]
    assert out["n_pairs_used"][0] == ref.align(wall, wall, None, S["P"])["n_pairs_used"] >= S["P"]["min_pairs"]
    assert out["n_pairs_used"][1] == out["n_pairs_used"][2] == 0
    # a frame against itself: r = 0 for every sample, a zero step on every level, the identity exactly
    assert (out["iterations"][3], out["converged"][3]) == (S["P"]["n_levels"], 1)
    assert np.array_equal(out["pose_ij"][3], IDENTITY) and out["chi2"][3] == 0.0 and out["rmse"][3] == 0.0
    assert out["n_pairs_used"][3] == ref.align(depth[3], depth[3], None, S["P"])["n_pairs_used"]


# ---- forms and determinism --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["big", "small"])
def test_the_two_forms_give_the_same_bits(kind):
    a, b = gpu_run(kind, 1), gpu_run(kind, 2)
    assert_same_bits(a, b)
    assert_same_bits(a, gpu_run(kind))                     # the default is the lds form where a frame fits


@pytest.mark.parametrize("kind", ["big", "small"])
def test_two_calls_and_any_batch_give_a_pair_the_same_bits(kind):
    S, first = ref.scene(kind), gpu_run(kind)
    P = ref.params_struct(S["P"])
    again = D.depth_align_batch(S["depth"], S["frame_i"], S["frame_j"], None, P, want_normal_eq=True)
    assert_same_bits(first, again)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    shuffled = D.depth_align_batch(S["depth"], S["frame_i"][perm], S["frame_j"][perm], None, P, want_normal_eq=True)
    for k in first:
        assert np.array_equal(shuffled[k], first[k][perm]), k
    for sub in ([3], [6, 1]):
        part = D.depth_align_batch(S["depth"], S["frame_i"][sub], S["frame_j"][sub], None, P, want_normal_eq=True)
        for k in first:
            assert np.array_equal(part[k], first[k][sub]), k


# ---- from the RANSAC's void records to edges --------------------------------------------------------------------------------------
def test_align_failed_records_repairs_the_void_records_and_leaves_the_rest():
    S = ref.scene("big")
    rng = np.random.default_rng(5)
    # four records: 0 and 2 have 30 exact matches under the true motion, 1 has two matches and 3 none -- the RANSAC voids those
    counts = [30, 2, 30, 0]
    ptr = np.concatenate([[0], np.cumsum(counts)])
    xj = rng.uniform([-1, -1, 1.5], [1, 1, 3.5], (ptr[-1], 3)); xi = np.zeros_like(xj)
    for p in range(4):
        t = S["truth"][p]
        R = np.array(ref.qmat(t[3:]))
        xi[ptr[p]:ptr[p + 1]] = xj[ptr[p]:ptr[p + 1]] @ R.T + t[:3]
    vro = G.vro_ransac_batch(ptr, xi, xj)
    assert vro["status"].tolist() == [G.FGO_VRO_OK, G.FGO_VRO_TOO_FEW, G.FGO_VRO_OK, G.FGO_VRO_TOO_FEW]
    out = D.align_failed_records(S["depth"], S["frame_i"][:4], S["frame_j"][:4], vro, params=ref.params_struct(S["P"]))
    assert out["source"].tolist() == [D.FGO_DA_SOURCE_VRO, D.FGO_DA_SOURCE_DENSE, D.FGO_DA_SOURCE_VRO, D.FGO_DA_SOURCE_DENSE]
    assert out["dense_index"].tolist() == [1, 3]
    for p in (0, 2):                                       # untouched, bit for bit
        assert np.array_equal(out["pose_ij"][p], vro["pose_ij"][p]) and np.array_equal(out["info"][p], vro["info"][p])
    full_run = gpu_run("big")
    for p in (1, 3):
        assert np.array_equal(vro["pose_ij"][p], IDENTITY)                         # what the RANSAC left: the void record
        assert np.all(np.isfinite(out["pose_ij"][p])) and np.linalg.eigvalsh(full(out["info"][p])).min() > 0
        assert np.array_equal(out["pose_ij"][p], full_run["pose_ij"][p]) and np.array_equal(out["info"][p], full_run["info"][p])
        dt, dr = ref.pose_error(out["pose_ij"][p], S["truth"][p])
        assert dt <= ref.truth_bound("big")[0] and dr <= ref.truth_bound("big")[1]
    # where the alignment fails too the void record stays, flagged
    blank = np.zeros_like(S["depth"])
    out = D.align_failed_records(blank, S["frame_i"][:4], S["frame_j"][:4], vro)
    assert out["source"].tolist() == [D.FGO_DA_SOURCE_VRO, D.FGO_DA_SOURCE_VOID, D.FGO_DA_SOURCE_VRO, D.FGO_DA_SOURCE_VOID]
    assert np.array_equal(out["pose_ij"][1], IDENTITY) and out["info"][1][0] == 10000.0
