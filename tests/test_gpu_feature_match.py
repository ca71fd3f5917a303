"""The batched descriptor matching of key-frame pairs (csrc/kernels_feature_match.hip, fgo_match_features_batch: one workgroup per
pair, all pairs in one launch) against its numpy restatement (tests/feature_match_reference.py, itself pinned by
tests/test_feature_match_reference_cpu.py).  The VRO library's matching is not in the reference tree: the restatement is the yardstick.

ONE batch of 38 pairs over 18 frames (feature_match_reference.gpu_cases): (N_j, N_i) from {0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128,
129, 255, 256, 257, 600} -- either side of a 16 x 16 tile, of a wave's 64 queries, of the 128-train LDS chunk and of the 256-query
block, N_j != N_i in most pairs -- over one world of 600 points and 100 look-alikes, a tenth of the features without depth (z = 0 or
NaN), a duplicated descriptor in every larger frame (a tie among the trains: the lowest index, best = second; two queries sharing a
best train: the cross-check conflict), rows of all 0 against all 255 (the exact maximum 8 323 200), a frame against itself, frames in
several pairs, guided pairs (one with an un-normalised quaternion) whose gate excludes the planted global nearest neighbour, a guided
pair whose pose sends every projection 40 m away and one that puts every train behind the camera, and three pairs repeated at other
places of the batch.  The batch runs with (ratio_test, cross_check) in all four combinations and once with ratio = 0.8, a cap, a
3-D gate and a wider radius; the results are shared.

Everything is compared EXACTLY: the arithmetic is integer, and the generated gates are decided by a relative margin of 1e-6 (the CPU
test asserts it), five orders above the rounding of the f64 projection.

End to end: frames under a planted pose, 2 mm of noise, descriptor noise, 30 % of the second frame's descriptors swapped (wrong
matches for the registration to reject) and half of the points with a look-alike elsewhere in the frame (which the unguided ratio
test rejects and the gate tells apart: why the guided re-match finds no fewer matches); the match
goes to vro_ransac_batch as it is, and the pose is held to the planted one within the bound the RANSAC restatement's own test holds
it to at that noise (rotation matrix 5e-3, translation 1e-2: tests/test_vro_ransac_reference_cpu.py)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from tests import feature_match_reference as ref

PER_QUERY = ("best", "d1", "d2", "reason")
PER_PAIR = ("status", "n_query", "n_train", "n_matches", "n_ratio", "n_cross")
PACKED = ("ptr", "idx_i", "idx_j", "xyz_i", "xyz_j", "uv_i", "uv_j")


def run(frames, pairs, params, **kw):
    ptr, desc, xyz, uv = ref.pack(frames)
    fj = [p[0] for p in pairs]; fi = [p[1] for p in pairs]
    guided = np.array([p[2] is not None for p in pairs])
    pose = np.array([p[2] if p[2] is not None else np.zeros(7) for p in pairs]).reshape(-1, 7)   # an unguided pair's pose is not read
    return G.match_features_batch(ptr, desc, xyz, uv, fi, fj, pose_ij=pose if guided.any() else None, guided=guided if guided.any() else None,
                                  params=G.match_params(**params), **kw)


@functools.lru_cache(maxsize=None)
def cases():
    frames, pairs, planted = ref.gpu_cases()
    tables = [ref.tables(frames[j], frames[i], pose, **ref.CONFIGS[0]) for j, i, pose in pairs]
    tables4 = [ref.tables(frames[j], frames[i], pose, **ref.CONFIGS[4]) for j, i, pose in pairs]       # its gate differs
    want, got = [], []
    for c, params in enumerate(ref.CONFIGS):
        T = tables4 if c == 4 else tables
        want.append([dict(ref.verdict(t, **params), dist=t["dist"]) for t in T])
        got.append(run(frames, pairs, params, want_dist=True))
    return frames, pairs, want, got


@pytest.mark.parametrize("cfg", range(len(ref.CONFIGS)))
def test_distances_equal_the_reference(cfg):
    frames, pairs, want, got = cases()
    g = got[cfg]
    off = 0
    for k, w in enumerate(want[cfg]):
        d = g["dist"][off:off + w["dist"].size].reshape(w["dist"].shape)
        off += w["dist"].size
        bad = np.argwhere(d != w["dist"])
        assert len(bad) == 0, (k, pairs[k][:2], w["dist"].shape, len(bad), bad[:4].tolist(), d[tuple(bad[0])], w["dist"][tuple(bad[0])])
    assert off == len(g["dist"])
    assert g["dist"].max() == 8323200                             # all 0 against all 255


@pytest.mark.parametrize("cfg", range(len(ref.CONFIGS)))
def test_verdicts_matches_and_counts_equal_the_reference(cfg):
    frames, pairs, want, got = cases()
    g = got[cfg]
    fptr = ref.pack(frames)[0]
    _, _, xyz, uv = ref.pack(frames)
    nq = [len(frames[j]["desc"]) for j, _, _ in pairs]
    assert np.array_equal(g["q_ptr"], np.concatenate([[0], np.cumsum(nq)]))
    seen = np.zeros(6, int)
    for k, w in enumerate(want[cfg]):
        a, b = g["q_ptr"][k], g["q_ptr"][k + 1]
        for f in PER_QUERY:
            assert np.array_equal(g[f][a:b], w[f]), (k, pairs[k][:2], f, np.nonzero(g[f][a:b] != w[f])[0][:5])
        for f in PER_PAIR:
            assert g[f][k] == w[f], (k, pairs[k][:2], f, g[f][k], w[f])
        m0, m1 = g["ptr"][k], g["ptr"][k + 1]
        j, i, _ = pairs[k]
        assert np.array_equal(g["idx_j"][m0:m1], fptr[j] + w["a"]) and np.array_equal(g["idx_i"][m0:m1], fptr[i] + w["b"]), k
        assert g["status"][k] == (G.FGO_FM_TOO_FEW if m1 - m0 < 12 else G.FGO_FM_OK)
        seen += np.bincount(w["reason"], minlength=6)
    assert g["xyz_i"].tobytes() == xyz[g["idx_i"]].tobytes() and g["xyz_j"].tobytes() == xyz[g["idx_j"]].tobytes()
    assert g["uv_i"].tobytes() == uv[g["idx_i"]].tobytes() and g["uv_j"].tobytes() == uv[g["idx_j"]].tobytes()
    assert len(g["idx_i"]) == g["ptr"][-1] == g["n_matches"].sum()
    assert set(g["status"]) == {G.FGO_FM_OK, G.FGO_FM_TOO_FEW}
    print("config %d: %d matches in %d pairs; reasons 0..5: %s" % (cfg, g["ptr"][-1], len(pairs), seen))


def test_two_calls_are_bit_identical_and_a_pair_does_not_depend_on_its_place():
    frames, pairs, want, got = cases()
    for cfg in (0, 4):
        g = got[cfg]
        again = run(frames, pairs, ref.CONFIGS[cfg], want_dist=True)
        for f in PER_QUERY + PER_PAIR + PACKED + ("dist", "q_ptr"):
            assert again[f].tobytes() == g[f].tobytes(), (cfg, f)
        # the repeated pairs: (15, 14) unguided at 0 and 35, guided at 25 and 36; (9, 8) at 6 and 37
        for k, m in ((0, 35), (25, 36), (6, 37)):
            assert pairs[k][:2] == pairs[m][:2] and (pairs[k][2] is None) == (pairs[m][2] is None)
            for f in PER_QUERY:
                assert np.array_equal(g[f][g["q_ptr"][k]:g["q_ptr"][k + 1]], g[f][g["q_ptr"][m]:g["q_ptr"][m + 1]]), (k, m, f)
            for f in PER_PAIR:
                assert g[f][k] == g[f][m], (k, m, f)
            for f in PACKED[1:]:
                assert np.array_equal(g[f][g["ptr"][k]:g["ptr"][k + 1]], g[f][g["ptr"][m]:g["ptr"][m + 1]]), (k, m, f)
        # a pair alone, and the batch reversed
        for k in (0, 25, 21, 33):
            one = run(frames, [pairs[k]], ref.CONFIGS[cfg], want_dist=True)
            for f in PER_QUERY:
                assert np.array_equal(one[f], g[f][g["q_ptr"][k]:g["q_ptr"][k + 1]]), (k, f)
            assert np.array_equal(one["idx_i"], g["idx_i"][g["ptr"][k]:g["ptr"][k + 1]]), k
        rev = run(frames, pairs[::-1], ref.CONFIGS[cfg])
        assert "dist" not in rev
        n = len(pairs)
        for k in range(n):
            r = n - 1 - k
            for f in PER_QUERY:
                assert np.array_equal(rev[f][rev["q_ptr"][r]:rev["q_ptr"][r + 1]], g[f][g["q_ptr"][k]:g["q_ptr"][k + 1]]), (k, f)
            assert rev["n_matches"][r] == g["n_matches"][k]
    assert G.lib.fgo_debug_match_kernel_ms() > 0
    empty = G.match_features_batch([0, 3], np.zeros((3, 128), np.uint8), np.ones((3, 3)), np.ones((3, 2)), [], [])
    assert len(empty["status"]) == 0 and len(empty["idx_i"]) == 0


def test_matches_register_the_planted_pose_and_the_guided_rematch_finds_no_fewer():
    frames, planted = ref.e2e_cases()
    ptr, desc, xyz, uv = ref.pack(frames)
    n = len(planted)
    fi, fj = 2 * np.arange(n), 2 * np.arange(n) + 1
    m = G.match_features_batch(ptr, desc, xyz, uv, fi, fj)
    assert (m["status"] == G.FGO_FM_OK).all() and (m["n_matches"] >= 60).all()
    v = G.vro_ransac_batch(m["ptr"], m["xyz_i"], m["xyz_j"])     # the packed matches go in as they are
    assert (v["status"] == G.FGO_VRO_OK).all(), v["status"]
    for p, (R, t) in enumerate(planted):
        a, b = m["ptr"][p], m["ptr"][p + 1]
        wrong = frames[2 * p + 1]["ids"][m["idx_j"][a:b] - ptr[2 * p + 1]] != frames[2 * p]["ids"][m["idx_i"][a:b] - ptr[2 * p]]
        assert 0.1 < wrong.mean() < 0.5                          # the swapped descriptors did give wrong matches
        assert not (v["inliers"][a:b].astype(bool) & wrong).any() and v["n_inliers"][p] >= 0.9 * (~wrong).sum()
        assert np.abs(ref.quat_matrix(v["pose_ij"][p][3:]) - R).max() < 5e-3 and np.abs(v["pose_ij"][p][:3] - t).max() < 1e-2, p
    adj = G.vro_adjust_batch(ptr, desc, xyz, uv, fi, fj, v["pose_ij"], info=v["info"])
    assert adj["adjusted"].all()
    assert (adj["n_matches"] >= m["n_matches"]).all(), (adj["n_matches"], m["n_matches"])
    for p, (R, t) in enumerate(planted):
        assert np.abs(ref.quat_matrix(adj["pose_ij"][p][3:]) - R).max() < 5e-3 and np.abs(adj["pose_ij"][p][:3] - t).max() < 1e-2, p
    print("unguided matches %s, guided %s" % (m["n_matches"], adj["n_matches"]))
    # a record whose guided match finds nothing is left as it is
    away = v["pose_ij"].copy(); away[:, 0] += 40.0
    left = G.vro_adjust_batch(ptr, desc, xyz, uv, fi, fj, away, info=v["info"])
    assert not left["adjusted"].any() and left["pose_ij"].tobytes() == away.tobytes() and left["info"].tobytes() == v["info"].tobytes()
    assert (left["n_matches"] <= 4).all() and left["vro"] is None
