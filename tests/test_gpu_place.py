"""Place recognition by visual words (csrc/kernels_place.hip: fgo_vocab_train, fgo_place_query_batch) against its numpy restatement
(tests/place_reference.py, itself pinned to brute force by tests/test_place_reference_cpu.py).  A bag-of-words retrieval is not in
the reference tree: the restatement is the yardstick.

Everything is compared EXACTLY -- the arithmetic is integer up to the score, and the score is one multiply, one square root and one
divide in f64, each correctly rounded on both sides -- except the default weights, which go through two C libraries' log2: they are
equal where N / df is a power of two and within one elsewhere, and every comparison of scores hands the table the device returned to
the restatement.

  assign    F in {1, 17, 255, 256, 257, 600} against V in {1, 2, 15, 16, 17, 127, 128, 129, 257}: either side of a 16 x 16 tile, of a
            wave's 64 features, of the 128-centre LDS chunk and of the 256-feature block; a duplicated centre (the lowest index
            wins), a descriptor equal to a centre (d = 0), all 0 against all 255 (8 323 200).
  training  F = 600 with V in {1, 16, 129}; more words than distinct descriptors (empty words keep their centre), a two-member word
            whose byte sum is odd, convergence before n_iters, n_iters = 0.
  query     40 frames of 0, 1, 2, 63, 64, 65 and 300 features; see scene() and the tests.  One more call at the cap, V = 16384:
            the histogram's 32 KB of counters and the scoring's 64 KB table.
  end to end  the planted trajectory of the CPU test: train, query, match_features_batch, vro_ransac_batch."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from tests import feature_match_reference as fm
from tests import place_reference as ref

F_SIZES = (1, 17, 255, 256, 257, 600)
V_SIZES = (1, 2, 15, 16, 17, 127, 128, 129, 257)
QUERY_KEYS = ("df", "norm2", "n_cand", "cand_frame", "cand_dot", "cand_score", "frame_i", "frame_j", "dot_matrix")


def clustered(seed, n, n_clusters, noise=20):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n_clusters, 128))
    return np.clip(base[rng.integers(0, n_clusters, n)] + rng.integers(-noise, noise + 1, (n, 128)), 0, 255).astype(np.uint8)


def words_of(desc, centres):
    """the device's assignment of desc, through a one-frame query (nothing to retrieve)"""
    out = G.place_query_batch([0, len(desc)], desc, centres, want_words=True)
    assert out["n_cand"].tolist() == [0] and len(out["frame_i"]) == 0
    return out["word"], out["word_d"]


# ---- assign -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", V_SIZES)
def test_assign_equals_the_reference(V):
    desc = clustered(31, 600, 40)
    cen = clustered(32, V, 40)
    cen[0] = desc[0]                                             # a descriptor equal to a centre: d = 0
    if V > 1:
        cen[V - 1] = cen[0]                                      # a duplicated centre: the lowest index wins
        cen[V // 2] = desc[599]
    for F in F_SIZES:
        w, d = words_of(desc[:F], cen)
        rw, rd = ref.assign(desc[:F], cen)
        assert np.array_equal(w, rw) and np.array_equal(d, rd), (F, V, np.nonzero(w != rw)[0][:5], np.nonzero(d != rd)[0][:5])
        assert w.dtype == np.int32 and d[0] == 0 and w[0] == 0 and (V == 1 or V - 1 not in w or V // 2 == V - 1)


def test_assign_reaches_the_largest_distance():
    desc = np.zeros((2, 128), np.uint8); desc[1] = 255
    w, d = words_of(desc, np.full((1, 128), 255, np.uint8))
    assert w.tolist() == [0, 0] and d.tolist() == [8323200, 0]
    w, d = words_of(desc, np.array([[255] * 128, [0] * 128, [0] * 128], np.uint8))
    assert w.tolist() == [1, 0] and d.tolist() == [0, 0]


# ---- training -----------------------------------------------------------------------------------------------------------------
TRAIN_KEYS = ("iterations", "converged", "changed_last", "inertia", "n_empty")


def check_training(desc, **kw):
    got = G.vocab_train(desc, G.vocab_options(**kw))
    want = ref.train(desc, **kw)
    assert np.array_equal(got["centres"], want["centres"]), (kw, np.argwhere(got["centres"] != want["centres"])[:5])
    assert np.array_equal(got["count"], want["count"]) and got["count"].dtype == np.int64 and got["count"].sum() == len(desc)
    for k in TRAIN_KEYS:
        assert got[k] == want[k], (kw, k, got[k], want[k])
    return got


@pytest.mark.parametrize("V", (1, 16, 129))
def test_training_equals_the_reference(V):
    desc = clustered(41, 600, 24)
    got = check_training(desc, n_words=V, n_iters=10)
    assert got["iterations"] >= 1 and got["n_empty"] == 0
    check_training(desc, n_words=V, n_iters=1)
    zero = check_training(desc, n_words=V, n_iters=0)
    assert zero["iterations"] == 0 and zero["converged"] == 0 and zero["changed_last"] == -1
    assert np.array_equal(zero["centres"], desc[(np.arange(V) * 600) // V])
    again = G.vocab_train(desc, G.vocab_options(n_words=V, n_iters=10))
    assert all(np.array_equal(again[k], got[k]) for k in ("centres", "count") + TRAIN_KEYS)       # two calls are bit-identical
    assert G.lib.fgo_debug_place_kernel_ms() > 0


def test_training_edge_cases():
    # more words than distinct descriptors: the duplicates among the initial centres tie, the higher ones stay empty and keep their centre
    few = np.tile(clustered(42, 8, 8), (75, 1))
    got = check_training(few, n_words=16, n_iters=10)
    assert got["n_empty"] == 8 and got["converged"] == 1 and got["inertia"] == 0
    assert np.array_equal(got["centres"], few[(np.arange(16) * 600) // 16])
    # a two-member word whose byte sum is odd rounds up
    two = np.zeros((2, 128), np.uint8); two[1] = 1; two[1, 5] = 254; two[0, 5] = 255
    got = check_training(two, n_words=1, n_iters=1)
    assert got["centres"][0, 0] == 1 and got["centres"][0, 5] == 255 and got["count"].tolist() == [2]
    # convergence before n_iters: well separated clusters
    got = check_training(clustered(43, 600, 6, noise=4), n_words=16, n_iters=40)
    assert got["converged"] == 1 and got["changed_last"] == 0 and got["iterations"] < 40
    # permuting descriptors that do not move the initial picks changes nothing
    desc = clustered(41, 600, 24)
    base = G.vocab_train(desc, G.vocab_options(n_words=16, n_iters=10))
    picks = (np.arange(16) * 600) // 16
    rest = np.setdiff1d(np.arange(600), picks)
    perm = np.arange(600); perm[rest] = rest[np.random.default_rng(5).permutation(len(rest))]
    moved = G.vocab_train(desc[perm], G.vocab_options(n_words=16, n_iters=10))
    assert all(np.array_equal(moved[k], base[k]) for k in ("centres", "count") + TRAIN_KEYS)


# ---- query --------------------------------------------------------------------------------------------------------------------
N_FRAMES = 40
SIZES = [(63, 64, 65, 300, 2, 64, 1, 65, 0, 63)[f % 10] for f in range(N_FRAMES)]
ZERO_FRAME = 4                                                   # two features: config "explicit" gives its words the weight 0


@functools.lru_cache(maxsize=None)
def scene():
    """40 frames over one world of 500 landmarks: frame f looks at place f % 13 (a revisit is 13 frames back, behind min_gap = 10);
    frames 3 and 20 are frame 2 again, byte for byte: two identical database frames, and a query that scores 1 against both"""
    rng = np.random.default_rng(20271)
    world = rng.integers(0, 256, (500, 128))
    frames = []
    for f, n in enumerate(SIZES):
        ids = (30 * (f % 13) + rng.permutation(max(100, n))[:n]) % 500
        frames.append(np.clip(world[ids] + rng.integers(-8, 9, (n, 128)), 0, 255).astype(np.uint8))
    frames[3] = frames[2].copy(); frames[20] = frames[2].copy()
    fp = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    desc = np.concatenate(frames)
    centres = ref.train(desc, n_words=129, n_iters=3)["centres"]
    return fp, desc, centres


def run_query(weights=None, frames=None, **kw):
    fp, desc, centres = scene()
    if frames is not None:
        desc = np.concatenate([desc[fp[f]:fp[f + 1]] for f in frames] + [np.zeros((0, 128), np.uint8)])
        fp = np.concatenate([[0], np.cumsum([fp[f + 1] - fp[f] for f in frames])]).astype(np.int64)
    got = G.place_query_batch(fp, desc, centres, weights=weights, options=G.place_options(**kw), want_words=True, want_dot=True)
    want = ref.query(fp, desc, centres, weights=got["weights"], **kw)                # the table the device used
    return got, want


def assert_equal(got, want, what):
    for k in ("word", "word_d") + QUERY_KEYS:
        assert got[k].dtype == want[k].dtype or k in ("frame_i", "frame_j"), (what, k, got[k].dtype, want[k].dtype)
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:5].tolist())
    kept = got["cand_frame"] >= 0
    assert np.array_equal(got["frame_i"], got["cand_frame"][kept]) and np.array_equal(got["frame_j"], np.nonzero(kept)[0])
    assert np.array_equal(got["score"], got["cand_score"][kept]) and np.array_equal(got["dot"], got["cand_dot"][kept])
    assert np.array_equal(kept.sum(1), got["n_cand"])


@functools.lru_cache(maxsize=None)
def default_run():
    return run_query()


def explicit_weights():
    _, want = default_run()
    rng = np.random.default_rng(7)
    q = rng.integers(0, 300, 129).astype(np.int32)
    q[rng.permutation(129)[:10]] = 0
    fp = scene()[0]
    busiest = np.bincount(want["word"], minlength=129).argmax()
    q[busiest] = 65535
    q[want["word"][fp[ZERO_FRAME]:fp[ZERO_FRAME + 1]]] = 0
    return q


def test_default_weights_and_candidates_equal_the_reference():
    got, want = default_run()
    assert_equal(got, want, "default")
    fp, desc, centres = scene()
    mine = ref.default_weights(got["df"], N_FRAMES)
    assert np.abs(got["weights"].astype(np.int64) - mine).max() <= 1
    pow2 = np.isin(got["df"], (5, 10, 20, 40))                   # 40 / df a power of two
    assert pow2.any() and np.array_equal(got["weights"][pow2], mine[pow2]) and (got["weights"][got["df"] == 40] == 0).all()
    # an empty frame has no candidates and is never one; frames 2 and 3 are identical: frame 20 scores 1 against both, the lower first
    empty = SIZES.index(0)
    assert got["norm2"][empty] == 0 and got["n_cand"][empty] == 0 and empty not in got["cand_frame"]
    assert got["cand_frame"][20, :2].tolist() == [2, 3] and got["cand_score"][20, :2].tolist() == [1.0, 1.0]
    assert (got["n_cand"][:10] == 0).all() and (got["dot_matrix"][:10] == -1).all() and got["n_cand"].max() == 5
    # every revisit (13 frames back) of a frame with enough features is retrieved
    for f in range(13, N_FRAMES):
        if min(SIZES[f], SIZES[f - 13]) >= 63 and not {f, f - 13} & {3, 20}:      # those two show place 2
            assert f - 13 in got["cand_frame"][f], f
    assert G.lib.fgo_debug_place_kernel_ms() > 0
    parts = np.zeros(3); G.lib.fgo_debug_place_phase_ms(G.ptr(parts))
    assert (parts > 0).all() and abs(parts.sum() - G.lib.fgo_debug_place_kernel_ms()) < 1e-9


def test_explicit_weights_with_zero_and_the_largest():
    q = explicit_weights()
    assert q.min() == 0 and q.max() == 65535
    got, want = run_query(weights=q, top_k=3, min_gap=1)
    assert np.array_equal(got["weights"], q)
    assert_equal(got, want, "explicit")
    # a frame of only zero-weight words: norm 0, no candidates, never a candidate
    assert got["norm2"][ZERO_FRAME] == 0 and got["n_cand"][ZERO_FRAME] == 0 and ZERO_FRAME not in got["cand_frame"]
    assert (got["dot_matrix"][ZERO_FRAME, :ZERO_FRAME] == 0).all() and got["norm2"].max() > 2 ** 40
    assert got["n_cand"][0] == 0 and got["n_cand"][1] <= 1 and got["n_cand"].max() == 3


def test_top_k_larger_than_the_database_and_a_score_cut():
    w = default_run()[0]["weights"]
    got, want = run_query(weights=w, top_k=64, min_gap=2)
    assert_equal(got, want, "top_k 64")
    assert got["cand_frame"].shape == (N_FRAMES, 64) and got["n_cand"].max() <= N_FRAMES - 2 and got["n_cand"].max() >= 30
    assert (np.diff(got["cand_score"], axis=1) <= 0).all()
    # a min_score between two known scores of one frame: the higher stays, the lower goes
    a = int(np.argmax(got["n_cand"] >= 2))
    s1, s2 = got["cand_score"][a, :2]
    later = [r for r in range(1, got["n_cand"][a]) if got["cand_score"][a, r] < s1]
    s2 = got["cand_score"][a, later[0]]
    cut = 0.5 * (s1 + s2)
    assert s2 < cut < s1
    g2, w2 = run_query(weights=w, top_k=64, min_gap=2, min_score=cut)
    assert_equal(g2, w2, "min_score")
    assert g2["n_cand"][a] == later[0] and (g2["cand_score"][g2["cand_frame"] >= 0] >= cut).all()
    assert g2["n_cand"].sum() < got["n_cand"].sum()
    assert np.array_equal(g2["dot_matrix"], got["dot_matrix"])   # the cut does not touch the dots


def test_stop_words_at_the_boundary():
    base = default_run()[0]
    df = base["df"]
    d = next(int(x) for x in range(1, N_FRAMES) if (df == x).any() and (df == x + 1).any())
    permille = 25 * d                                            # 1000 d == permille N for N = 40: kept; d + 1: dropped
    got, want = run_query(max_df_permille=permille)
    assert_equal(got, want, "stop words")
    assert np.array_equal(got["df"], df)
    assert (got["weights"][df == d] == base["weights"][df == d]).all() and (got["weights"][df == d] > 0).all()
    assert (got["weights"][df > d] == 0).all() and (got["weights"][df <= d] == base["weights"][df <= d]).all()
    none, want = run_query(max_df_permille=0)
    assert_equal(none, want, "every word a stop word")
    assert (none["weights"] == 0).all() and (none["norm2"] == 0).all() and len(none["frame_i"]) == 0


def test_no_more_frames_than_the_gap():
    got, want = run_query(frames=list(range(10)))
    assert_equal(got, want, "n_frames <= min_gap")
    assert len(got["frame_i"]) == 0 and (got["cand_frame"] == -1).all() and (got["dot_matrix"] == -1).all() and (got["norm2"] > 0).any()
    one, want = run_query(frames=[3], min_gap=1)
    assert_equal(one, want, "one frame")


def test_two_calls_are_bit_identical_and_a_frame_does_not_depend_on_the_batch():
    q = explicit_weights()
    got, _ = run_query(weights=q, top_k=3, min_gap=1)
    again, _ = run_query(weights=q, top_k=3, min_gap=1)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    fp = scene()[0]
    pick = [5, 20, 8, 3, 39]
    sub, want = run_query(weights=q, frames=pick, top_k=3, min_gap=1)
    assert_equal(sub, want, "subset")
    sp = np.concatenate([[0], np.cumsum([fp[f + 1] - fp[f] for f in pick])])
    for k, f in enumerate(pick):
        assert sub["norm2"][k] == got["norm2"][f], f
        for key in ("word", "word_d"):
            assert np.array_equal(sub[key][sp[k]:sp[k + 1]], got[key][fp[f]:fp[f + 1]]), (f, key)


def test_the_largest_vocabulary():
    """V = 16384: 32 KB of counters in the histogram, a 64 KB table in the scoring; words at both ends of the table"""
    rng = np.random.default_rng(9)
    land = rng.integers(0, 256, (48, 128))
    centres = rng.integers(0, 256, (G.FGO_PLACE_MAX_WORDS, 128)).astype(np.uint8)
    centres[np.r_[0:16, 8000:8016, 16368:16384]] = land
    frames = [np.clip(land[(8 * (f % 6) + np.arange(8)) % 48] + rng.integers(-8, 9, (8, 128)), 0, 255).astype(np.uint8) for f in range(12)]
    fp = 8 * np.arange(13, dtype=np.int64)
    desc = np.concatenate(frames)
    got = G.place_query_batch(fp, desc, centres, options=G.place_options(top_k=2, min_gap=3), want_words=True, want_dot=True)
    want = ref.query(fp, desc, centres, weights=got["weights"], top_k=2, min_gap=3)
    assert_equal(got, want, "V = 16384")
    assert got["word"].min() == 0 and got["word"].max() == 16383
    assert [int(got["cand_frame"][f, 0]) for f in range(6, 12)] == list(range(6))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_retrieved_pairs_register_the_planted_poses():
    T = ref.TRAJECTORY
    frames, fp, desc, xyz, uv = ref.planted_trajectory()
    voc = G.vocab_train(desc, G.vocab_options(n_words=T["n_words"], n_iters=10))
    want_voc = ref.train(desc, n_words=T["n_words"], n_iters=10)
    assert np.array_equal(voc["centres"], want_voc["centres"]) and np.array_equal(voc["count"], want_voc["count"])
    assert all(voc[k] == want_voc[k] for k in TRAIN_KEYS)
    got = G.place_query_batch(fp, desc, voc["centres"], options=G.place_options(top_k=T["top_k"], min_gap=T["min_gap"]), want_words=True,
                              want_dot=True)
    assert_equal(got, ref.query(fp, desc, voc["centres"], weights=got["weights"], top_k=T["top_k"], min_gap=T["min_gap"]), "trajectory")
    n = T["n_places"]
    for f in range(n, 2 * n):
        assert f - n in got["cand_frame"][f], (f, got["cand_frame"][f], got["cand_score"][f])
    m = G.match_features_batch(fp, desc, xyz, uv, got["frame_i"], got["frame_j"])          # the pairs go in as they are
    v = G.vro_ransac_batch(m["ptr"], m["xyz_i"], m["xyz_j"])
    true = np.nonzero(got["frame_i"] == got["frame_j"] - n)[0]
    assert len(true) == n
    for p in true:
        i, j = int(got["frame_i"][p]), int(got["frame_j"][p])
        assert m["status"][p] == G.FGO_FM_OK and v["status"][p] == G.FGO_VRO_OK, (i, j, m["n_matches"][p], v["status"][p])
        pose = fm.relative_pose(frames[i]["T"], frames[j]["T"])
        assert np.abs(fm.quat_matrix(v["pose_ij"][p][3:]) - fm.quat_matrix(pose[3:])).max() < 5e-3, (i, j)
        assert np.abs(v["pose_ij"][p][:3] - pose[:3]).max() < 1e-2, (i, j)
    print("scores of the true partners %.3f .. %.3f; matches %d .. %d" % (got["score"][true].min(), got["score"][true].max(),
                                                                        m["n_matches"][true].min(), m["n_matches"][true].max()))
