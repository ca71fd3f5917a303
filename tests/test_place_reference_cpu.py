"""tests/place_reference.py, the yardstick of tests/test_gpu_place.py, pinned without a GPU: against a per-element brute force
written from include/fgo_place.h with Python integers and loops on tiny inputs, and the conditions the GPU test leans on -- the
planted trajectory retrieves every revisit (24 of 24 at one fixed seed; three seeds gave 24 of 24 when the set-up was chosen, top
scores 0.44 to 0.84) with no tie at the cut between rank top_k and rank top_k + 1, and the default weights are exact where N / df is
a power of two."""
import math

import numpy as np

from tests import place_reference as ref


def brute_d(a, b):
    return sum((int(x) - int(y)) ** 2 for x, y in zip(a, b))


def brute_assign(desc, centres):
    words, ds = [], []
    for a in desc:
        best = None
        for w, c in enumerate(centres):
            d = brute_d(a, c)
            if best is None or d < best[0]:                      # strict: the lowest w of a tie
                best = (d, w)
        ds.append(best[0]); words.append(best[1])
    return words, ds


def brute_train(desc, V, n_iters):
    F = len(desc)
    centres = [list(map(int, desc[(w * F) // V])) for w in range(V)]
    it_done, converged, changed_last, prev = 0, 0, -1, None
    for it in range(n_iters):
        words, _ = brute_assign(desc, centres)
        changed_last = F if it == 0 else sum(x != y for x, y in zip(words, prev))
        if changed_last == 0:
            converged = 1
            break
        for w in range(V):
            members = [f for f in range(F) if words[f] == w]
            n = len(members)
            if n:
                centres[w] = [(2 * sum(int(desc[f][k]) for f in members) + n) // (2 * n) for k in range(ref.DIM)]
        prev = words
        it_done += 1
    words, ds = brute_assign(desc, centres)
    count = [words.count(w) for w in range(V)]
    return dict(centres=centres, count=count, iterations=it_done, converged=converged, changed_last=changed_last, inertia=sum(ds),
                n_empty=count.count(0))


def brute_query(fp, desc, centres, q, top_k, min_gap, min_score):
    N, V = len(fp) - 1, len(centres)
    words, _ = brute_assign(desc, centres)
    c = [[0] * V for _ in range(N)]
    for n in range(N):
        for f in range(fp[n], fp[n + 1]):
            c[n][words[f]] += 1
    v = [[c[n][w] * int(q[w]) for w in range(V)] for n in range(N)]
    norm2 = [sum(x * x for x in v[n]) for n in range(N)]
    cands = []
    for a in range(N):
        found = []
        for b in range(0, a - min_gap + 1):
            dot = sum(x * y for x, y in zip(v[a], v[b]))
            s = 0.0 if norm2[a] == 0 or norm2[b] == 0 else float(dot) / math.sqrt(float(norm2[a]) * float(norm2[b]))
            if dot > 0 and s >= min_score:
                found.append((-s, b, dot))
        cands.append(sorted(found)[:top_k])
    df = [sum(c[n][w] > 0 for n in range(N)) for w in range(V)]
    return dict(words=words, df=df, norm2=norm2, cands=cands)


def tiny(seed, F, spread=3):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (spread, ref.DIM))
    return np.clip(base[rng.integers(0, spread, F)] + rng.integers(-20, 21, (F, ref.DIM)), 0, 255).astype(np.uint8)


def test_assign_and_distances_equal_the_brute_force():
    desc, cen = tiny(1, 9), tiny(2, 5)
    cen[3] = cen[1]                                              # a duplicated centre: the lowest index wins
    desc[4] = cen[1]                                             # d = 0
    desc[0] = 0; cen[0] = 255
    w, d = ref.assign(desc, cen)
    bw, bd = brute_assign(desc, cen)
    assert w.tolist() == bw and d.tolist() == bd
    assert w[4] == 1 and d[4] == 0 and 3 not in w
    assert ref.distances(desc[:1], cen[:1])[0, 0] == 8323200 == brute_d(desc[0], cen[0])


def test_training_equals_the_brute_force():
    for seed, F, V, iters in ((3, 30, 4, 10), (4, 30, 4, 1), (5, 12, 12, 3), (6, 20, 1, 2), (7, 16, 5, 0)):
        desc = tiny(seed, F)
        if seed == 5:
            desc[6:] = desc[:6]                                  # more words than distinct descriptors: empty words keep their centre
        got = ref.train(desc, n_words=V, n_iters=iters)
        want = brute_train(desc, V, iters)
        assert got["centres"].tolist() == want["centres"] and got["count"].tolist() == want["count"], seed
        for k in ("iterations", "converged", "changed_last", "inertia", "n_empty"):
            assert got[k] == want[k], (seed, k)
    assert ref.train(tiny(3, 30), n_words=4, n_iters=10)["converged"] == 1
    assert ref.train(tiny(5, 12), n_words=12, n_iters=0)["changed_last"] == -1
    # a two-member word whose byte sum is odd rounds up
    desc = np.zeros((2, ref.DIM), np.uint8); desc[1] = 1
    t = ref.train(desc, n_words=1, n_iters=1)
    assert (t["centres"] == 1).all() and t["count"].tolist() == [2]


def test_query_equals_the_brute_force():
    rng = np.random.default_rng(8)
    sizes = [3, 0, 4, 2, 3, 5, 1, 3, 4, 2]
    fp = np.concatenate([[0], np.cumsum(sizes)])
    desc = tiny(9, int(fp[-1]), spread=4)
    desc[fp[7]:fp[8]] = desc[fp[0]:fp[1]]                        # frame 7 is frame 0 again
    cen = ref.train(desc, n_words=5, n_iters=3)["centres"]
    for q, kw in ((None, dict(top_k=2, min_gap=2)), (rng.integers(0, 9, 5), dict(top_k=3, min_gap=1, min_score=0.6)),
                  (np.array([0, 65535, 1, 0, 7]), dict(top_k=64, min_gap=3))):
        got = ref.query(fp, desc, cen, weights=q, **kw)
        P = dict(ref.PLACE_DEFAULTS, **kw)
        want = brute_query(fp.tolist(), desc, cen, got["weights"], P["top_k"], P["min_gap"], P["min_score"])
        assert got["word"].tolist() == want["words"] and got["df"].tolist() == want["df"] and got["norm2"].tolist() == want["norm2"]
        pairs = []
        for a, cands in enumerate(want["cands"]):
            assert got["n_cand"][a] == len(cands)
            for r, (ms, b, dot) in enumerate(cands):
                assert got["cand_frame"][a, r] == b and got["cand_dot"][a, r] == dot and got["cand_score"][a, r] == -ms, (a, r)
                assert got["dot_matrix"][a, b] == dot
                pairs.append((b, a))
            assert (got["cand_frame"][a, len(cands):] == -1).all() and (got["cand_score"][a, len(cands):] == 0).all()
            assert (got["dot_matrix"][a, max(a - P["min_gap"] + 1, 0):] == -1).all()
        assert list(zip(got["frame_i"].tolist(), got["frame_j"].tolist())) == pairs
    assert ref.query(fp, desc, cen, weights=np.ones(5), top_k=2, min_gap=2)["cand_frame"][7, 0] == 0


def test_default_weights_are_exact_at_powers_of_two():
    df = np.array([0, 1, 2, 4, 8, 16, 3, 5, 16])
    q = ref.default_weights(df, 16)
    assert q[:6].tolist() == [0, 1024, 768, 512, 256, 0] and q[8] == 0
    for d in (3, 5):
        assert abs(int(q[list(df).index(d)]) - math.floor(256.0 * math.log2(16.0 / d))) <= 1
    # the stop-word boundary: 1000 df == permille N is kept, one above is dropped
    q = ref.default_weights(np.array([4, 5]), 16, max_df_permille=250)
    assert q.tolist() == [512, 0]


def test_the_planted_trajectory_retrieves_every_revisit_without_a_tie_at_the_cut():
    T = ref.TRAJECTORY
    frames, fp, desc, xyz, uv = ref.planted_trajectory()
    assert len(frames) == 48 and (np.diff(fp) == 40).all()
    tr = ref.train(desc, n_words=T["n_words"], n_iters=10)
    q = ref.query(fp, desc, tr["centres"], top_k=T["top_k"], min_gap=T["min_gap"])
    n_places = T["n_places"]
    hits = [f for f in range(n_places, 2 * n_places) if f - n_places in q["cand_frame"][f]]
    assert len(hits) == n_places, hits
    for f in range(n_places, 2 * n_places):
        r, s = q["ranked"][f], q["score_matrix"][f]
        assert len(r) <= T["top_k"] or s[r[T["top_k"] - 1]] > s[r[T["top_k"]]], f
    top = q["cand_score"][n_places:, 0]
    print("top scores %.3f .. %.3f, %d iterations" % (top.min(), top.max(), tr["iterations"]))
