"""Numpy restatement of fgo_vocab_train and fgo_place_query_batch (include/fgo_place.h), written from the semantics stated there:
the yardstick of tests/test_gpu_place.py, itself pinned to a per-element brute force by tests/test_place_reference_cpu.py.  A
bag-of-words retrieval is not in the reference tree; the definition is this project's.

  distance    d(a, b) = sum_k (a[k] - b[k])^2 from the differences themselves, in integers, dense; assign = argmin (the first of a
              tie: the lowest word)
  train       init: descriptor floor(w F / V); Lloyd iterations with np.add.at sums and floor((2 sum + n) / (2 n)); an empty word
              keeps its centre
  query       counts by np.add.at, v = c q and dot = v v^T in int64, s = dot / sqrt(norm2_a norm2_b) in f64, the candidates of a frame
              by np.lexsort on (s descending, b ascending) over its database b <= a - min_gap
The default weights go through numpy's log2 and may differ by one from the library's (the C library's log2) where N / df is no power
of two: every comparison of scores passes the table one side returned to the other side."""
import numpy as np

from tests import feature_match_reference as fm

DIM = 128
MAX_WORDS = 16384
VOCAB_DEFAULTS = dict(n_words=1024, n_iters=10)
PLACE_DEFAULTS = dict(top_k=5, min_gap=10, min_score=0.0, max_df_permille=1000)


def distances(a, b):
    """len(a) x len(b) int64, a block of rows at a time"""
    a = np.asarray(a, np.uint8).reshape(-1, DIM).astype(np.int32); b = np.asarray(b, np.uint8).reshape(-1, DIM).astype(np.int32)
    out = np.zeros((len(a), len(b)), np.int64)
    step = max(1, (1 << 22) // max(len(b) * DIM, 1))
    for r in range(0, len(a), step):
        e = a[r:r + step, None, :] - b[None, :, :]
        out[r:r + step] = (e * e).sum(2)
    return out


def assign(desc, centres):
    """(word, d) per feature: the nearest centre, the lowest index of a tie"""
    D = distances(desc, centres)
    w = D.argmin(1) if len(D) else np.zeros(0, np.int64)
    return w.astype(np.int32), D[np.arange(len(D)), w].astype(np.int32)


def train(desc, **params):
    P = dict(VOCAB_DEFAULTS, **params)
    desc = np.asarray(desc, np.uint8).reshape(-1, DIM)
    F, V = len(desc), P["n_words"]
    centres = desc[(np.arange(V, dtype=np.int64) * F) // V].copy()
    out = dict(iterations=0, converged=0, changed_last=-1)
    prev = None
    for it in range(P["n_iters"]):
        word, d = assign(desc, centres)
        out["changed_last"] = F if it == 0 else int((word != prev).sum())
        if out["changed_last"] == 0:
            out["converged"] = 1
            break
        sums = np.zeros((V, DIM), np.int64); n = np.zeros(V, np.int64)
        np.add.at(sums, word, desc.astype(np.int64)); np.add.at(n, word, 1)
        has = n > 0
        centres[has] = ((2 * sums[has] + n[has, None]) // (2 * n[has, None])).astype(np.uint8)
        prev = word
        out["iterations"] += 1
    word, d = assign(desc, centres)
    count = np.bincount(word, minlength=V).astype(np.int64)
    out.update(centres=centres, count=count, inertia=int(d.astype(np.int64).sum()), n_empty=int((count == 0).sum()), word=word)
    return out


def default_weights(df, n_frames, max_df_permille=1000):
    df = np.asarray(df, np.int64)
    q = np.zeros(len(df), np.int32)
    keep = (df > 0) & (1000 * df <= max_df_permille * n_frames)
    q[keep] = np.floor(256.0 * np.log2(float(n_frames) / df[keep].astype(np.float64))).astype(np.int32)
    return q


def query(feat_ptr, desc, centres, weights=None, **params):
    P = dict(PLACE_DEFAULTS, **params)
    fp = np.asarray(feat_ptr, np.int64)
    N, V, K = len(fp) - 1, len(centres), P["top_k"]
    desc = np.asarray(desc, np.uint8).reshape(-1, DIM)[:fp[-1]]
    word, word_d = assign(desc, centres)
    frame = np.repeat(np.arange(N), np.diff(fp))
    c = np.zeros((N, V), np.int64)
    np.add.at(c, (frame, word[fp[0]:]), 1)
    df = (c > 0).sum(0).astype(np.int32)
    q = default_weights(df, N, P["max_df_permille"]) if weights is None else np.asarray(weights, np.int32)
    v = c * q.astype(np.int64)
    full = v @ v.T                                              # int64, exact: the bounds are in the header
    norm2 = np.diagonal(full).copy() if N else np.zeros(0, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = full.astype(np.float64) / np.sqrt(norm2[:, None].astype(np.float64) * norm2[None, :].astype(np.float64))
    s[(norm2 == 0)[:, None] | (norm2 == 0)[None, :]] = 0.0
    b_of = np.arange(N)
    in_db = b_of[None, :] <= b_of[:, None] - P["min_gap"]
    cf = np.full((N, K), -1, np.int64); cd = np.zeros((N, K), np.int64); cs = np.zeros((N, K)); nc = np.zeros(N, np.int32)
    ranked = []
    for a in range(N):
        b = np.nonzero(in_db[a] & (full[a] > 0) & (s[a] >= P["min_score"]))[0]
        b = b[np.lexsort((b, -s[a, b]))]
        ranked.append(b)
        k = min(K, len(b))
        cf[a, :k] = b[:k]; cd[a, :k] = full[a, b[:k]]; cs[a, :k] = s[a, b[:k]]; nc[a] = k
    kept = cf >= 0
    return dict(word=word, word_d=word_d, df=df, weights=q, norm2=norm2, n_cand=nc, cand_frame=cf, cand_dot=cd, cand_score=cs,
                frame_i=cf[kept], frame_j=np.repeat(np.arange(N), nc).astype(np.int64), dot_matrix=np.where(in_db, full, -1), score_matrix=s,
                ranked=ranked, counts=c)


# ---- generated cases ------------------------------------------------------------------------------------------------------------

TRAJECTORY = dict(n_places=24, n_features=40, window=60, advance=30, desc_noise=8, n_words=256, min_gap=10, top_k=3)
_cache = {}


def planted_trajectory(seed=20270):
    """24 places visited twice: frame f looks at place f % 24, whose landmarks are the window [30 p, 30 p + 60) of one world; a
    frame sees 40 of them with descriptor noise +-8 and 2 mm on the points, under a pose of its own (feature_match_reference's
    make_world / make_frame: the frames carry points, so a retrieved pair can be matched and registered).  Returns (frames,
    feat_ptr, desc, xyz, uv)."""
    if seed in _cache:
        return _cache[seed]
    T = TRAJECTORY
    rng = np.random.default_rng(seed)
    world = fm.make_world(rng, T["advance"] * (T["n_places"] - 1) + T["window"], 0)
    frames = []
    for f in range(2 * T["n_places"]):
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        pose = (fm.so3_exp(0.1 * axis), rng.uniform(-0.1, 0.1, 3))
        ids = T["advance"] * (f % T["n_places"]) + rng.permutation(T["window"])[:T["n_features"]]
        frames.append(fm.make_frame(rng, world, pose, ids, desc_noise=T["desc_noise"]))
    _cache[seed] = (frames,) + fm.pack(frames)
    return _cache[seed]
