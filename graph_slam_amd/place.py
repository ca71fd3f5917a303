"""Place recognition by visual words (include/fgo_place.h): the vocabulary and the loop-closure candidates of every key frame.  The
Structures and prototypes of that header live here, not in _abi (which is held to include/fgo.h alone); tests/test_abi_place_cpu.py
holds them to fgo_place.h."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import FGO_FM_DIM, FgoError, call, fields, lib, opt, ptr

FGO_PLACE_MAX_WORDS = 16384
FGO_PLACE_MAX_TRAIN = 1 << 24


class VocabParams(C.Structure):
    c_name = "fgo_vocab_params"
    _fields_ = [("n_words", C.c_int), ("n_iters", C.c_int)]


class VocabResult(C.Structure):
    c_name = "fgo_vocab_result"
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("changed_last", C.c_int64), ("inertia", C.c_int64),
                ("n_empty", C.c_int64)]


class PlaceParams(C.Structure):
    c_name = "fgo_place_params"
    _fields_ = [("top_k", C.c_int), ("min_gap", C.c_int), ("min_score", C.c_double), ("max_df_permille", C.c_int)]


def _prototypes():
    """{function: argtypes, or (restype, argtypes) where it does not return int}, one entry for every function
    include/fgo_place.h declares and in its order"""
    i, i64, d, P = C.c_int, C.c_int64, C.c_double, C.POINTER
    dp, i64p, i32p, u8p = (P(t) for t in (d, i64, C.c_int32, C.c_uint8))
    return {
        "fgo_vocab_params_default": (None, [P(VocabParams)]),
        "fgo_vocab_train": [i, i64, u8p, P(VocabParams), u8p, i64p, P(VocabResult)],
        "fgo_place_params_default": (None, [P(PlaceParams)]),
        "fgo_place_query_batch": [i, i64, i64p, u8p, i, u8p, i32p, P(PlaceParams), i32p, i32p, i32p, i32p, i64p, i32p, i64p, i64p, dp,
                                  i64p, i64p, i64p, i64p],
        "fgo_debug_place_kernel_ms": (d, []),
        "fgo_debug_place_phase_ms": (None, [dp]),
    }


PLACE_PROTOTYPES = _prototypes()
for _name, _proto in PLACE_PROTOTYPES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _proto if isinstance(_proto, tuple) else (C.c_int, _proto)


def vocab_options(**kw):
    """fgo_vocab_params_default, with the given fields replaced"""
    return _abi.params(VocabParams, **kw)


def place_options(**kw):
    """fgo_place_params_default, with the given fields replaced"""
    return _abi.params(PlaceParams, **kw)


def vocab_train(desc, options=None, device=0):
    """fgo_vocab_train: a vocabulary of options.n_words centres by deterministic integer Lloyd iterations over desc (F x 128 uint8).
    Returns a dict: centres (V x 128 uint8), count (V int64: the members of every word) and the numbers iterations, converged,
    changed_last, inertia, n_empty."""
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, FGO_FM_DIM)
    if options is None:
        options = vocab_options()
    v = min(max(options.n_words, 1), FGO_PLACE_MAX_WORDS)         # a bad argument is the library's to refuse
    centres = np.zeros((v, FGO_FM_DIM), np.uint8); count = np.zeros(v, np.int64)
    res = VocabResult()
    call("fgo_vocab_train", device, len(d), ptr(d), C.byref(options), ptr(centres), ptr(count), C.byref(res))
    out = {"centres": centres, "count": count}
    out.update(fields(res))
    return out


def place_query_batch(feat_ptr, desc, centres, weights=None, options=None, want_words=False, want_dot=False, device=0):
    """fgo_place_query_batch: the loop-closure candidates of every key frame in one call.  Frame n owns the features
    [feat_ptr[n], feat_ptr[n + 1]) of desc (F x 128 uint8); centres (V x 128 uint8) is the vocabulary (vocab_train's `centres`),
    weights (V, 0 .. 65535) the word weights, None = the inverse document frequency of this batch.  Returns a dict of arrays.  The
    pairs, as match_features_batch takes them: frame_i (the old frame), frame_j (the new one), ordered by frame_j and then by rank,
    with score and dot beside them.  Per frame: n_cand, norm2 and, with the stride top_k, cand_frame (-1: none), cand_dot,
    cand_score.  Per word: df and weights (the table used).  With want_words, per feature: word, word_d; with want_dot,
    dot_matrix (N x N int64, -1 outside a frame's database)."""
    fp = np.ascontiguousarray(feat_ptr, np.int64).reshape(-1)
    n = len(fp) - 1
    if n < 0:
        raise FgoError("place_query_batch: feat_ptr needs n_frames + 1 entries")
    F = max(int(fp[-1]), 0)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, FGO_FM_DIM)
    if len(d) < F:
        raise FgoError("place_query_batch: feat_ptr names %d features, desc holds fewer" % F)
    c = np.ascontiguousarray(centres, np.uint8).reshape(-1, FGO_FM_DIM)
    v = len(c)
    q = None if weights is None else np.ascontiguousarray(weights, np.int32).reshape(-1)
    if q is not None and len(q) != v:
        raise FgoError("place_query_batch: weights needs one entry per word")
    if options is None:
        options = place_options()
    k = min(max(options.top_k, 1), 64)
    word = np.zeros(F, np.int32) if want_words else None
    word_d = np.zeros(F, np.int32) if want_words else None
    df = np.zeros(v, np.int32); used = np.zeros(v, np.int32)
    norm2 = np.zeros(n, np.int64); n_cand = np.zeros(n, np.int32)
    cf = np.full((n, k), -1, np.int64); cd = np.zeros((n, k), np.int64); cs = np.zeros((n, k))
    pi = np.zeros(n * k, np.int64); pj = np.zeros(n * k, np.int64); m = np.zeros(1, np.int64)
    dot = np.zeros((n, n), np.int64) if want_dot else None
    call("fgo_place_query_batch", device, n, ptr(fp), ptr(d), v, ptr(c), opt(q), C.byref(options), opt(word), opt(word_d), ptr(df),
         ptr(used), ptr(norm2), ptr(n_cand), ptr(cf), ptr(cd), ptr(cs), ptr(pi), ptr(pj), ptr(m), opt(dot))
    m = int(m[0])
    kept = cf >= 0
    out = {"frame_i": pi[:m], "frame_j": pj[:m], "score": cs[kept], "dot": cd[kept], "n_cand": n_cand, "norm2": norm2, "cand_frame": cf,
           "cand_dot": cd, "cand_score": cs, "df": df, "weights": used}
    if want_words:
        out.update(word=word, word_d=word_d)
    if want_dot:
        out["dot_matrix"] = dot
    return out
