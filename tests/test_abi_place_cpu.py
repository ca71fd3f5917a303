"""The ctypes binding of place recognition (graph_slam_amd/place.py) held to include/fgo_place.h, without a GPU, the way
tests/test_abi_cpu.py holds _abi.py to include/fgo.h: every prototype against the declaration, every Structure's layout against
what the C compiler makes of the header, the option builders against the library's defaults -- and every argument the header says is
refused before the first HIP call, with the two n_frames == 0 cases."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import graph_slam_amd as G
from graph_slam_amd import place as P
from tests.fgo_header import HEADER, _strip_braces, _type_of

OK, EINVAL, ENODEV = 0, -1, -2                                   # FGO_OK, FGO_EINVAL, FGO_ENODEV of include/fgo.h
PLACE_HEADER = os.path.join(os.path.dirname(HEADER), "fgo_place.h")
STRUCTS = sorted((v for v in vars(P).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure),
                 key=lambda s: s.__name__)
BY_C_NAME = {s.c_name: s for s in STRUCTS}
RETURNS = {"int": C.c_int, "void": None, "double": C.c_double}
VALUES = {"int": C.c_int, "int64_t": C.c_int64}
POINTEES = {"double": C.c_double, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint8_t": C.c_uint8}


def declared_functions():
    """[(return type, name, [parameter types])] of include/fgo_place.h, read as tests/fgo_header.py reads include/fgo.h"""
    src = open(PLACE_HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"^\s*#[^\n]*", "", src, flags=re.M)
    src = _strip_braces(re.sub(r'extern\s+"C"\s*\{', "", src))
    out = []
    for stmt in src.split(";"):
        s = " ".join(stmt.split())
        m = re.match(r"^(.+?)\b(fgo_\w+)\s*\((.*)\)$", s)
        if not s or s.startswith("typedef") or not m:
            continue
        args = m.group(3).strip()
        out.append((m.group(1).strip(), m.group(2), [] if args in ("", "void") else [_type_of(a) for a in args.split(",")]))
    return out


def _ctype_of(param):
    t = param[6:] if param.startswith("const ") else param
    if t in VALUES:
        return VALUES[t]
    assert t.endswith(" *"), param
    base = t[:-2]
    return C.POINTER(POINTEES[base] if base in POINTEES else BY_C_NAME[base])


def test_every_prototype_matches_the_header():
    decl = declared_functions()
    assert len(decl) == 6
    assert list(P.PLACE_PROTOTYPES) == [name for _, name, _ in decl]
    assert not set(P.PLACE_PROTOTYPES) & set(G.PROTOTYPES)
    for ret, name, params in decl:
        fn = getattr(G.lib, name)
        assert fn.restype is RETURNS[ret], name
        assert len(fn.argtypes) == len(params), name
        for k, (p, have) in enumerate(zip(params, fn.argtypes)):
            assert have is _ctype_of(p), "%s, parameter %d: %s in the header, %r in the binding" % (name, k, p, have)


def test_layouts_and_constants_match_the_header(tmp_path):
    assert [s.c_name for s in STRUCTS] == ["fgo_place_params", "fgo_vocab_params", "fgo_vocab_result"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fgo_place.h"', 'int main(void) {']
    for s in STRUCTS:
        lines.append('  printf("%s . %%zu\\n", sizeof(%s));' % (s.c_name, s.c_name))
        for f, _ in s._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s.c_name, f, s.c_name, f))
    lines += ['  printf("FGO_PLACE_MAX_WORDS . %zu\\n", (size_t)FGO_PLACE_MAX_WORDS);',
              '  printf("FGO_PLACE_MAX_TRAIN . %zu\\n", (size_t)FGO_PLACE_MAX_TRAIN);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c_side = {(a, b): int(v) for a, b, v in (l.split() for l in out.splitlines())}
    py_side = {("FGO_PLACE_MAX_WORDS", "."): G.FGO_PLACE_MAX_WORDS, ("FGO_PLACE_MAX_TRAIN", "."): G.FGO_PLACE_MAX_TRAIN}
    for s in STRUCTS:
        py_side[(s.c_name, ".")] = C.sizeof(s)
        for f, _ in s._fields_:
            py_side[(s.c_name, f)] = getattr(s, f).offset
    assert py_side == c_side


def test_option_builders():
    v, p = G.vocab_options(), G.place_options()
    assert type(v) is P.VocabParams and (v.n_words, v.n_iters) == (1024, 10)
    assert type(p) is P.PlaceParams and (p.top_k, p.min_gap, p.min_score, p.max_df_permille) == (5, 10, 0.0, 1000)
    assert G.place_options(top_k=3, min_score=0.25).min_score == 0.25 and G.vocab_options(n_words=7).n_words == 7
    with pytest.raises(TypeError):
        G.place_options(no_such_field=1)
    G.lib.fgo_vocab_params_default(None); G.lib.fgo_place_params_default(None)     # NULL tolerated


# ---- what is refused before the first HIP call --------------------------------------------------------------------------------
def _train(F=8, desc="ok", centres="ok", count="ok", result="ok", **kw):
    d = np.zeros((max(F, 1), 128), np.uint8)
    opts = G.vocab_options(**dict(dict(n_words=4, n_iters=2), **kw))
    v = min(max(opts.n_words, 1), G.FGO_PLACE_MAX_WORDS)
    cen = np.zeros((v, 128), np.uint8); cnt = np.zeros(v, np.int64); res = P.VocabResult()
    pick = lambda flag, x: x if flag == "ok" else None
    return G.lib.fgo_vocab_train(0, F, pick(desc, G.ptr(d)), C.byref(opts), pick(centres, G.ptr(cen)), pick(count, G.ptr(cnt)),
                                 pick(result, C.byref(res)))


def test_vocab_train_refuses_bad_arguments():
    for kw in (dict(desc=None), dict(centres=None), dict(count=None), dict(result=None), dict(n_words=0), dict(n_words=-3),
               dict(n_words=G.FGO_PLACE_MAX_WORDS + 1, F=G.FGO_PLACE_MAX_WORDS + 8), dict(F=3), dict(F=0), dict(n_iters=-1)):
        assert _train(**kw) == EINVAL, kw
    assert G.lib.fgo_vocab_train(0, G.FGO_PLACE_MAX_TRAIN + 1, G.ptr(np.zeros((1, 128), np.uint8)), None,
                                 G.ptr(np.zeros((1024, 128), np.uint8)), G.ptr(np.zeros(1024, np.int64)), C.byref(P.VocabResult())) == EINVAL
    assert _train() in (OK, ENODEV)                   # the same call with nothing wrong gets as far as the device


def _query(fp=(0, 2, 3), V=4, weights=None, missing=(), pairs=(True, True), **kw):
    fp = np.asarray(fp, np.int64)
    n = len(fp) - 1
    d = np.zeros((4, 128), np.uint8); cen = np.zeros((max(min(V, G.FGO_PLACE_MAX_WORDS), 1), 128), np.uint8)
    opts = G.place_options(**kw)
    k = min(max(opts.top_k, 1), 64)
    cf = np.zeros((n, k), np.int64); cd = np.zeros((n, k), np.int64); cs = np.zeros((n, k))
    pi = np.zeros(n * k, np.int64); pj = np.zeros(n * k, np.int64); m = np.full(1, -7, np.int64)
    q = None if weights is None else np.asarray(weights, np.int32)
    a = dict(feat_ptr=G.ptr(fp), desc=G.ptr(d), centres=G.ptr(cen), cf=G.ptr(cf), cd=G.ptr(cd), cs=G.ptr(cs))
    for name in missing:
        a[name] = None
    rc = G.lib.fgo_place_query_batch(0, n, a["feat_ptr"], a["desc"], V, a["centres"], G.opt(q), C.byref(opts), None, None, None, None, None,
                                     None, a["cf"], a["cd"], a["cs"], G.ptr(pi) if pairs[0] else None, G.ptr(pj) if pairs[1] else None,
                                     G.ptr(m), None)
    return rc, int(m[0])


def test_place_query_refuses_bad_arguments():
    nan = float("nan")
    bad = [dict(missing=(name,)) for name in ("feat_ptr", "desc", "centres", "cf", "cd", "cs")]
    bad += [dict(fp=(-1, 2, 3)), dict(fp=(0, 3, 2)), dict(fp=(0, G.FGO_FM_MAX_FEATURES + 1)), dict(V=0), dict(V=G.FGO_PLACE_MAX_WORDS + 1),
            dict(top_k=0), dict(top_k=65), dict(min_gap=0), dict(min_score=-0.1), dict(min_score=1.5), dict(min_score=nan),
            dict(max_df_permille=-1), dict(max_df_permille=1001), dict(weights=[0, 1, -1, 2]), dict(weights=[0, 1, 65536, 2]),
            dict(pairs=(True, False)), dict(pairs=(False, True))]
    for kw in bad:
        assert _query(**kw)[0] == EINVAL, kw
    assert G.lib.fgo_place_query_batch(0, -1, *[None] * 2, 4, *[None] * 16) == EINVAL
    assert _query()[0] in (OK, ENODEV)
    assert _query(weights=[0, 65535, 1, 2], top_k=64, min_score=1.0, max_df_permille=0)[0] in (OK, ENODEV)


def test_no_frames_is_ok_without_a_device():
    assert _query(fp=(0,)) == (OK, 0)                       # *n_pairs_out is written
    assert G.lib.fgo_place_query_batch(0, 0, None, None, 4, *[None] * 16) == OK           # nothing is read
    out = G.place_query_batch([0], np.zeros((0, 128), np.uint8), np.zeros((4, 128), np.uint8), want_words=True, want_dot=True)
    assert len(out["frame_i"]) == len(out["frame_j"]) == 0 and out["cand_frame"].shape == (0, 5) and out["dot_matrix"].shape == (0, 0)
