"""The ctypes binding (graph_slam_amd/_abi.py) held to include/fgo.h, without a GPU: every prototype against the declaration, every
Structure's layout against what the C compiler makes of the header, and the helpers that read structs out and fill parameter
structs in."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import graph_slam_amd as G
from graph_slam_amd import _abi as A
from tests.fgo_header import HEADER, declared_functions

STRUCTS = sorted((v for v in vars(A).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure),
                 key=lambda s: s.__name__)
BY_C_NAME = {s.c_name: s for s in STRUCTS}

# ---- (a) prototypes ----------------------------------------------------------------------------------------------------------
RETURNS = {"int": C.c_int, "void": None, "double": C.c_double, "int64_t": C.c_int64, "const char *": C.c_char_p, "fgo_ctx *": C.c_void_p}
VALUES = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double, "char *": C.c_char_p, "void *": C.c_void_p,
          "fgo_ctx *": C.c_void_p, "fgo_allreduce_fn": A.ALLREDUCE_FN}
POINTEES = {"double": C.c_double, "int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int, "int8_t": C.c_int8, "uint8_t": C.c_uint8,
            "unsigned char": C.c_uint8, "uint16_t": C.c_uint16}
# the only excuses: two structs that are nothing but doubles travel as the numpy arrays the callers keep them in
# (Preintegrator.buf, preint_batch's rows; the IMU parameters); test_layouts_match_the_header pins their sizes to that
ALIASES = {"fgo_preint": C.c_double, "fgo_imu_params": C.c_double}


def _ctype_of(param):
    t = param[6:] if param.startswith("const ") else param
    if t in VALUES:
        return VALUES[t]
    assert t.endswith(" *"), "a parameter type the header did not use before: %r" % param
    base = t[:-2]
    if base in POINTEES:
        return C.POINTER(POINTEES[base])
    if base in ALIASES:
        return C.POINTER(ALIASES[base])
    assert base in BY_C_NAME, "no Structure of the binding has the C name %r" % base
    return C.POINTER(BY_C_NAME[base])


def test_every_prototype_matches_the_header():
    decl = declared_functions()
    assert len(decl) == 111                     # a parser that silently matches less fails here; a new function moves this
    assert len({name for _, name, _ in decl}) == len(decl)
    assert sorted(A.PROTOTYPES) == sorted(name for _, name, _ in decl)
    for ret, name, params in decl:
        fn = getattr(G.lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        assert fn.restype is RETURNS[ret], "%s returns %s, the binding says %r" % (name, ret, fn.restype)
        for k, (p, have) in enumerate(zip(params, fn.argtypes)):
            assert have is _ctype_of(p), "%s, parameter %d: %s in the header, %r in the binding" % (name, k, p, have)


# ---- (b) layouts -------------------------------------------------------------------------------------------------------------
def test_layouts_match_the_header(tmp_path):
    assert len(STRUCTS) == 28 and len(BY_C_NAME) == 28
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fgo.h"', 'int main(void) {']
    for s in STRUCTS:
        lines.append('  printf("%s . %%zu\\n", sizeof(%s));' % (s.c_name, s.c_name))
        for f, _ in s._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s.c_name, f, s.c_name, f))
    for name in ALIASES:
        lines.append('  printf("%s . %%zu\\n", sizeof(%s));' % (name, name))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c_side = {(a, b): int(v) for a, b, v in (l.split() for l in out.splitlines())}
    py_side = {}
    for s in STRUCTS:
        py_side[(s.c_name, ".")] = C.sizeof(s)
        for f, _ in s._fields_:
            py_side[(s.c_name, f)] = getattr(s, f).offset
    py_side[("fgo_preint", ".")] = 8 * G.PREINT_DOUBLES
    py_side[("fgo_imu_params", ".")] = 8 * G.IMU_PARAM_DOUBLES
    assert py_side == c_side, sorted(k for k in c_side if py_side.get(k) != c_side[k])


# ---- (c) records -------------------------------------------------------------------------------------------------------------
def _fill(arr):
    """a distinct value in every (record, field, element) of a ctypes struct array, through attribute access"""
    count = 0
    for rec in arr:
        for f, t in rec._fields_:
            n = t._length_ if issubclass(t, C.Array) else 1
            base = t._type_ if issubclass(t, C.Array) else t
            vals = []
            for _ in range(n):
                count += 1
                vals.append(count + 0.25 if base is C.c_double else count % 251 if C.sizeof(base) == 1 else count)
            setattr(rec, f, t(*vals) if issubclass(t, C.Array) else vals[0])


def _read(arr, f):
    return [list(getattr(rec, f)) if hasattr(getattr(rec, f), "_length_") else getattr(rec, f) for rec in arr]


@pytest.mark.parametrize("struct", STRUCTS, ids=lambda s: s.__name__)
def test_records_reads_what_attribute_access_reads(struct):
    arr = (struct * 3)()
    _fill(arr)
    want = {f: _read(arr, f) for f, _ in struct._fields_ if f != "reserved"}
    cols = A.records(arr, 3)
    assert list(cols) == list(want)                             # the fields in their order, no `reserved`
    raw = np.frombuffer(arr, np.uint8)
    for f, col in cols.items():
        assert col.shape[0] == 3 and col.tolist() == want[f], f
        assert col.flags.owndata and not np.shares_memory(col, raw), f
    C.memset(arr, 0, C.sizeof(arr))                             # the columns are copies: the buffer may go
    for f, col in cols.items():
        assert col.tolist() == want[f], f
    assert all(len(col) == 2 for col in A.records(arr, 2).values())


def test_records_shape_and_single_results():
    arr = (G.PlaneExtractPlane * 6)()
    _fill(arr)
    flat, grid = A.records(arr, 6), A.records(arr, 6, (2, 3))
    assert grid["rmse"].shape == (2, 3) and grid["centroid"].shape == (2, 3, 3)
    for f in flat:
        assert grid[f].flags.owndata and grid[f].flags.c_contiguous
        np.testing.assert_array_equal(grid[f].reshape(flat[f].shape), flat[f])
    res = G.MapCleanResult()
    res.n_kept, res.floor_height = 7, 0.5
    d = A.fields(res)
    assert list(d) == [f for f, _ in G.MapCleanResult._fields_]
    assert type(d["n_kept"]) is int and d["n_kept"] == 7 and type(d["floor_height"]) is float and d["floor_height"] == 0.5


# ---- (d) params --------------------------------------------------------------------------------------------------------------
PARAM_FUNCS = sorted(n for n, v in vars(G).items() if n.endswith("_params") and callable(v) and not isinstance(v, type))


def test_there_is_a_params_function_per_params_struct():
    assert len(PARAM_FUNCS) == 11
    assert sorted("fgo_" + n for n in PARAM_FUNCS) == sorted(s.c_name for s in STRUCTS if s.c_name.endswith("_params"))


def _bytes(p):
    return bytes(memoryview(p).cast("B"))


@pytest.mark.parametrize("name", PARAM_FUNCS)
def test_params_builder(name):
    struct = BY_C_NAME["fgo_" + name]
    make = getattr(G, name)
    default = struct()
    for f, t in struct._fields_:                                # poison, so that the library's defaults have to be written
        setattr(default, f, t(*[1] * t._length_) if issubclass(t, C.Array) else 1)
    getattr(G.lib, struct.c_name + "_default")(C.byref(default))
    p = make()
    assert type(p) is struct and _bytes(p) == _bytes(default)
    for f, t in struct._fields_:
        if issubclass(t, C.Array):
            seq = [k + 2 for k in range(t._length_)]
            for v in (seq, tuple(seq), np.array(seq)):
                assert list(getattr(make(**{f: v}), f)) == seq, f
        else:
            q = make(**{f: 3})
            assert getattr(q, f) == 3 and type(getattr(q, f)) is type(getattr(default, f)), f
            setattr(q, f, getattr(default, f))
            assert _bytes(q) == _bytes(default), f              # nothing else moved
    with pytest.raises(TypeError) as ei:
        make(no_such_field=1)
    assert struct.c_name in str(ei.value) and "no_such_field" in str(ei.value)


def test_the_array_fields_are_the_four_the_wrappers_document():
    arrays = {f for s in STRUCTS if s.c_name.endswith("_params") for f, t in s._fields_ if issubclass(t, C.Array)}
    assert arrays == {"sigma_z", "rect", "viewpoint", "background"}
