"""The ctypes binding of the dense depth alignment (graph_slam_amd/dense.py) held to include/fgo_dense.h, without a GPU, the way
tests/test_abi_place_cpu.py holds place.py to include/fgo_place.h: every prototype against the declaration, every Structure's
layout against what the C compiler makes of the header, the parameter builder against the library's defaults -- and every argument
the header says is refused before the first HIP call, with the n_pairs == 0 case."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import graph_slam_amd as G
from graph_slam_amd import dense as D
from tests.fgo_header import HEADER, _strip_braces, _type_of

OK, EINVAL, ENODEV = 0, -1, -2                                   # FGO_OK, FGO_EINVAL, FGO_ENODEV of include/fgo.h
DENSE_HEADER = os.path.join(os.path.dirname(HEADER), "fgo_dense.h")
STRUCTS = sorted((v for v in vars(D).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure),
                 key=lambda s: s.__name__)
BY_C_NAME = {s.c_name: s for s in STRUCTS}
RETURNS = {"int": C.c_int, "void": None, "double": C.c_double}
VALUES = {"int": C.c_int, "int64_t": C.c_int64}
POINTEES = {"double": C.c_double, "int64_t": C.c_int64, "uint16_t": C.c_uint16}
CONSTANTS = ("FGO_DA_OK", "FGO_DA_TOO_FEW", "FGO_DA_DEGENERATE", "FGO_DA_NUM", "FGO_DA_MAX_LEVELS", "FGO_DA_MAX_PIXELS")


def declared_functions():
    """[(return type, name, [parameter types])] of include/fgo_dense.h, read as tests/fgo_header.py reads include/fgo.h"""
    src = open(DENSE_HEADER).read()
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
    assert len(decl) == 4
    assert list(D.DENSE_PROTOTYPES) == [name for _, name, _ in decl]
    assert not set(D.DENSE_PROTOTYPES) & (set(G.PROTOTYPES) | set(G.PLACE_PROTOTYPES))
    for ret, name, params in decl:
        fn = getattr(G.lib, name)
        assert fn.restype is RETURNS[ret], name
        assert len(fn.argtypes) == len(params), name
        for k, (p, have) in enumerate(zip(params, fn.argtypes)):
            assert have is _ctype_of(p), "%s, parameter %d: %s in the header, %r in the binding" % (name, k, p, have)


def test_layouts_and_constants_match_the_header(tmp_path):
    assert [s.c_name for s in STRUCTS] == ["fgo_depth_align_params", "fgo_depth_align_result"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fgo_dense.h"', 'int main(void) {']
    for s in STRUCTS:
        lines.append('  printf("%s . %%zu\\n", sizeof(%s));' % (s.c_name, s.c_name))
        for f, _ in s._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s.c_name, f, s.c_name, f))
    lines += ['  printf("%s . %%zu\\n", (size_t)%s);' % (c, c) for c in CONSTANTS] + ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c_side = {(a, b): int(v) for a, b, v in (l.split() for l in out.splitlines())}
    py_side = {(c, "."): getattr(D, c) for c in CONSTANTS}
    for s in STRUCTS:
        py_side[(s.c_name, ".")] = C.sizeof(s)
        for f, _ in s._fields_:
            py_side[(s.c_name, f)] = getattr(s, f).offset
    assert py_side == c_side


def test_parameter_builder_and_the_defaults_of_the_header():
    p = D.depth_align_params()
    assert type(p) is D.DepthAlignParams
    m, v = G.map_params(), G.vro_params()
    assert (p.fx, p.fy, p.cx, p.cy, p.z_scale, p.z_min, p.z_max) == (m.fx, m.fy, m.cx, m.cy, m.z_scale, m.z_min, m.z_max)
    assert p.sigma_px == v.sigma_px and list(p.sigma_z) == list(v.sigma_z)
    assert (p.n_levels, list(p.skip), list(p.iters), p.normal_step) == (3, [4, 2, 2], [10, 10, 5], 2)
    assert (p.normal_jump, p.max_dist, p.min_pairs, p.eps_rot, p.eps_trans, p.min_pivot) == (0.05, 0.10, 500, 1e-6, 1e-6, 1e-6)
    assert abs(p.min_cos - np.cos(np.radians(80.0))) < 1e-16
    q = D.depth_align_params(skip=(2, 1, 1), iters=[3, 2, 1], sigma_z=np.array([0.01, 0.0, 0.002]), max_dist=0.2)
    assert (list(q.skip), list(q.iters), list(q.sigma_z), q.max_dist) == ([2, 1, 1], [3, 2, 1], [0.01, 0.0, 0.002], 0.2)
    with pytest.raises(TypeError):
        D.depth_align_params(no_such_field=1)
    G.lib.fgo_depth_align_params_default(None)                                                  # NULL tolerated
    assert "depth_align_params" not in vars(G)             # the names of fgo_dense.h stay in graph_slam_amd.dense


# ---- what is refused before the first HIP call --------------------------------------------------------------------------------
def _align(n_frames=2, W=8, H=6, n_pairs=1, fi=(0,), fj=(1,), init=None, missing=(), **kw):
    depth = np.zeros((max(n_frames, 1), max(H, 1), max(W, 1)), np.uint16)
    fi = np.asarray(fi, np.int64); fj = np.asarray(fj, np.int64)
    n = max(n_pairs, 1)
    pose = np.zeros((n, 7)); res = (D.DepthAlignResult * n)()
    p0 = None if init is None else np.asarray(init, np.float64)
    a = dict(depth=G.ptr(depth), fi=G.ptr(fi), fj=G.ptr(fj), pose=G.ptr(pose), res=res)
    for name in missing:
        a[name] = None
    return G.lib.fgo_depth_align_batch(0, n_frames, W, H, a["depth"], n_pairs, a["fi"], a["fj"], G.opt(p0),
                                       C.byref(D.depth_align_params(**kw)), a["pose"], None, None, None, a["res"])


def test_depth_align_refuses_bad_arguments():
    nan, inf = float("nan"), float("inf")
    bad = [dict(missing=(name,)) for name in ("depth", "fi", "fj", "pose", "res")]
    bad += [dict(n_frames=-1), dict(n_pairs=-1), dict(W=0), dict(H=0), dict(W=1 << 13, H=(1 << 11) + 1),
            dict(fi=(-1,)), dict(fi=(2,)), dict(fj=(-1,)), dict(fj=(2,)),
            dict(init=[[0, 0, 0, 0, 0, 0, 0]]), dict(init=[[nan, 0, 0, 0, 0, 0, 1]]), dict(init=[[0, 0, 0, 0, inf, 0, 1]]),
            dict(fx=0.0), dict(fy=-1.0), dict(fx=nan), dict(cx=inf), dict(cy=nan), dict(z_scale=0.0), dict(z_min=-0.1), dict(z_min=5.0),
            dict(z_max=nan), dict(sigma_px=0.0), dict(sigma_px=nan), dict(sigma_z=(0, 0, 0)), dict(sigma_z=(0.01, -1, 0)),
            dict(sigma_z=(nan, 0, 0)), dict(n_levels=0), dict(n_levels=4), dict(skip=(0, 2, 2)), dict(skip=(4, 2, -1)),
            dict(iters=(-1, 1, 1)), dict(iters=(1, 101, 1)), dict(normal_step=0), dict(normal_step=65), dict(normal_jump=0.0),
            dict(normal_jump=nan), dict(max_dist=0.0), dict(max_dist=inf), dict(min_cos=-0.1), dict(min_cos=1.1), dict(min_cos=nan),
            dict(min_pairs=5), dict(eps_rot=-1e-9), dict(eps_trans=nan), dict(min_pivot=-1e-9), dict(min_pivot=1.0), dict(min_pivot=nan)]
    for kw in bad:
        assert _align(**kw) == EINVAL, kw
    assert _align() in (OK, ENODEV)                   # the same call with nothing wrong gets as far as the device
    # a level that is not in use is not looked at; the widest settings the header allows pass
    assert _align(n_levels=1, skip=(1, 0, -5), iters=(0, -1, 1000)) in (OK, ENODEV)
    assert _align(n_levels=3, iters=(100, 0, 100), normal_step=64, min_cos=1.0, min_pairs=6, eps_rot=0.0, eps_trans=0.0, min_pivot=0.0,
                  z_min=0.0, init=[[1, 2, 3, 0, 0, 0, -2.0]]) in (OK, ENODEV)


def test_no_pairs_is_ok_without_a_device():
    assert _align(n_pairs=0, fi=(), fj=()) == OK
    assert G.lib.fgo_depth_align_batch(0, 0, 8, 6, None, 0, None, None, None, None, None, None, None, None, None) == OK   # nothing is read
    assert _align(n_pairs=0, fi=(), fj=(), n_levels=0) == EINVAL                          # the parameters are checked all the same
    out = D.depth_align_batch(np.zeros((2, 6, 8), np.uint16), [], [], want_normal_eq=True)
    assert out["pose_ij"].shape == (0, 7) and out["info"].shape == (0, 21) and out["cov"].shape == (0, 6, 6)
    assert out["normal_eq"].shape == (0, 28) and len(out["status"]) == 0
    merged = D.align_failed_records(np.zeros((2, 6, 8), np.uint16), [0, 0], [1, 1],
                                    {"status": np.zeros(2, np.int32), "pose_ij": np.arange(14.0).reshape(2, 7), "info": np.ones((2, 21))})
    assert np.array_equal(merged["pose_ij"], np.arange(14.0).reshape(2, 7)) and np.array_equal(merged["info"], np.ones((2, 21)))
    assert list(merged["source"]) == [D.FGO_DA_SOURCE_VRO] * 2 and len(merged["dense_index"]) == 0


def test_debug_form_switch():
    try:
        assert G.lib.fgo_debug_depth_align_form(2) == 2 and G.lib.fgo_debug_depth_align_form(1) == 1
        assert G.lib.fgo_debug_depth_align_form(7) == 1 and G.lib.fgo_debug_depth_align_form(-1) == 1      # not a form: unchanged
    finally:
        assert G.lib.fgo_debug_depth_align_form(0) == 0
    assert G.lib.fgo_debug_depth_align_kernel_ms() >= 0.0
