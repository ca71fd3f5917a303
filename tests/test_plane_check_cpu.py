"""CPU-only checks of the plane check's entry point (include/fgo.h fgo_plane_check_vro_batch): the symbols are exported, the
defaults are the reference's (gtsam/test_plane_check_vo.cpp:171, 330, 355), the structs have the declared sizes, every bad
argument is refused before any HIP call, and a valid call FAILS LOUDLY without a GPU (no CPU fallback), as
fgo_two_view_ba_batch does."""
import ctypes as C

import numpy as np
import pytest

import graph_slam_amd as G

IDENT = [0, 0, 0, 0, 0, 0, 1.0]
PLANE = [0, 0, 1.0, 1.0]


def _call(n=1, pose=IDENT, info=True, cov=False, pi_ptr=(0, 1), pj_ptr=(0, 1), pi=PLANE, pj=PLANE, params=None, res=True,
          drop=()):
    """one record with one plane on either side unless told otherwise; `drop` names required pointers passed as NULL"""
    ps = np.ascontiguousarray(np.tile(np.asarray(pose, np.float64), max(n, 1)).reshape(-1, 7))
    ip, jp = np.asarray(pi_ptr, np.int64), np.asarray(pj_ptr, np.int64)
    mi, mj = max(int(np.abs(ip).max()), 1), max(int(np.abs(jp).max()), 1)
    a = np.ascontiguousarray(np.tile(np.asarray(pi, np.float64), mi)); b = np.ascontiguousarray(np.tile(np.asarray(pj, np.float64), mj))
    ca = np.tile(1e-4 * np.eye(4).reshape(16), mi); cb = np.tile(1e-4 * np.eye(4).reshape(16), mj)
    nf = np.tile(100.0 * np.eye(6)[np.triu_indices(6)], max(n, 1)); cv = np.tile(0.01 * np.eye(6).reshape(36), max(n, 1))
    r = (G.PlaneCheckResult * max(n, 1))()
    arg = lambda name, v, conv: None if name in drop else conv(v)
    return G.lib.fgo_plane_check_vro_batch(
        0, n, arg("pose", ps, G._dp), G._dp(nf) if info else None, G._dp(cv) if cov else None,
        arg("pi_ptr", ip, G._i64p), arg("pi", a, G._dp), arg("ci", ca, G._dp), arg("pj_ptr", jp, G._i64p), arg("pj", b, G._dp),
        arg("cj", cb, G._dp), None if params is None else C.byref(params), r if res else None, None, None, None, None, None, None)


def test_symbols_defaults_and_struct_sizes():
    assert hasattr(G.lib, "fgo_plane_check_vro_batch") and hasattr(G.lib, "fgo_plane_check_params_default")
    p = G.PlaneCheckParams()
    G.lib.fgo_plane_check_params_default(C.byref(p))
    assert (p.cos_min, p.d_max, p.failed_info00) == (np.cos(10.0 * np.pi / 180.0), 0.2, 10000.0)
    G.lib.fgo_plane_check_params_default(None)                   # tolerated
    assert C.sizeof(G.PlaneCheckParams) == 24 and C.sizeof(G.PlaneCheckResult) == 40
    assert G.PlaneCheckResult.err.offset == 24 and G.PlaneCheckResult.err_raw.offset == 32
    assert G.plane_check_params(d_max=0.5).d_max == 0.5 and G.plane_check_params(d_max=0.5).failed_info00 == 10000.0
    with pytest.raises(TypeError):
        G.plane_check_params(no_such_field=1)
    assert (G.FGO_PC_OK, G.FGO_PC_SKIPPED, G.FGO_PC_NUM) == (0, 1, 2)


def test_bad_arguments_are_refused_without_a_device():
    assert _call(n=-1) == -1
    for name in ("pose", "pi_ptr", "pj_ptr", "pi", "ci", "pj", "cj"):            # a NULL required pointer
        assert _call(drop=(name,)) == -1, name
    assert _call(res=False) == -1
    assert _call(info=True, cov=True) == -1                       # both
    assert _call(info=False, cov=False) == -1                     # neither
    assert _call(pi_ptr=(-1, 1)) == -1                            # negative
    assert _call(pj_ptr=(-1, 1)) == -1
    assert _call(n=2, pi_ptr=(0, 2, 1), pj_ptr=(0, 1, 2)) == -1   # decreasing
    assert _call(n=2, pi_ptr=(0, 1, 2), pj_ptr=(0, 2, 1)) == -1
    assert _call(pose=[0, 0, 0, 0, 0, 0, 0]) == -1                # zero quaternion
    assert _call(pose=[0, 0, 0, 0, 0, 0, float("nan")]) == -1
    assert _call(pi=[0, 0, 0, 1.0]) == -1                         # zero normal, either list
    assert _call(pj=[0, 0, 0, 1.0]) == -1
    for bad in (1.5, -1.5, float("nan")):
        assert _call(params=G.plane_check_params(cos_min=bad)) == -1, bad
    for bad in (-0.1, float("nan")):
        assert _call(params=G.plane_check_params(d_max=bad)) == -1, bad


def test_empty_batch_is_ok_and_a_valid_call_needs_a_device():
    assert _call(n=0, pi_ptr=(0,), pj_ptr=(0,)) == 0
    if G.lib.fgo_device_count() <= 0:
        assert _call() == -2
        assert _call(info=False, cov=True) == -2
        assert _call(pi_ptr=(0, 0), pj_ptr=(0, 0), drop=("pi", "ci", "pj", "cj")) == -2      # empty lists need no plane arrays
        assert _call(params=G.plane_check_params(cos_min=-1.0, d_max=0.0, failed_info00=-1.0)) == -2
        with pytest.raises(G.FgoError, match="-2"):
            G.plane_check_vro_batch([IDENT], [0, 1], [PLANE], [np.eye(4)], [0, 1], [PLANE], [np.eye(4)], cov=[np.eye(6)])


def test_python_wrapper_checks_shapes_before_the_call():
    ok = ([IDENT], [0, 1], [PLANE], [np.eye(4)], [0, 1], [PLANE], [np.eye(4)])
    with pytest.raises(G.FgoError, match="exactly one"):
        G.plane_check_vro_batch(*ok)
    with pytest.raises(G.FgoError, match="exactly one"):
        G.plane_check_vro_batch(*ok, info=np.zeros((1, 21)), cov=np.zeros((1, 6, 6)))
    with pytest.raises(G.FgoError, match="n_records"):
        G.plane_check_vro_batch([IDENT], [0, 1, 2], *ok[2:], cov=np.zeros((1, 6, 6)))
    with pytest.raises(G.FgoError, match="fewer"):
        G.plane_check_vro_batch([IDENT], [0, 2], *ok[2:], cov=np.zeros((1, 6, 6)))
    with pytest.raises(G.FgoError, match="one entry per record"):
        G.plane_check_vro_batch(*ok, cov=np.zeros((2, 6, 6)))
