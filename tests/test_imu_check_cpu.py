"""CPU-only checks of the IMU check's entry point (include/fgo.h fgo_imu_check_vro_batch): the symbols are exported, the defaults
are the reference's (gtsam/test_vro_imu_graph.cpp:683, :753), the structs have the declared sizes, every bad argument is refused
before any HIP call, and a valid call FAILS LOUDLY without a GPU (no CPU fallback), as fgo_plane_check_vro_batch does."""
import ctypes as C

import numpy as np
import pytest

import graph_slam_amd as G

IDENT = [0, 0, 0, 0, 0, 0, 1.0]


def _preint(n=1):
    p = G.Preintegrator()
    p.integrate([0, 0, 9.7], [0.1, 0, 0], 0.005)
    return np.ascontiguousarray(np.tile(p.buf, (n, 1)))


def _call(n=1, pose=IDENT, info=True, cov=False, n_preint=1, index=0, bias=False, q_uc=None, params=None, res=True, drop=()):
    """one record on one preintegration unless told otherwise; `drop` names required pointers passed as NULL"""
    m = max(n, 1)
    ps = np.ascontiguousarray(np.tile(np.asarray(pose, np.float64), m).reshape(-1, 7))
    nf = np.tile(100.0 * np.eye(6)[np.triu_indices(6)], m); cv = np.tile(0.01 * np.eye(6).reshape(36), m)
    pm = _preint(max(n_preint, 1))
    ix = np.full(m, index, np.int64)
    b = np.zeros((m, 6))
    q = None if q_uc is None else np.asarray(q_uc, np.float64)
    r = (G.ImuCheckResult * m)()
    arg = lambda name, v, conv: None if name in drop else conv(v)
    return G.lib.fgo_imu_check_vro_batch(
        0, n, arg("pose", ps, G._dp), G._dp(nf) if info else None, G._dp(cv) if cov else None, n_preint, arg("preint", pm, G._dp),
        arg("index", ix, G._i64p), G._dp(b) if bias else None, None if q is None else G._dp(q),
        None if params is None else C.byref(params), r if res else None, None, None)


def test_symbols_defaults_and_struct_sizes():
    for s in ("fgo_imu_check_vro_batch", "fgo_imu_check_params_default", "fgo_chi2_quantile"):
        assert hasattr(G.lib, s), s
    p = G.ImuCheckParams()
    G.lib.fgo_imu_check_params_default(C.byref(p))
    assert abs(p.d2_gate - 7.814727903251179) <= 1e-11 and (p.d2_ref_gate, p.failed_info00) == (40000.0, 10000.0)
    assert p.d2_gate == G.chi2_quantile(3, 0.95)
    G.lib.fgo_imu_check_params_default(None)                     # tolerated
    assert C.sizeof(G.ImuCheckParams) == 24 and C.sizeof(G.ImuCheckResult) == 32
    assert (G.ImuCheckParams.d2_gate.offset, G.ImuCheckParams.d2_ref_gate.offset, G.ImuCheckParams.failed_info00.offset) == (0, 8, 16)
    R = G.ImuCheckResult
    assert (R.status.offset, R.reject.offset, R.d2.offset, R.d2_ref.offset, R.angle.offset) == (0, 4, 8, 16, 24)
    assert G.imu_check_params(d2_gate=9.0).d2_gate == 9.0 and G.imu_check_params(d2_gate=9.0).d2_ref_gate == 40000.0
    with pytest.raises(TypeError):
        G.imu_check_params(no_such_field=1)
    assert (G.FGO_IC_OK, G.FGO_IC_SKIPPED, G.FGO_IC_NUM) == (0, 1, 2)


def test_bad_arguments_are_refused_without_a_device():
    assert _call(n=-1) == -1
    for name in ("pose", "preint", "index"):                      # a NULL required pointer
        assert _call(drop=(name,)) == -1, name
    assert _call(res=False) == -1
    assert _call(info=True, cov=True) == -1                       # both
    assert _call(info=False, cov=False) == -1                     # neither
    assert _call(n_preint=0) == -1 and _call(n_preint=-3) == -1   # no preintegration to test against
    assert _call(index=-1) == -1 and _call(index=1) == -1 and _call(n_preint=2, index=2) == -1     # an index out of range
    assert _call(n=3, n_preint=2, index=2) == -1
    assert _call(pose=[0, 0, 0, 0, 0, 0, 0]) == -1                # zero quaternion: record
    assert _call(pose=[0, 0, 0, 0, 0, 0, float("nan")]) == -1
    assert _call(q_uc=[0, 0, 0, 0]) == -1                         # zero quaternion: extrinsic
    assert _call(q_uc=[0, float("inf"), 0, 1]) == -1
    for field in ("d2_gate", "d2_ref_gate"):                      # a gate <= 0
        for bad in (0.0, -1.0, float("nan")):
            assert _call(params=G.imu_check_params(**{field: bad})) == -1, (field, bad)


def test_empty_batch_is_ok_and_a_valid_call_needs_a_device():
    assert _call(n=0) == 0
    assert _call(n=0, n_preint=0, drop=("pose", "preint", "index"), res=False) == 0
    if G.lib.fgo_device_count() <= 0:
        assert _call() == -2
        assert _call(info=False, cov=True) == -2
        assert _call(n=3, n_preint=2, index=1, bias=True, q_uc=[0.1, 0.2, 0.3, 0.9]) == -2
        assert _call(params=G.imu_check_params(d2_gate=1.0, d2_ref_gate=1.0, failed_info00=-1.0)) == -2
        with pytest.raises(G.FgoError, match="-2"):
            G.imu_check_vro_batch([IDENT], _preint(), [0], cov=[np.eye(6)], want_dw=True, want_cov=True)


def test_python_wrapper_checks_shapes_before_the_call():
    pm = _preint()
    with pytest.raises(G.FgoError, match="exactly one"):
        G.imu_check_vro_batch([IDENT], pm, [0])
    with pytest.raises(G.FgoError, match="exactly one"):
        G.imu_check_vro_batch([IDENT], pm, [0], info=np.zeros((1, 21)), cov=np.zeros((1, 6, 6)))
    with pytest.raises(G.FgoError, match="preint_index"):
        G.imu_check_vro_batch([IDENT], pm, [0, 0], cov=np.zeros((1, 6, 6)))
    with pytest.raises(G.FgoError, match="one entry per record"):
        G.imu_check_vro_batch([IDENT], pm, [0], cov=np.zeros((2, 6, 6)))
    with pytest.raises(G.FgoError, match="bias_i"):
        G.imu_check_vro_batch([IDENT], pm, [0], cov=np.zeros((1, 6, 6)), bias_i=np.zeros((2, 6)))
    with pytest.raises(G.FgoError, match="x y z w"):
        G.imu_check_vro_batch([IDENT], pm, [0], cov=np.zeros((1, 6, 6)), imu_q_cam=[1.0, 0, 0])
