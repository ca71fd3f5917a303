"""CPU-only checks of the product library: it loads, exports every symbol include/fgo.h declares, the
host-only entry points (synthetic generator, shard helper) behave, and device entry points FAIL LOUDLY
without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import graph_slam_amd as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "fgo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fgo_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported():
    syms = _declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(G.lib, s), "libfgo.so does not export %s" % s


def test_version_and_error_string():
    assert b"gfx950" in G.lib.fgo_version()


def test_no_gpu_fails_loudly():
    if G.lib.fgo_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(G.FgoError) as ei:
        G.Graph()
    assert "no CPU fallback" in str(ei.value) or "HIP" in str(ei.value)


def test_synth_cfg1_shape_and_determinism():
    g = G.synth_manhattan3d(1000, 4, 0, seed=42)
    assert len(g["ei"]) == 4984                 # ~5k edges: BASELINE config 1
    assert (g["ei"] < g["ej"]).all()            # edges point old -> new (g2o_graph.cpp:174,196-205)
    g2 = G.synth_manhattan3d(1000, 4, 0, seed=42)
    for k in g:
        np.testing.assert_array_equal(g[k], g2[k])
    g3 = G.synth_manhattan3d(1000, 4, 0, seed=43)
    assert not np.array_equal(g["meas"], g3["meas"])
    # unit quaternions, lattice truth, odometry-chained initial guess
    np.testing.assert_allclose(np.linalg.norm(g["poses"][:, 3:], axis=1), 1, atol=1e-12)
    np.testing.assert_allclose(g["truth"][:, :3], np.round(g["truth"][:, :3]), atol=0)
    steps = np.linalg.norm(np.diff(g["truth"][:, :3], axis=0), axis=1)
    np.testing.assert_allclose(steps, 1.0)
    # information = diag(1/sigma_t^2 x3, 1/sigma_q^2 x3)
    W = g["info"][0]
    assert W[0] == pytest.approx(1 / 0.02 ** 2) and W[20] == pytest.approx(1 / 0.005 ** 2) and W[1] == 0


def test_synth_cfg2_edge_budget():
    g = G.synth_manhattan3d(20000, 5, 4, seed=42)
    e = len(g["ei"])
    assert abs(e - 10 * 20000) < 0.01 * 10 * 20000          # 10 edges / pose -> 1M at 100k poses
    span = g["ej"] - g["ei"]
    assert (span >= 1).all() and span.max() > 100           # real long-range loop closures exist


def test_synth_measurements_consistent_with_truth():
    from tests.util import pose_mul, pose_inv
    g = G.synth_manhattan3d(300, 4, 2, seed=5, sigma_t=0.0, sigma_q=0.0)
    for k in range(0, len(g["ei"]), 17):
        z = pose_mul(pose_inv(g["truth"][g["ei"][k]]), g["truth"][g["ej"][k]])
        s = np.sign(z[3:] @ g["meas"][k][3:])
        np.testing.assert_allclose(g["meas"][k][:3], z[:3], atol=1e-12)
        np.testing.assert_allclose(g["meas"][k][3:] * s, z[3:], atol=1e-12)
    np.testing.assert_allclose(g["poses"][:, :3], g["truth"][:, :3], atol=1e-9)


def test_shard_range_partitions():
    lo, hi = C.c_int64(), C.c_int64()
    for n, w in [(10, 3), (1000000, 8), (5, 8), (0, 2)]:
        cover = []
        for r in range(w):
            assert G.lib.fgo_shard_range(n, r, w, C.byref(lo), C.byref(hi)) == 0
            cover.append((lo.value, hi.value))
        assert cover[0][0] == 0 and cover[-1][1] == n
        for a, b in zip(cover, cover[1:]):
            assert a[1] == b[0]
        sizes = [b - a for a, b in cover]
        assert max(sizes) - min(sizes) <= 1
    assert G.lib.fgo_shard_range(10, 3, 3, C.byref(lo), C.byref(hi)) == -1


def test_preint_batch_refuses_without_gpu_and_validates():
    """the batched preintegration is a GPU entry point: no device -> FGO_ENODEV (no CPU fallback), bad input -> FGO_EINVAL"""
    import ctypes as C
    assert hasattr(G.lib, "fgo_preint_batch")
    sp = np.array([0, 2], np.int64)
    acc = np.zeros((2, 3)); gyro = np.zeros((2, 3))
    params = np.zeros(G.IMU_PARAM_DOUBLES); G.lib.fgo_imu_params_vn100(G._dp(params))
    out = np.zeros((1, G.PREINT_DOUBLES))
    bad = np.array([3, 2], np.int64)
    assert G.lib.fgo_preint_batch(0, 1, G._i64p(bad), G._dp(acc), G._dp(gyro), 0.005, None, G._dp(params), G._dp(out)) == -1
    assert G.lib.fgo_preint_batch(0, 1, G._i64p(sp), G._dp(acc), G._dp(gyro), -1.0, None, G._dp(params), G._dp(out)) == -1
    if G.lib.fgo_device_count() <= 0:
        assert G.lib.fgo_preint_batch(0, 1, G._i64p(sp), G._dp(acc), G._dp(gyro), 0.005, None, G._dp(params), G._dp(out)) == -2


def test_front_end_batches_validate_before_the_device_and_refuse_without_gpu():
    """the five stand-alone batched front ends decide every FGO_EINVAL, and n == 0 -> FGO_OK, before their first HIP call, so all
    of that holds without a device; a valid one-record call then gets FGO_ENODEV (no CPU fallback)"""
    L = G.lib
    OK, EINVAL, ENODEV = 0, -1, -2
    no_gpu = L.fgo_device_count() <= 0
    dec = G._i64p(np.array([0, 2, 1], np.int64))              # a decreasing ptr array (two records)
    neg = G._i64p(np.array([-1, 1], np.int64))                # a negative ptr[0] (one record)

    # fgo_two_view_ba_batch
    calib = np.array([250.0, 250.0, 0.0, 90.0, 70.0, 0.0, 0.0, 0.0, 0.0])
    ptr6 = np.array([0, 6], np.int64)
    xyz = np.random.default_rng(0).uniform(1.0, 2.0, (6, 3)); uvi = np.zeros((6, 2)); uvj = np.zeros((6, 2))
    pj = np.zeros((2, 7)); tres = (G.TwoViewResult * 2)()

    def two_view(n, ptr, params=None):
        return L.fgo_two_view_ba_batch(0, n, ptr, G._dp(xyz), G._dp(uvi), G._dp(uvj), None, G._dp(calib), None, params, G._dp(pj), None,
                                       None, None, tres)
    assert L.fgo_two_view_ba_batch(0, 0, None, None, None, None, None, None, None, None, None, None, None, None, None) == OK
    assert two_view(2, dec) == EINVAL
    assert two_view(1, neg) == EINVAL
    tp = G.TwoViewParams(); L.fgo_two_view_params_default(C.byref(tp)); tp.min_matches = 2
    assert two_view(1, G._i64p(ptr6), C.byref(tp)) == EINVAL
    if no_gpu:
        assert two_view(1, G._i64p(ptr6)) == ENODEV

    # fgo_plane_check_vro_batch
    pose = np.array([[0.0, 0, 0, 0, 0, 0, 1]] * 2); pose0 = np.zeros((2, 7))
    info = np.zeros((2, 21)); info[:, [0, 6, 11, 15, 18, 20]] = 1.0
    cov = np.tile(np.eye(6).ravel(), (2, 1))
    one = np.array([0, 1], np.int64)
    abcd = np.array([[0.0, 0, 1, 1]] * 2); cov16 = np.tile((1e-4 * np.eye(4)).ravel(), (2, 1))
    pres = (G.PlaneCheckResult * 2)()

    def plane_check(n, ps, inf, cv, pi_ptr, pj_ptr, params=None):
        return L.fgo_plane_check_vro_batch(0, n, G._dp(ps), inf, cv, pi_ptr, G._dp(abcd), G._dp(cov16), pj_ptr, G._dp(abcd), G._dp(cov16),
                                           params, pres, None, None, None, None, None, None)
    assert L.fgo_plane_check_vro_batch(0, 0, *([None] * 17)) == OK
    assert plane_check(2, pose, G._dp(info), None, dec, G._i64p(np.array([0, 1, 2], np.int64))) == EINVAL
    assert plane_check(2, pose, G._dp(info), None, G._i64p(np.array([0, 1, 2], np.int64)), dec) == EINVAL
    assert plane_check(1, pose, G._dp(info), None, neg, G._i64p(one)) == EINVAL
    assert plane_check(1, pose, G._dp(info), None, G._i64p(one), neg) == EINVAL
    assert plane_check(1, pose0, G._dp(info), None, G._i64p(one), G._i64p(one)) == EINVAL
    assert plane_check(1, pose, G._dp(info), G._dp(cov), G._i64p(one), G._i64p(one)) == EINVAL
    assert plane_check(1, pose, None, None, G._i64p(one), G._i64p(one)) == EINVAL
    pp = G.PlaneCheckParams(); L.fgo_plane_check_params_default(C.byref(pp)); pp.d_max = -1.0
    assert plane_check(1, pose, G._dp(info), None, G._i64p(one), G._i64p(one), C.byref(pp)) == EINVAL
    if no_gpu:
        assert plane_check(1, pose, G._dp(info), None, G._i64p(one), G._i64p(one)) == ENODEV
        assert plane_check(1, pose, None, G._dp(cov), G._i64p(one), G._i64p(one)) == ENODEV

    # fgo_imu_check_vro_batch
    pm = np.zeros((1, G.PREINT_DOUBLES)); idx = np.zeros(2, np.int64)
    ires = (G.ImuCheckResult * 2)()

    def imu_check(n, ps, inf, cv, params=None):
        return L.fgo_imu_check_vro_batch(0, n, G._dp(ps), inf, cv, 1, G._dp(pm), G._i64p(idx), None, None, params, ires, None, None)
    assert L.fgo_imu_check_vro_batch(0, 0, None, None, None, 0, None, None, None, None, None, None, None, None) == OK
    assert imu_check(1, pose0, G._dp(info), None) == EINVAL
    assert imu_check(1, pose, G._dp(info), G._dp(cov)) == EINVAL
    assert imu_check(1, pose, None, None) == EINVAL
    ip = G.ImuCheckParams(); L.fgo_imu_check_params_default(C.byref(ip)); ip.d2_gate = 0.0
    assert imu_check(1, pose, G._dp(info), None, C.byref(ip)) == EINVAL
    if no_gpu:
        assert imu_check(1, pose, G._dp(info), None) == ENODEV

    # fgo_vro_ransac_batch
    xi = np.zeros((6, 3)); xj = np.zeros((6, 3)); vpose = np.zeros((2, 7)); vres = (G.VroResult * 2)()

    def vro(n, ptr, params=None):
        return L.fgo_vro_ransac_batch(0, n, ptr, G._dp(xi), G._dp(xj), params, G._dp(vpose), None, None, None, None, vres)
    assert L.fgo_vro_ransac_batch(0, 0, None, None, None, None, None, None, None, None, None, None) == OK
    assert vro(2, dec) == EINVAL
    assert vro(1, neg) == EINVAL
    vp = G.VroParams(); L.fgo_vro_params_default(C.byref(vp)); vp.hypotheses = 0
    assert vro(1, G._i64p(ptr6), C.byref(vp)) == EINVAL
    if no_gpu:
        assert vro(1, G._i64p(ptr6)) == ENODEV

    # fgo_plane_extract_batch
    depth = np.zeros((4, 4), np.uint16); xres = (G.PlaneExtractResult * 1)()
    xabcd = np.zeros((G.FGO_PX_MAX_PLANES, 4)); xcov = np.zeros((G.FGO_PX_MAX_PLANES, 16))

    def extract(n, w, params=None):
        return L.fgo_plane_extract_batch(0, n, w, 4, depth.ctypes.data_as(C.POINTER(C.c_uint16)), params, xres, G._dp(xabcd), G._dp(xcov),
                                         None, None, None, None)
    assert L.fgo_plane_extract_batch(0, 0, 4, 4, None, None, None, None, None, None, None, None, None) == OK
    assert extract(1, 0) == EINVAL
    xp = G.PlaneExtractParams(); L.fgo_plane_extract_params_default(C.byref(xp)); xp.max_planes = 0
    assert extract(1, 4, C.byref(xp)) == EINVAL
    if no_gpu:
        assert extract(1, 4) == ENODEV


def test_exports_are_the_c_abi_only_and_the_allocator_stays_inside():
    """libfgo.so exports the fgo_* entry points and nothing else of its own -- in particular not its operator new / delete
    (csrc/host_alloc.cpp: the library's allocations forward to the process's global operators and add a huge-page hint; a host
    program must never be routed through them).  FGO_THP=0 switches the hint off: the host-only decomposition runs either way."""
    import subprocess
    import sys
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "graph_slam_amd", "libfgo.so")], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("nm not available")
    names = [l.split()[-1] for l in out.stdout.splitlines() if l.strip()]
    own = [n for n in names if not n.startswith("fgo_") and n not in ("FGO_1", "_init", "_fini", "__bss_start", "_edata", "_end")]
    assert own == [], own
    assert not any(n.startswith("_Zn") or n.startswith("_Zd") for n in names)
    code = ("import numpy as np, graph_slam_amd as G\n"
            "g = G.synth_manhattan3d(20000, 5, 4, seed=3)\n"
            "grp = G.debug_partition(20000, g['ei'], g['ej'], 2)\n"
            "print(int(np.bincount(grp, minlength=3)[2]))\n")
    tops = []
    for thp in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, FGO_THP=thp), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        tops.append(int(r.stdout.split()[-1]))
    assert tops[0] == tops[1] and tops[0] > 0
