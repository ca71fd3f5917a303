"""GPU: the covariance k_preint_batch (csrc/preint_kernel.hip) propagates, and the whole route from raw IMU samples to H -- k_preint_batch,
fgo_preint_information, ImuPayload.info, k_imu_eval, k_imu_blocks -- against references that share nothing with it but the noise convention
(tests/preint_cov_independent.py, tests/chart_edges.preintegrate, tests/imu_independent.py: 40 digits, every derivative a central difference
of the definition).  The inputs are tests.preint_cov_independent.cases(), the list tests/test_preint_cov_cpu.py holds host and oracle to.

fgo_preint_batch takes one fgo_imu_params per call, so the cases go in one call per parameter set (three calls; the VN100 one holds the ragged
counts 0, 1, 2, 3, 8, 16, 40 with the empty factor first).

Measured on the MI355X (gfx950):
  device covariance, scaled error   largest 1.47e-15 (n40; oracle 1.35e-15, host 1.61e-15); largest relative to the oracle's error on the same
                                    case 1.33 (n8: 6.8e-16 against 5.1e-16); 0 on the empty factor                 bound 16 x the oracle's
  raw samples -> H                  H 5.3e-16 of the component's largest entry, b 4.9e-16, chi2 2.2e-16             bounds 1e-8, 1e-8, 1e-9
With -h replaced by -dt * dt in the p-theta block of F in imu_preint.cpp, preint_kernel.hip and orc_imu.h alike (a scratch build), the
covariance errs by 2.2e-4 (n2) ... 2.3e-2 (spread_b), 1.2e-3 at n8, and H by 1.3e-5, b by 4.2e-4, chi2 by 1.9e-4: both tests fail, as do the
oracle's and the host's in tests/test_preint_cov_cpu.py, while tests/test_host_preint.py and tests/test_oracle_imu.py pass."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from tests import orc_binding as orc
from tests import preint_cov_independent as pc

CASES = pc.cases()
IDS = [c["name"] for c in CASES]


def batch(idx):
    """one fgo_preint_batch call on cases idx (one parameter set), in that order"""
    cs = [CASES[k] for k in idx]
    assert len({c["params"] for c in cs}) == 1 and len({c["dt"] for c in cs}) == 1
    sp = np.concatenate([[0], np.cumsum([len(c["acc"]) for c in cs])])
    acc = np.concatenate([c["acc"] for c in cs]).reshape(-1, 3)
    gyro = np.concatenate([c["gyro"] for c in cs]).reshape(-1, 3)
    bias = None if all(c["bhat"] is None for c in cs) else np.array([np.zeros(6) if c["bhat"] is None else c["bhat"] for c in cs])
    return G.preint_batch(sp, acc, gyro, cs[0]["dt"], bias_hat=bias, params=pc.params9(cs[0]))


def groups():
    out = {}
    for k, c in enumerate(CASES):
        out.setdefault(c["params"], []).append(k)
    return list(out.values())


@functools.lru_cache(maxsize=None)
def device_payloads():
    """payload of every case, each parameter set in list order"""
    out = {}
    for idx in groups():
        for k, row in zip(idx, batch(idx)):
            out[k] = row
    return out


def test_device_covariance_vs_differentiated_step():
    """out[f, 62:] against the 40-digit covariance, scaled error max |C - C*|_ij / sqrt(C*_ii C*_jj), bound 16 x the oracle's own error on the
    case and no less than 2^-52 (FMA contraction and the summation order of the device differ from the host's)."""
    gr = groups()
    assert len(gr) == 3 and sorted(len(CASES[k]["acc"]) for k in gr[0])[:4] == [0, 1, 2, 2] and len(CASES[gr[0][0]]["acc"]) == 0
    assert any(all(CASES[k]["bhat"] is None for k in idx) for idx in gr)          # one call without a bias array
    out = device_payloads()
    bad = []
    for k, c in enumerate(CASES):
        n = len(c["acc"])
        assert out[k][0] == pytest.approx(n * c["dt"], abs=1e-15)
        np.testing.assert_array_equal(out[k][56:62], np.zeros(6) if c["bhat"] is None else c["bhat"])
        err = pc.scaled_error(out[k][62:].reshape(15, 15), pc.reference(k)[0])
        print("%-10s n %2d  device %.3e  oracle %.3e  bound %.3e" % (IDS[k], n, err, pc.oracle_error(k), pc.product_bound(k)))
        if not err <= pc.product_bound(k):
            bad.append((IDS[k], err, pc.product_bound(k)))
    assert not bad, bad


def test_device_payload_does_not_depend_on_the_block_it_ran_in():
    """the same factors permuted: every payload bit for bit the one of the first run (block index -> factor, nothing left in LDS by the
    factor a block's predecessor on the compute unit integrated)"""
    first = device_payloads()
    for idx in groups():
        perm = list(np.random.default_rng(len(idx)).permutation(len(idx)))
        if len(idx) > 1:
            assert perm != list(range(len(idx)))
        again = batch([idx[p] for p in perm])
        for row, p in zip(again, perm):
            assert np.array_equal(row, first[idx[p]]), IDS[idx[p]]


# ------------------------------------------------------------------------------------------------ raw samples -> H
def test_raw_samples_to_H_vs_independent_references():
    """tests.preint_cov_independent.imu_only_graph(): IMU factors only, payloads from fgo_preint_batch on raw samples: three factors on disjoint
    variables (one colour) and a chain of two that share X / V / B of the middle key frame (a second colour) and whose first pose is FIXED --
    the col < 0 paths of k_imu_blocks: no diagonal block, pair slots -1, no gradient column.  Reference: r and J from
    tests.imu_independent.factor read through the reference's own preintegration, W the 40-digit inverse of the 40-digit covariance.
    Bounds as in test_combined_imu_factor_blocks_vs_matrix_logarithm, per component of the graph: H 1e-8 of its largest entry, b 1e-8, chi2 1e-9
    (tests/test_preint_cov_cpu.py holds the oracle to the same system)."""
    g = pc.imu_only_graph()
    dev = device_payloads()
    gr = G.Graph()
    gr.add_poses(g["poses"], g["fixed"])
    for k in range(pc.N_KEY):
        gr.add_vec3(pc.N_KEY + k, g["vels"][k])
    for k in range(pc.N_KEY):
        gr.add_bias(2 * pc.N_KEY + k, g["bias"][k])
    gr.set_gravity(orc.GRAVITY)
    for ids, k in zip(g["ids"], g["ks"]):
        gr.add_imu(ids, dev[k])
    chi, H, b = gr.linearize(dense=True)
    chi_alone = gr.chi2()
    gr.close()
    figures, ec = pc.system_errors(chi, H, b)
    print("H, b per component:", " ".join("(%.3e, %.3e)" % f for f in figures), " chi2 %.3e" % ec)
    assert max(e for e, _ in figures) <= 1e-8 and max(e for _, e in figures) <= 1e-8, figures
    cref = pc.reference_system()[2]
    assert ec <= 1e-9 and abs(chi_alone - cref) <= 1e-9 * cref                            # k_chi2_imu: the stand-alone chi2


# ------------------------------------------------------------------------------------------------ fixed gauge
def test_vio_linearization_with_a_fixed_first_pose_matches_oracle():
    """test_vio_linearization_matches_oracle (n_kf = 7, planes) with pose 0 fixed instead of carrying the 1e14 prior: the IMU factor, the
    between factor and the plane factors on pose 0 lose its columns on both sides; H / b 1e-10 of the largest entry, chi2 1e-11, nothing masked"""
    from tests.test_gpu_imu import same_information, vio_gpu
    from tests.util import vio_graph
    g = same_information(vio_graph(np.random.default_rng(1), n_kf=7, with_planes=True))
    fixed = np.zeros(len(g["values"]), np.uint8); fixed[0] = 1
    po = orc.Problem(g["values"], fixed, g["ei"], g["ej"], g["meas"], g["info"])
    po.set_kinds(g["vkind"], g["kind"])
    po.set_calibration(g["calib"], g["bps"])
    assert g["prior_ids"][0] == 0
    po.add_priors(g["prior_ids"][1:], g["prior_mean"][1:], g["prior_info"][1:])
    po.add_imu_factors(g["imu_ids"], g["imu_pre"], g["imu_info"])
    gr = vio_gpu(g, fix_first=True)
    chi, H, b = gr.linearize()
    Ho, bo = po.dense_system()
    assert H.shape == Ho.shape == (6 * (len(fixed) - 1),) * 2
    assert abs(chi - po.chi2()) <= 1e-11 * po.chi2()
    np.testing.assert_allclose(H, Ho, rtol=0, atol=1e-10 * np.abs(Ho).max())
    np.testing.assert_allclose(b, bo, rtol=0, atol=1e-10 * np.abs(bo).max())
    assert abs(gr.chi2() - po.chi2()) <= 1e-11 * po.chi2()
