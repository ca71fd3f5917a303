"""Pins the numpy restatement of the VRO RANSAC registration (tests/vro_ransac_reference.py) on the CPU: the hash on hand-computed
values, the sampling, the triad fit and the least-squares fit on planted transforms, the information against a finite-difference
Hessian, and the generated GPU cases for being well posed."""
import functools

import numpy as np
import pytest

from tests import vro_ransac_reference as ref

CONFIGS = ((1, 8), (100, 8), (256, 8), (256, 3))   # (hypotheses, min_inliers) of the GPU test's calls


def test_mix_on_hand_computed_values():
    # u_k of hypothesis 0 with seed 0 are the first three outputs of the splitmix64 generator seeded with 0 (Steele, Lea & Flood 2014;
    # the values are the ones published with the generator's reference implementation)
    want = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)
    assert tuple(ref.mix((k + 1) * ref.GOLDEN) for k in range(3)) == want
    assert ref.mix(0) == 0                                       # every step maps 0 to 0
    # one value by hand, step by step: z = 1
    z = 1
    z ^= z >> 30; assert z == 1
    z = (z * 0xBF58476D1CE4E5B9) % 2 ** 64; assert z == 0xBF58476D1CE4E5B9
    z ^= z >> 27; assert z == 0xBF58476D1CE4E5B9 ^ (0xBF58476D1CE4E5B9 >> 27)
    z = (z * 0x94D049BB133111EB) % 2 ** 64
    z ^= z >> 31
    assert ref.mix(1) == z
    assert ref.mix(2 ** 64 + 1) == z                             # arithmetic is mod 2^64
    assert ref.sample3(0, 0, 100) == tuple(ref.sample3(0, 0, 100)) and ref.sample3(0, 0, 100)[0] == want[0] % 100


@pytest.mark.parametrize("M", [3, 4, 5, 64])
def test_samples_are_distinct_and_in_range(M):
    seen = set()
    for h in range(1000):
        a, b, c = ref.sample3(0, h, M)
        assert len({a, b, c}) == 3 and min(a, b, c) >= 0 and max(a, b, c) < M, (h, a, b, c)
        seen.add((a, b, c))
    assert ref.sample3(7, 5, M) == ref.sample3(7, 5, M)
    if M > 3:
        assert len(seen) > 1 and any(ref.sample3(1, h, M) != ref.sample3(0, h, M) for h in range(20))
    if M == 4:
        assert len(seen) == 24                                   # every ordered triple of 4 occurs within 1000 draws


def _planted(rng, angle):
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    return ref.so3_exp(angle * axis), rng.uniform(-1, 1, 3)


def test_triad_fit_returns_a_planted_transform_from_three_exact_points():
    rng = np.random.default_rng(1)
    for angle in (0.0, 0.3, 2.0, np.pi - 1e-3):
        R, t = _planted(rng, angle)
        pj = rng.uniform(-1, 1, (3, 3)) + [0, 0, 3]
        Rf, tf = ref.triad_fit(pj @ R.T + t, pj)
        assert np.abs(Rf - R).max() < 1e-13 and np.abs(tf - t).max() < 1e-13, angle
        assert abs(np.linalg.det(Rf) - 1) < 1e-14


def test_least_squares_fit_recovers_a_planted_transform():
    rng = np.random.default_rng(2)
    for angle in (0.0, 0.1, 1.0, np.pi - 1e-3):
        R, t = _planted(rng, angle)
        pj = rng.uniform(ref.BOX_LO, ref.BOX_HI, (30, 3))
        Rf, tf, gap = ref.fit(pj @ R.T + t, pj)
        assert np.abs(Rf - R).max() < 1e-13 and np.abs(tf - t).max() < 1e-12 and 0 < gap <= 2, (angle, gap)
        q = ref.quat_xyzw(Rf)
        assert q[3] >= 0 and abs(q @ q - 1) < 1e-15 and np.abs(ref.quat_matrix(q) - R).max() < 1e-13
    # a reflection is the better orthogonal fit of mirrored points: the proper rotation is returned all the same
    pj = rng.uniform(-1, 1, (10, 3))
    Rf, tf, gap = ref.fit(pj * [1, 1, -1], pj)
    assert abs(np.linalg.det(Rf) - 1) < 1e-14


def _se3_exp(xi):
    w, v = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    K = ref.skew(w)
    if th < 1e-12:
        return np.eye(3) + K, v + 0.5 * K @ v
    V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    return ref.so3_exp(w), V @ v


def test_information_is_the_finite_difference_hessian():
    """f(xi) = 1/2 sum r_k(T Exp(xi))^T S_k^-1 r_k(T Exp(xi)) with S_k frozen at T, on noise-free matches: r_k(0) = 0, so the
    Hessian at 0 is sum J^T S^-1 J exactly (the second-derivative term is multiplied by r = 0).
    Central second difference with step h: H_ab ~ (f(+a+b) - f(+a-b) - f(-a+b) + f(-a-b)) / (4 h^2).  f is quadratic up to terms
    of fourth order in xi, which enter at a relative h^2 |p|^2 <= 1e-9 x 30 = 3e-8 for h = 3e-5 and |p| <= 5.5 m.  Rounding: r is a
    difference of coordinates of size 5 m (absolute error 1e-15) and is of size 5 h, so f carries a relative 2e-16 x 5 / (5 h) ~ 1e-11,
    and so does the difference quotient.  Tolerance: 1e-6 of the largest entry, a factor 30 above the larger of the two."""
    rng = np.random.default_rng(3)
    P = dict(ref.DEFAULTS, sigma_z=(0.014, 0.002, 0.001))
    R, t = _planted(rng, 0.7)
    pi = rng.uniform(ref.BOX_LO, ref.BOX_HI, (25, 3))
    pj = (pi - t) @ R
    info, _ = ref.information(R, t, pi, pj, P)
    Sinv = [np.linalg.inv(ref.residual_cov(R, a, b, P)) for a, b in zip(pi, pj)]

    def f(xi):
        dR, dt = _se3_exp(xi)
        r = pi - (pj @ (R @ dR).T + (t + R @ dt))
        return 0.5 * sum(x @ S @ x for x, S in zip(r, Sinv))

    h, H, E = 3e-5, np.zeros((6, 6)), np.eye(6)
    for a in range(6):
        for b in range(6):
            H[a, b] = (f(h * (E[a] + E[b])) - f(h * (E[a] - E[b])) - f(h * (E[b] - E[a])) + f(-h * (E[a] + E[b]))) / (4 * h * h)
    assert np.abs(H - info).max() <= 1e-6 * np.abs(info).max(), np.abs(H - info).max() / np.abs(info).max()
    assert np.array_equal(info, info.T) and np.linalg.eigvalsh(info)[0] > 0


def test_point_noise_is_the_back_projection_of_pixel_and_depth_noise():
    # p = ((u - cx) z / fx, (v - cy) z / fy, z): its Jacobian in (u, v, z), written in terms of the point, is G
    P = ref.DEFAULTS
    p = np.array([0.7, -0.4, 2.5])
    back = lambda u, v, z: np.array([u * z / P["fx"], v * z / P["fy"], z])
    u, v = p[0] * P["fx"] / p[2], p[1] * P["fy"] / p[2]
    e = 1e-6
    G = np.stack([(back(u + e, v, p[2]) - back(u - e, v, p[2])) / (2 * e), (back(u, v + e, p[2]) - back(u, v - e, p[2])) / (2 * e),
                  (back(u, v, p[2] + e) - back(u, v, p[2] - e)) / (2 * e)], 1)
    want = G @ np.diag([1.0, 1.0, 0.014 ** 2]) @ G.T
    assert np.abs(ref.point_cov(p, P) - want).max() < 1e-12


@functools.lru_cache(maxsize=None)
def _results(K, min_inliers):
    return [ref.ransac_pair(p["xi"], p["xj"], hypotheses=K, min_inliers=min_inliers) for p in ref.gpu_cases()]


@pytest.mark.parametrize("K,min_inliers", CONFIGS)
def test_generated_gpu_cases_are_well_posed(K, min_inliers):
    pairs = ref.gpu_cases()
    res = _results(K, min_inliers)
    ok = 0
    for k, (p, r) in enumerate(zip(pairs, res)):
        assert r["decided"].mean() >= 0.95, (k, p["kind"], r["decided"].mean())
        if r["status"] == ref.VRO_OK:
            ok += 1
            if min_inliers == 8:                                 # below the default a handful of matches can register on outliers
                assert np.array_equal(r["mask"], p["planted"]), (k, len(p["xi"]))
    kinds = {p["kind"]: r for p, r in zip(pairs, res)}
    assert kinds["too_few"]["status"] == kinds["collinear"]["status"] == ref.VRO_TOO_FEW
    assert kinds["below_min"]["status"] == (ref.VRO_TOO_FEW if min_inliers == 8 or K == 1 else ref.VRO_OK)
    assert kinds["collinear"]["n_valid"] == 0 and kinds["collinear"]["best_hypothesis"] == -1
    if K > 1:
        assert kinds["below_min"]["n_valid"] > 0 and kinds["z_nonpositive"]["status"] == ref.VRO_NUM
        assert ok >= 20                                          # most of the batch registers
    print("K = %d: %d of %d pairs OK, smallest decided share %.3f" % (K, ok, len(pairs), min(r["decided"].mean() for r in res)))


def test_a_perturbation_of_1e_9_flips_no_count():
    rng = np.random.default_rng(5)
    for p, r in zip(ref.gpu_cases(), _results(256, 8)):
        xi = p["xi"] + 1e-9 * rng.uniform(-1, 1, p["xi"].shape); xj = p["xj"] + 1e-9 * rng.uniform(-1, 1, p["xj"].shape)
        c, _, _, _ = ref.score(xi, xj, dict(ref.DEFAULTS, hypotheses=256))
        assert np.array_equal(c[r["decided"]], r["hyp_counts"][r["decided"]])


def test_failed_pairs_carry_the_void_record_and_depend_on_nothing_else():
    r = ref.ransac_pair(np.zeros((2, 3)), np.zeros((2, 3)), hypotheses=16)
    assert r["status"] == ref.VRO_TOO_FEW and (r["best_hypothesis"], r["best_count"], r["n_valid"], r["rounds"]) == (-1, -1, 0, 0)
    assert np.array_equal(r["pose"], [0, 0, 0, 0, 0, 0, 1]) and np.array_equal(r["info"], 10000 * np.eye(6)) and not r["cov"].any()
    assert np.array_equal(r["hyp_counts"], np.full(16, -1)) and r["n_inliers"] == 0 and r["rmse"] == 0
    # refine_rounds = 0 reports the winner's own pose and inliers
    p = ref.make_pair(np.random.default_rng(6), 50, 0.3, 0.5)
    a = ref.ransac_pair(p["xi"], p["xj"], hypotheses=64, refine_rounds=0)
    assert a["status"] == ref.VRO_OK and a["rounds"] == 0 and a["n_inliers"] == a["best_count"]
    b = ref.ransac_pair(p["xi"], p["xj"], hypotheses=64)
    assert 1 <= b["rounds"] <= 3 and b["rmse"] <= a["rmse"] and np.array_equal(b["mask"], p["planted"])
    assert np.abs(ref.quat_matrix(b["pose"][3:]) - p["R"]).max() < 5e-3 and np.abs(b["pose"][:3] - p["t"]).max() < 1e-2
