"""Pins the numpy restatement of the plane extraction (tests/plane_extract_reference.py) on the CPU: it is the yardstick of
csrc/kernels_plane_extract.hip, so it has to be right on its own account.  The sampler is the VRO one, planted planes come back, a
corner gives its three walls, the sandwich covariance obeys the chi-square law on single-plane scenes, cov16 carries C, and every
case of the GPU test is well posed."""
import functools

import numpy as np
import pytest

from tests import plane_extract_reference as ref
from tests import vro_ransac_reference as vro


def test_the_sampler_is_the_vro_sampler_with_the_round_folded_in():
    for seed in (0, 12345, 2 ** 63 + 5):
        for M in (3, 4, 100, 25344):
            for h in (0, 1, 511, 65535):
                assert ref.sample3(seed, 0, h, 512, M) == vro.sample3(seed, h, M)
                for r, K in ((1, 512), (3, 100), (7, 65536)):
                    u = [ref.mix(seed + ((r * K + h) * 3 + k + 1) * ref.GOLDEN) for k in range(3)]
                    a = u[0] % M
                    b = u[1] % (M - 1); b += b >= a
                    c = u[2] % (M - 2); c += c >= min(a, b); c += c >= max(a, b)
                    got = ref.sample3(seed, r, h, K, M)
                    assert got == (a, b, c) and len(set(got)) == 3 and max(got) < M


def test_planted_planes_without_noise_come_back_to_rounding():
    rng = np.random.default_rng(1)
    # the fit alone, on points that lie on the plane to rounding: the normal is determined to rounding / g
    for _ in range(20):
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        B = ref.basis(n)
        p = (rng.uniform(-1, 1, (500, 2)) * rng.uniform(0.2, 2.0, 2)) @ B.T + rng.uniform(1.0, 3.0) * n
        d = -float(n @ p[0])
        n0, d0 = ref.orient(n, d)
        nf, df, c, w = ref.fit(p)
        g = ref.gap(w)
        assert g > 1e-2
        assert np.abs(nf - n0).max() <= 1e-13 / g and abs(df - d0) <= 1e-13 * (1 + np.linalg.norm(p, axis=1).max()) / g
    # the whole extraction: two fronto-parallel walls whose depths are whole depth words, so the points are exact
    W, H = 48, 40
    depth = np.full((H, W), 2000, np.uint16); depth[:, W // 2:] = 3000
    o = ref.extract_frame(depth, **ref.camera(W, H), hypotheses=64, min_pixels=W * H // 20)
    assert (o["status"], o["n_planes"]) == (ref.PX_OK, 2)
    assert sorted(o["n_pixels"][:2]) == [W * H // 2, W * H // 2] and set(np.unique(o["labels"])) == {0, 1}
    for k in range(2):
        truth = 2.0 if o["labels"][0, 0] == k else 3.0
        assert np.abs(o["abcd"][k] - [0, 0, -1, truth]).max() <= 1e-12 / o["g"][k], (k, o["abcd"][k])
        assert o["rmse"][k] <= 1e-12


def _angle(a, b):
    return np.degrees(np.arccos(min(1.0, abs(float(a @ b)))))


def test_a_corner_gives_its_three_walls():
    W, H = 48, 40
    rng = np.random.default_rng(2)
    found = 0
    for _ in range(5):
        depth, cam, truth = ref.make_frame("corner", W, H, rng)
        assert len(truth) == 3
        o = ref.extract_frame(depth, **cam, hypotheses=256, min_pixels=W * H // 20)
        assert (o["status"], o["n_planes"]) == (ref.PX_OK, 3)
        for n, d in truth:
            k = int(np.argmin([_angle(n, o["abcd"][j][:3]) for j in range(3)]))
            assert _angle(n, o["abcd"][k][:3]) <= 1.0 and abs(d - o["abcd"][k][3]) <= 0.02, (n, d, o["abcd"][:3])
            assert o["abcd"][k][:3] @ n > 0 and o["abcd"][k][3] > 0                 # the camera on the positive side
            found += 1
    assert found == 15


@pytest.mark.parametrize("yaw_deg", (0.0, 35.0, 60.0))
def test_the_sandwich_covariance_obeys_the_chi_square_law_on_one_plane(yaw_deg):
    """48 x 40, one wall, the default max_dist, sigma_px = 1e-3 (the render has no pixel noise): over N = 400 noise draws the mean of
    e^T C^-1 e, e the tangent difference to the true plane, lies within 5 sqrt(6 / N) of 3 (chi-square with 3 degrees: mean 3,
    variance 6)."""
    W, H, N = 48, 40, 400
    rng = np.random.default_rng(int(yaw_deg) + 3)
    cam = ref.camera(W, H)
    planes = ref.wall_scene(np.deg2rad(yaw_deg))
    m2 = []
    for _ in range(N):
        depth, wall = ref.render(planes, W, H, cam, 0.014, rng)
        truth = planes[int(np.bincount(wall[wall >= 0]).argmax())]
        o = ref.extract_frame(depth, **cam, hypotheses=16, min_pixels=W * H // 20, sigma_px=1e-3)
        assert (o["status"], o["n_planes"]) == (ref.PX_OK, 1)
        n, d = o["abcd"][0][:3], o["abcd"][0][3]
        e = np.append(ref.basis(n).T @ truth[0], truth[1] - d)
        C = np.zeros((3, 3)); C[np.triu_indices(3)] = o["cov_ut6"][0]; C = C + np.triu(C, 1).T
        m2.append(float(e @ np.linalg.solve(C, e)))
    mean = float(np.mean(m2))
    print("yaw %g deg: mean e^T C^-1 e = %.3f over %d draws (band 3 +- %.3f)" % (yaw_deg, mean, N, 5 * np.sqrt(6.0 / N)))
    assert abs(mean - 3.0) <= 5 * np.sqrt(6.0 / N), mean


def test_cov16_carries_the_tangent_covariance():
    W, H = 48, 40
    depth, cam, truth = ref.make_frame("corner", W, H, np.random.default_rng(4))
    o = ref.extract_frame(depth, **cam, hypotheses=128, min_pixels=W * H // 20)
    assert o["n_planes"] == 3
    for k in range(3):
        B = ref.basis(o["abcd"][k][:3])
        C = np.zeros((3, 3)); C[np.triu_indices(3)] = o["cov_ut6"][k]; C = C + np.triu(C, 1).T
        S = o["cov16"][k]
        scale = np.abs(C).max()
        assert np.array_equal(S, S.T) and np.all(np.linalg.eigvalsh(C) > 0)
        assert np.abs(B.T @ S[:3, :3] @ B - C[:2, :2]).max() <= 1e-13 * scale and abs(S[3, 3] - C[2, 2]) <= 1e-13 * scale
        assert np.abs(B.T @ S[:3, 3] - C[:2, 2]).max() <= 1e-13 * scale
    # the slots past n_planes are zero
    assert not o["abcd"][3:].any() and not o["cov16"][3:].any() and not o["cov_ut6"][3:].any()


@functools.lru_cache(maxsize=None)
def _cases():
    calls = ref.gpu_cases()
    return calls, [[ref.extract_frame(f, **ref.call_params(c)) for f in c["depth"]] for c in calls]


def test_every_gpu_case_is_well_posed():
    """what lets the GPU test compare counts, labels and statuses exactly and values to 1e-11 times a condition number: at most
    1 % of a frame's hypotheses undecided, no later decision within 1e-9 of its threshold, every fit's gap at least 1e-3,
    cond(A) at most 1e6, no winner or fit with |d| below 1e-6 (its orientation would hang on rounding); and the scenes give what
    they were built for"""
    calls, outs = _cases()
    pixels = {(c["W"], c["H"]) for c in calls}
    assert {w * h for w, h in pixels} >= {16 * 12, 48 * 40, ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1, 176 * 144}
    assert {c["hypotheses"] for c in calls} == {1, 100, ref.PASS, ref.PASS + 8}
    for c, frames in zip(calls, outs):
        for kind, o in zip(c["kinds"], frames):
            tag = (c["W"], c["H"], c["hypotheses"], kind)
            run = o["decided"][:o["rounds_run"]]
            assert run.size == 0 or 1.0 - run.mean() <= 0.01, tag
            assert o["margin"] >= 1e-9 and o["g_min"] >= 1e-3 and o["cond_A"].max() <= 1e6 and o["status"] == ref.PX_OK, tag
            assert o["d_min"] >= 1e-6, tag
            assert np.all(o["hyp_counts"][o["rounds_run"]:] == -2) and np.all(o["hyp_counts"][:o["rounds_run"]] >= -1), tag
            if kind == "zero":
                assert (o["n_valid_pixels"], o["rounds_run"], o["n_planes"]) == (0, 0, 0) and np.all(o["labels"] == -2), tag
            if kind == "few":
                assert 0 < o["n_valid_pixels"] < c["min_pixels"] and (o["rounds_run"], o["n_planes"]) == (0, 0), tag
            if c["hypotheses"] >= 100:
                if kind == "corner_one_plane":
                    assert o["n_planes"] == 1 and np.sum(o["labels"] == -1) >= 2 * c["min_pixels"], tag
                if kind in ("wall", "outliers") and c["W"] * c["H"] >= 1000 and c["H"] > 3:
                    assert o["n_planes"] == 1, tag
                if kind == "corner":
                    assert o["n_planes"] == 3, tag
