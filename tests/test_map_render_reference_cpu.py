"""The numpy restatement of the map rendering (tests/map_render_reference.py) held to an independently written brute force on the
CPU: plain Python floats and integers, a loop over every pixel and every point, the minimum of the tuple (zq, index) -- no shared
code with the restatement but the pose arithmetic of the fusion's restatement, which has its own CPU test.  Then the properties the
GPU test leans on: the hand-checkable rows of the tiny case, the permutation invariance, the depth check's classes, and look_at."""
import math

import numpy as np

import graph_slam_amd as G
from tests import map_fuse_reference as mf
from tests import map_render_reference as ref


def brute(c):
    """every pixel x every point; returns zq, index (V x H x W), the colour image and the counts, from the semantics of the header"""
    P = dict(ref.DEFAULTS, **{k: v for k, v in c.items() if k in ref.DEFAULTS})
    W, H = c["width"], c["height"]
    x = [[float(a) for a in row] for row in c["xyz"]]
    poses = np.asarray(c["pose_w"]).reshape(-1, 7)
    depth = c.get("depth")
    tq = int(round(P["agree_tol"] * 2.0 ** 20))                   # Python's round is ties-to-even, like llrint
    out = dict(zq=[], index=[], counts=[])
    for v, pose in enumerate(poses):
        rt = [float(a) for a in ref.view_rt(pose, c.get("extrinsic"), c.get("view_offset"))]
        R, t = [rt[0:3], rt[3:6], rt[6:9]], rt[9:12]
        foot = []                                                 # (zq, index, u_lo, u_hi, v_lo, v_hi) of the drawn points
        n_valid = n_drawn = 0
        for i, p in enumerate(x):
            if not all(math.isfinite(a) for a in p):
                continue
            d = [p[k] - t[k] for k in range(3)]
            q = [(R[0][k] * d[0] + R[1][k] * d[1]) + R[2][k] * d[2] for k in range(3)]
            z = q[2]
            if not (P["z_min"] < z < P["z_max"]):
                continue
            n_valid += 1
            uf, vf = ((P["fx"] * q[0]) / z) + P["cx"], ((P["fy"] * q[1]) / z) + P["cy"]
            if not (-2.0 ** 30 < uf < 2.0 ** 30 and -2.0 ** 30 < vf < 2.0 ** 30):
                continue
            u0, v0 = math.floor(uf + 0.5), math.floor(vf + 0.5)
            s = min(math.floor((P["fx"] * P["radius"]) / z), P["max_half"]) if P["radius"] > 0 else 0
            h = min(P["max_half"], P["splat"] + s)
            lo_u, hi_u, lo_v, hi_v = max(u0 - h, 0), min(u0 + h, W - 1), max(v0 - h, 0), min(v0 + h, H - 1)
            if lo_u > hi_u or lo_v > hi_v:
                continue
            n_drawn += 1
            foot.append((int(round(z * 2.0 ** 20)), i, lo_u, hi_u, lo_v, hi_v))
        zq = np.full((H, W), -1, np.int64); index = np.full((H, W), -1, np.int64)
        cnt = dict(n_valid=n_valid, n_drawn=n_drawn, n_pixels=0, n_meas=0, n_both=0, n_agree=0, n_closer=0, n_through=0)
        for b in range(H):
            for a in range(W):
                best = min(((f[0], f[1]) for f in foot if f[2] <= a <= f[3] and f[4] <= b <= f[5]), default=None)
                if best is not None:
                    zq[b, a], index[b, a] = best
                    cnt["n_pixels"] += 1
                if depth is None:
                    continue
                zm = float(depth[v, b, a]) * P["z_scale"]
                if not (P["z_min"] < zm < P["z_max"]):
                    continue
                cnt["n_meas"] += 1
                if best is None:
                    continue
                mq = int(round(zm * 2.0 ** 20))
                cnt["n_both"] += 1
                cnt["n_agree"] += abs(mq - best[0]) <= tq
                cnt["n_closer"] += mq < best[0] - tq
                cnt["n_through"] += mq > best[0] + tq
        out["zq"].append(zq); out["index"].append(index); out["counts"].append(cnt)
    return out


def _args(c):
    return {k: v for k, v in c.items() if k != "want"}


def _small(name, n, views=None):
    """a case cut down to its first n points (and some of its views), small enough for the brute force"""
    c = _args(ref.case(name))
    c = dict(c, xyz=c["xyz"][:n], color=None if c["color"] is None else c["color"][:n])
    if views is not None:
        c["pose_w"] = c["pose_w"][views]
    return c


def test_restatement_equals_the_brute_force():
    cases = [_args(ref.case(n)) for n in ("tiny", "ties", "footprints", "footprints_radius")]
    cases.append(_small("many_views_rgb", 150, [0, 137, 299]))    # extrinsic and the chase camera
    cases.append(dict(_small("strips_200x83", 400), width=40, height=17, fx=36.0, fy=36.0, cx=19.5, cy=8.0))
    cases.append(_small("depth_check", 250))                       # the depth words were made for the whole cloud: every class still occurs
    for c in cases:
        want, got = brute(c), ref.render(**c)
        for v in range(len(want["zq"])):
            assert np.array_equal(got["zq"][v], want["zq"][v]) and np.array_equal(got["index"][v], want["index"][v])
            for f, n in want["counts"][v].items():
                assert got[f][v] == n, (f, v)
            if c["color"] is not None:
                col = np.asarray(c["color"]).reshape(len(c["xyz"]), -1)
                img = got["color"][v].reshape(c["height"], c["width"], -1)
                cov = want["index"][v] >= 0
                assert np.array_equal(img[cov], col[want["index"][v][cov]])
                assert np.all(img[~cov] == np.asarray(ref.DEFAULTS["background"], np.uint8)[:col.shape[1]])


def test_the_tiny_case_by_hand():
    w = ref.case("tiny")["want"]
    covered = {(4, 3): (0, 1.0), (2, 2): (1, 2.0), (1, 1): (2, 1.0), (7, 5): (12, 1.0), (0, 0): (13, 1.0)}       # (u, v): (index, z)
    for v in range(6):
        for u in range(8):
            i, z = covered.get((u, v), (-1, None))
            assert w["index"][0, v, u] == i and w["zq"][0, v, u] == (-1 if z is None else int(z * 2 ** 20)), (u, v)
    assert (w["n_valid"][0], w["n_drawn"][0], w["n_pixels"][0], w["n_nonfinite"], w["n_points"]) == (10, 6, 5, 2, 15)
    t = ref.case("ties")["want"]
    assert t["index"][0, 3, 4] == 1 and t["index"][0, 3, 5] == 3 and t["index"][0, 3, 2] == 7          # equal zq: the smaller index; the nearer of two


def test_permutation_changes_only_the_index_and_only_through_the_permutation():
    c = _args(ref.case("strips_200x83"))
    a = ref.render(**c)
    perm = np.random.default_rng(3).permutation(len(c["xyz"]))
    b = ref.render(**dict(c, xyz=c["xyz"][perm], color=c["color"][perm]))
    assert np.array_equal(a["zq"], b["zq"]) and all(np.array_equal(a[f], b[f]) for f in ref.VIEW_FIELDS)
    cov = a["index"] >= 0
    assert np.array_equal(perm[b["index"][cov]], a["index"][cov]) and np.array_equal(a["color"], b["color"])         # no ties in a random cloud


def test_depth_check_has_every_class_and_they_add_up():
    w = ref.case("depth_check")["want"]
    for v in range(2):
        assert w["n_agree"][v] + w["n_closer"][v] + w["n_through"][v] == w["n_both"][v] < w["n_meas"][v]
        assert w["n_both"][v] < w["n_pixels"][v]                  # the invalid words on covered pixels
        # of six covered pixels in a row: three agree (0, +tq, -tq), one is closer, one goes through, one is not measured
        assert abs(w["n_agree"][v] - 0.5 * w["n_pixels"][v]) < 60 and min(w["n_closer"][v], w["n_through"][v]) > 0.1 * w["n_pixels"][v]


def test_look_at_is_a_rotation_and_the_target_renders_at_the_principal_point():
    rng = np.random.default_rng(8)
    views = [((0, -2, -5), (0, 0, 5), (0, -0.98, 0.199)), ((1, 2, 3), (1, 2, 4), (0, -1, 0)), ((0, 0, 0), (0, 0, -1), (0, -1, 0)),
             ((0, 0, 0), (-1, 0, 0), (0, -1, 0)), ((0, 0, 0), (0, 1, 0), (0, 0, 1))]
    views += [(rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)) for _ in range(40)]
    P = dict(fx=30.0, fy=30.0, cx=10.0, cy=7.0, z_min=1e-3, z_max=100.0)
    for eye, target, up in views:
        pose = G.look_at(eye, target, up)
        eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
        assert pose.shape == (7,) and np.array_equal(pose[:3], eye) and abs(pose[3:] @ pose[3:] - 1) < 1e-15
        R = G.look_at_matrix(eye, target, up)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
        # the quaternion carries R: its components are good to a few eps, an entry of its matrix is 1 - 2 (a a + b b) or 2 (a b + c d)
        # of them, so 16 eps bounds the difference
        assert np.abs(mf.quat_matrix(pose[3:]) - R).max() < 16 * np.finfo(float).eps
        z = (target - eye) / np.linalg.norm(target - eye)
        assert np.abs(R[:, 2] - z).max() < 1e-15                  # z forward
        assert abs(R[:, 0] @ up) < 1e-15 and R[:, 1] @ up < 0     # x is level, y points down: against up
        o = ref.render(np.array([target]), pose[None], width=21, height=15, **P)
        assert o["n_pixels"][0] == 1 and o["index"][0, 7, 10] == 0          # the pixel nearest (cx, cy)
    assert np.abs(G.look_at(ref.CHASE_EYE, ref.CHASE_TARGET, ref.CHASE_UP) - ref.chase_offset()).max() < 1e-15


def test_the_strip_cases_have_footprints_across_every_strip_boundary():
    """what the GPU test's strip cases are for: at every boundary between two strips of the tiles form some drawn footprint covers
    the last row of one strip and the first row of the next; the last strip of 200 x 83 is partial and its pixel count no multiple
    of 256; the widest image the tiles form takes has one row per strip, and one more column runs in the global form"""
    for name in ("strips_176x144", "strips_200x83", "width_1", "widest_tiles"):
        c = _args(ref.case(name))
        W, H = c["width"], c["height"]
        form, rows = ref.form_fields(ref.TILES, W)
        assert form == ref.TILES and rows == max(1, 8192 // W)
        P = dict(ref.DEFAULTS, **{k: v for k, v in c.items() if k in ref.DEFAULTS})
        rt = ref.view_rt(c["pose_w"][0])
        valid, drawn, zq, u0, v0, h = ref.project(c["xyz"], np.all(np.isfinite(c["xyz"]), 1), rt, P, W, H)
        bounds = list(range(rows, H, rows))
        assert len(bounds) == -(-H // rows) - 1
        for r in bounds:                                          # rows r - 1 and r belong to different strips
            assert np.any(drawn & (v0 - h <= r - 1) & (v0 + h >= r) & (u0 + h >= 0) & (u0 - h < W)), (name, r)
    assert ref.form_fields(ref.TILES, 176) == (ref.TILES, 46) and 144 % 46 != 0
    assert ref.form_fields(ref.TILES, 200) == (ref.TILES, 40) and 83 % 40 == 3 and (3 * 200) % 256 != 0
    assert ref.form_fields(ref.TILES, ref.STRIP) == (ref.TILES, 1) and ref.form_fields(ref.TILES, ref.STRIP + 1) == (ref.GLOBAL, 0)
    one = ref.case("one_pixel")["want"]
    assert one["n_pixels"][0] == 1 and one["n_drawn"][0] == 20000 and len(np.unique(np.rint(ref.case("one_pixel")["xyz"][:, 2] * 2.0 ** 20))) == 20000
