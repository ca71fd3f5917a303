"""Pins the numpy restatement of the plane propagation (tests/plane_propagate_reference.py) on the CPU: it is the yardstick of
csrc/kernels_plane_propagate.hip, so it has to be right on its own account.  The literal queue of the reference's regionGrow and the
closure the header defines agree on every case of the GPU test, the prediction is plane_check_reference's, the transform has GTSAM's
known answer, every case does what its name says, and every case is well posed: no decision within 1e-9 of its threshold and no
refitted plane within 10 max_dist = 0.5 m of the camera."""
import functools

import numpy as np
import pytest

from tests import plane_check_reference as pcr
from tests import plane_propagate_reference as pp

SHAPES = ["%dx%d" % s for s in pp.SHAPES]


@functools.lru_cache(maxsize=None)
def call(i):
    return pp.make_call(*pp.SHAPES[i], pp.SEEDS[pp.SHAPES[i]])


@functools.lru_cache(maxsize=None)
def closure(i, p):
    return pp.reference_of(call(i), p)


def pair(i, name):
    return [p["name"] for p in call(i)["pairs"]].index(name)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPES)
def test_queue_and_closure_agree(i):
    c = call(i)
    for p, pr in enumerate(c["pairs"]):
        a, b = closure(i, p), pp.reference_of(c, p, growth="queue")
        for k in ("status", "n_planes", "num_added", "search_rest"):
            assert a[k] == b[k], (pr["name"], k)
        for k in ("labels", "n_pixels", "n_seed", "source", "kept", "n_prev", "pred_n_seed", "abcd", "cov16", "rmse"):
            assert np.array_equal(a[k], b[k]), (pr["name"], k)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPES)
def test_every_case_is_well_posed(i):
    c = call(i)
    for p, pr in enumerate(c["pairs"]):
        o = closure(i, p)
        assert o["margin"] >= pp.DECIDE, (pr["name"], o["margin"])          # zero undecided decisions: a condition, not a measurement
        assert o["keep_margin"] >= 1, pr["name"]
        assert o["d_min"] >= 0.5, (pr["name"], o["d_min"])
        k = o["n_planes"]
        assert np.all(o["g"][:k] >= 1e-3), (pr["name"], o["g"][:k])


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPES)
def test_prediction_is_the_plane_check_s(i):
    c = call(i)
    p = pair(i, "large-covariance")
    pr = c["pairs"][p]
    k = int(c["n_planes"][pr["i"]])
    o = closure(i, p)
    w = pcr.check_record(pr["pose"], c["abcd"][pr["i"], :k], c["cov16"][pr["i"], :k], np.zeros((0, 4)), np.zeros((0, 16)), cov=pr["S"])
    assert np.allclose(o["pred_abcd"][:k], w["pred_abcd"], rtol=1e-14, atol=1e-15)
    assert np.allclose(o["sdj"][:k], w["sdj"], rtol=1e-14, atol=0) and np.all(o["sdj"][:k] > 0.014 ** 2)


def test_transform_known_answer():
    """gtsam/test/testOrientedPlane3.cpp:61-70: the plane (-1, 0, 0, 5) seen from Pose3(Ypr(-pi / 4, 0, 0), (2, 3, 4))"""
    y = -np.pi / 4
    pose = np.array([2.0, 3.0, 4.0, 0.0, 0.0, np.sin(y / 2), np.cos(y / 2)])
    (pe, sdj) = pp.predict(np.array([-1.0, 0, 0, 5]), np.zeros(16), pose, np.zeros((3, 3)))
    assert np.allclose(pe, [-np.sqrt(2) / 2, -np.sqrt(2) / 2, 0.0, 3.0], atol=1e-9) and sdj == 0.0


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPES)
def test_every_case_does_what_its_name_says(i):
    c = call(i)
    W, H = pp.SHAPES[i]
    big = W * H >= 48 * 40                                            # a corner rendered on 3 rows or 192 pixels keeps no promise
    by = {pr["name"]: closure(i, p) for p, pr in enumerate(c["pairs"])}
    assert len(by) == 10
    o = by["no-planes"]
    assert (o["status"], o["n_planes"], o["num_added"], o["search_rest"]) == (pp.PP_OK, 0, 0, 2) and set(np.unique(o["labels"])) <= {-1, -2}
    o = by["not-positive-definite"]
    assert (o["status"], o["search_rest"]) == (pp.PP_NUM, 2) and not o["abcd"].any() and set(np.unique(o["labels"])) <= {-1, -2}
    o = by["eight-planes"]
    assert o["n_planes"] == 8 and list(o["source"]) == list(range(8)) and np.array_equal(o["labels"], c["labels"][c["pairs"][pair(i, "eight-planes")]["i"]])
    o = by["rectangle"]                                               # the growth stops at the rectangle although the geometry fits
    inside = o["labels"][H // 3:max(H // 3 + 1, 2 * H // 3), W // 3:2 * W // 3]
    assert o["n_planes"] == 1 and o["joined"][0] > 0 and np.all(inside[1:, 1:] == -1) and o["n_pixels"][0] >= W * H - inside.size - 1
    o = by["serpentine"]                                              # every corridor row is reached, no barrier pixel but the gaps
    lab = o["labels"]
    assert o["n_planes"] == 1 and np.all(lab[0::2] == 0) and np.all(lab[1::2].sum(1) == -(W - 1))
    o = by["block-and-conduct"]
    r1, c1 = max(2, H // 3), W // 2
    lab = o["labels"]
    assert o["n_planes"] == 2 and list(o["kept"][:2]) == [1, 1]
    assert np.all(lab[r1, :max(1, c1 // 4)] == -3)                    # lost to plane 1: they lie on its plane
    assert np.all(lab[:r1, :c1] == 0) and np.all(lab[r1, max(1, c1 // 4):c1] == 1) and np.all(lab[r1 + 1:] == 1) and np.all(lab[r1, c1:] == -1)
    o = by["large-covariance"]
    assert o["n_by_sdj"] > 0 and by["small-motion"]["n_by_sdj"] <= o["n_by_sdj"]
    if big:
        o = by["identity"]
        assert o["n_planes"] == 3 and np.all(o["n_pixels"][:3] >= 0.85 * o["n_prev"][:3])
        o = by["small-motion"]
        assert o["n_planes"] == 3 and np.all(o["joined"][:3] > 0)
        o = by["wall-dropped"]
        assert list(o["kept"][:3]) == [1, 1, 0] and o["pred_n_seed"][2] > 0 and np.sum(o["labels"] == -4) == o["pred_n_seed"][2]
        assert o["num_added"] == o["n_pixels"][:2].sum() + o["pred_n_seed"][2]
        assert by["large-covariance"]["n_by_sdj"] > 100


def test_codes_of_the_label_image_and_the_record():
    c = call(2)
    o = closure(2, pair(2, "wall-dropped"))
    assert set(np.unique(o["labels"])) <= {-4, -3, -2, -1, 0, 1} and (o["labels"] == -3).any()
    for k in range(o["n_planes"]):
        assert np.sum(o["labels"] == k) == o["n_pixels"][k] == o["n_seed"][k] + o["joined"][k]
    # search_rest: 0 above rest_ratio W H, 1 below
    assert o["search_rest"] == 0 and pp.reference_of(c, pair(2, "wall-dropped"), rest_ratio=1.0)["search_rest"] == 1
    # keep_ratio = 1 drops what does not gain pixels, keep_ratio = 0 keeps whatever has a seed
    assert pp.reference_of(c, pair(2, "wall-dropped"), keep_ratio=0.0)["n_planes"] == 3
