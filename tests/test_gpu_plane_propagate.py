"""The batched plane propagation (csrc/kernels_plane_propagate.hip, fgo_plane_propagate_batch: one workgroup per pair, all pairs in
one launch) against its numpy restatement (tests/plane_propagate_reference.py, itself pinned by
tests/test_plane_propagate_reference_cpu.py).

W and H belong to a call, so there is one call per shape (plane_propagate_reference.gpu_cases): 16 x 12 (fewer pixels than lanes),
67 x 3 (odd), 48 x 40, 176 x 144 (the reference's frame), 256 x 256 (the last shape whose flag and intensity bytes fit in LDS) and
257 x 256 (the first in device scratch).  Each call has ten pairs: the identity on one frame, a small motion of the three-wall corner,
a motion that leaves a wall under 70 % of its support, a wall with a rectangle of another intensity, a serpentine of intensity barriers
open at alternating ends with the previous support in one corner (what a capped or one-directional sweep gets wrong), a previous
frame without planes, a pose 3 cm off under a covariance that says so (the S_dj branch admits the pixels), two planes of which the
first's REJECTED pixels block the second and the first's claimed pixels conduct it, an information that is not positive definite,
and a previous frame with eight planes.  Every case is well posed (test_plane_propagate_reference_cpu.py): no decision within 1e-9 of
its threshold, so NOTHING is undecided.

Compared exactly: the label image, every count, kept, source, search_rest, the status.  Tolerances: pred abcd and sdj relative 1e-11
(the information of every pair is diagonal: condition 1); the refit as tests/test_gpu_plane_extract.py holds the extraction's, the
project's per-value tolerance 1e-11 times the condition numbers the restatement computes, with g = min(1, (l1 - l0) / l2):
  n      1e-11 / g                          d, centroid, rmse   1e-11 (1 + p_max) / g
  C, cov16   1e-11 cond(A) / g of their largest entry"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_slam_amd as G
from tests import plane_extract_reference as ref
from tests import plane_propagate_reference as pp

TOL = 1e-11
IDS = ["%dx%d" % s for s in pp.SHAPES]
FIELDS = ("status", "n_planes", "num_added", "search_rest", "abcd_all", "cov16_all", "cov_ut6_all", "n_pixels", "n_seed", "source", "rmse",
          "centroid", "pred_abcd", "sdj", "n_prev", "pred_n_seed", "kept", "labels")


def run(c, pairs=None, use="info", **kw):
    ps = c["pairs"] if pairs is None else [c["pairs"][p] for p in pairs]
    s = dict(info=pp.info_of(dict(pairs=ps))) if use == "info" else dict(cov=np.array([p["S"] for p in ps]))
    return G.plane_propagate_batch(c["depth"], c["intensity"], c["labels"], c["n_planes"], c["abcd"], c["cov16"], [p["i"] for p in ps],
                                   [p["j"] for p in ps], np.array([p["pose"] for p in ps]), params=G.plane_propagate_params(**c["cam"]), **s, **kw)


@functools.lru_cache(maxsize=None)
def case(i):
    """call i: the restatement's pairs and the entry point's output, computed once and shared"""
    c = pp.make_call(*pp.SHAPES[i], pp.SEEDS[pp.SHAPES[i]])
    return c, [pp.reference_of(c, p) for p in range(len(c["pairs"]))], run(c)


def same_pair(a, pa, b, pb, what):
    for f in FIELDS:
        assert a[f][pa].tobytes() == b[f][pb].tobytes(), (what, f)


@pytest.mark.parametrize("i", range(len(IDS)), ids=IDS)
def test_labels_counts_and_statuses_equal_the_reference(i):
    c, want, g = case(i)
    for p, w in enumerate(want):
        name = c["pairs"][p]["name"]
        for k in ("status", "n_planes", "num_added", "search_rest"):
            assert g[k][p] == w[k], (name, k, g[k][p], w[k])
        for k in ("n_prev", "pred_n_seed", "kept", "n_pixels", "n_seed", "source"):
            assert np.array_equal(g[k][p], w[k]), (name, k, g[k][p], w[k])
        assert np.array_equal(g["labels"][p], w["labels"]), (name, int(np.sum(g["labels"][p] != w["labels"])))
    print("%s: planes kept per pair %s, num_added %s" % (IDS[i], list(g["n_planes"]), list(g["num_added"])))
    assert np.array_equal(g["ptr"], np.concatenate([[0], np.cumsum(g["n_planes"])]))
    assert G.lib.fgo_debug_plane_propagate_kernel_ms() > 0


@pytest.mark.parametrize("i", range(len(IDS)), ids=IDS)
def test_predictions_planes_and_covariances_against_the_reference(i):
    c, want, g = case(i)
    worst = {}
    for p, w in enumerate(want):
        name = c["pairs"][p]["name"]
        npl = 0 if w["status"] else int(c["n_planes"][c["pairs"][p]["i"]])
        for l in range(npl):
            err = dict(pred=np.abs(g["pred_abcd"][p][l] - w["pred_abcd"][l]).max() / (TOL * np.abs(w["pred_abcd"][l]).max()),
                       sdj=abs(g["sdj"][p][l] - w["sdj"][l]) / (TOL * w["sdj"][l]))
            for nm, e in err.items():
                assert e <= 1.0, (name, l, nm, e)
            worst = {nm: max(e, worst.get(nm, 0.0)) for nm, e in err.items()}
        for l in range(npl, pp.MAX_PLANES):                        # the slots past the last previous plane are zero
            assert not g["pred_abcd"][p][l].any() and g["sdj"][p][l] == 0 and g["n_prev"][p][l] == 0 and g["kept"][p][l] == 0, (name, l)
        for k in range(w["n_planes"], pp.MAX_PLANES):              # and so are those past the last kept plane
            assert not g["abcd_all"][p][k].any() and not g["cov16_all"][p][k].any() and not g["cov_ut6_all"][p][k].any(), (name, k)
            assert g["n_pixels"][p][k] == 0 and g["rmse"][p][k] == 0 and not g["centroid"][p][k].any(), (name, k)
        for k in range(w["n_planes"]):
            gg, pm = w["g"][k], 1 + w["p_max"]
            abcd, S, C6 = g["abcd_all"][p][k], g["cov16_all"][p][k], g["cov_ut6_all"][p][k]
            assert abs(abcd[:3] @ abcd[:3] - 1) <= 1e-14 and abcd[3] >= 0 and np.array_equal(S, S.T), (name, k)
            ctol = TOL * w["cond_A"][k] / gg
            err = dict(n=np.abs(abcd[:3] - w["abcd"][k][:3]).max() / (TOL / gg),
                       d=abs(abcd[3] - w["abcd"][k][3]) / (TOL * pm / gg),
                       centroid=np.abs(g["centroid"][p][k] - w["centroid"][k]).max() / (TOL * pm / gg),
                       rmse=abs(g["rmse"][p][k] - w["rmse"][k]) / (TOL * pm / gg),
                       C=np.abs(C6 - w["cov_ut6"][k]).max() / (ctol * np.abs(w["cov_ut6"][k]).max()),
                       cov16=np.abs(S - w["cov16"][k]).max() / (ctol * np.abs(w["cov16"][k]).max()))
            for nm, e in err.items():
                assert e <= 1.0, (name, k, nm, e, gg, w["cond_A"][k])
            worst = {nm: max(e, worst.get(nm, 0.0)) for nm, e in err.items()}
    print("%s: largest error as a share of its bound: %s" % (IDS[i], ", ".join("%s %.1e" % ne for ne in worst.items())))
    keep = np.arange(pp.MAX_PLANES)[None, :] < g["n_planes"][:, None]
    assert g["abcd"].tobytes() == g["abcd_all"][keep].tobytes() and g["cov16"].tobytes() == g["cov16_all"][keep].tobytes()
    assert g["cov_ut6"].tobytes() == g["cov_ut6_all"][keep].tobytes()


def test_two_calls_are_bit_identical_and_outputs_are_optional():
    for i in (IDS.index("67x3"), IDS.index("176x144"), IDS.index("257x256")):
        c, want, g = case(i)
        again = run(c)
        for p in range(len(c["pairs"])):
            same_pair(again, p, g, p, (IDS[i], p))
    c, want, g = case(IDS.index("48x40"))
    bare = run(c, want_labels=False, want_pred=False, want_planes=False, want_ut6=False)
    assert set(bare) == {"status", "n_planes", "num_added", "search_rest", "abcd_all", "cov16_all", "ptr", "abcd", "cov16"}
    for f in bare:
        assert bare[f].tobytes() == g[f].tobytes(), f


def test_a_pair_alone_equals_the_pair_in_the_batch():
    for i, pairs in ((IDS.index("48x40"), range(10)), (IDS.index("256x256"), (1, 7)), (IDS.index("257x256"), (1, 7))):
        c, want, g = case(i)
        for p in pairs:
            same_pair(run(c, pairs=[p]), 0, g, p, (IDS[i], c["pairs"][p]["name"]))
    # the place in the batch does not matter either
    c, want, g = case(IDS.index("48x40"))
    back = run(c, pairs=list(range(10))[::-1])
    for p in range(10):
        same_pair(back, 9 - p, g, p, ("reversed", p))


def test_the_covariance_as_given_is_the_other_way_in():
    """cov36 instead of info_ut21: the same pairs (but the one whose information is not positive definite) against the same reference"""
    c, want, g = case(IDS.index("48x40"))
    pairs = [p for p, pr in enumerate(c["pairs"]) if pr["S"] is not None]
    o = run(c, pairs=pairs, use="cov")
    for r, p in enumerate(pairs):
        w = want[p]
        assert (o["status"][r], o["n_planes"][r], o["num_added"][r], o["search_rest"][r]) == (w["status"], w["n_planes"], w["num_added"], w["search_rest"])
        assert np.array_equal(o["labels"][r], w["labels"]) and np.array_equal(o["n_pixels"][r], w["n_pixels"]), c["pairs"][p]["name"]
        k = int(c["n_planes"][c["pairs"][p]["i"]])
        assert np.all(np.abs(o["sdj"][r][:k] - w["sdj"][:k]) <= TOL * w["sdj"][:k]), c["pairs"][p]["name"]


def test_other_parameters_reach_the_kernel():
    c, want, g = case(IDS.index("48x40"))
    pairs = [p for p, pr in enumerate(c["pairs"]) if pr["name"] in ("small-motion", "wall-dropped", "rectangle", "serpentine")]
    for kw in (dict(intensity_tol=0), dict(intensity_tol=120), dict(keep_ratio=0.0), dict(keep_ratio=1.0), dict(rest_ratio=1.0), dict(d_floor=0.004),
               dict(z_min=1.0005, z_max=2.4005)):                       # between two depth words
        ps = [c["pairs"][p] for p in pairs]
        o = G.plane_propagate_batch(c["depth"], c["intensity"], c["labels"], c["n_planes"], c["abcd"], c["cov16"], [p["i"] for p in ps],
                                    [p["j"] for p in ps], np.array([p["pose"] for p in ps]), info=pp.info_of(dict(pairs=ps)),
                                    params=G.plane_propagate_params(**dict(c["cam"], **kw)))
        for r, p in enumerate(pairs):
            w = pp.reference_of(c, p, **kw)
            assert w["margin"] >= pp.DECIDE, (kw, p)
            assert (o["status"][r], o["n_planes"][r], o["num_added"][r], o["search_rest"][r]) == (w["status"], w["n_planes"], w["num_added"], w["search_rest"]), (kw, p)
            assert np.array_equal(o["labels"][r], w["labels"]) and np.array_equal(o["kept"][r], w["kept"]), (kw, c["pairs"][p]["name"])


def test_the_output_feeds_the_next_pair():
    """the labels and planes the small motion gives for frame b are a previous frame in their turn: carried back into frame a"""
    c, want, g = case(IDS.index("48x40"))
    p = [pr["name"] for pr in c["pairs"]].index("small-motion")
    pr = c["pairs"][p]
    R, t = pp.pcr.qmat(pr["pose"][3:]), pr["pose"][:3]
    back = np.concatenate([-R.T @ t, ref.vro_quat(R.T)])
    depth = np.stack([c["depth"][pr["j"]], c["depth"][pr["i"]]]); inten = np.stack([c["intensity"][pr["j"]], c["intensity"][pr["i"]]])
    labels = np.stack([g["labels"][p], np.full_like(g["labels"][p], -1)])
    npl = np.array([g["n_planes"][p], 0], np.int32)
    abcd = np.stack([g["abcd_all"][p], np.zeros((8, 4))]); cov16 = np.stack([g["cov16_all"][p].reshape(8, 16), np.zeros((8, 16))])
    assert {-3, 0, 1, 2} <= set(np.unique(labels[0]))               # the codes below -2 come back in
    o = G.plane_propagate_batch(depth, inten, labels, npl, abcd, cov16, [0], [1], back[None], cov=pp.SMALL_COV[None],
                                params=G.plane_propagate_params(**c["cam"]))
    k = int(npl[0])
    w = pp.propagate_pair(depth[0], labels[0], abcd[0, :k], cov16[0, :k], depth[1], inten[1], back, pp.SMALL_COV, **c["cam"])
    assert w["margin"] >= pp.DECIDE and w["n_planes"] == 3
    assert (o["status"][0], o["n_planes"][0], o["num_added"][0]) == (w["status"], w["n_planes"], w["num_added"])
    assert np.array_equal(o["labels"][0], w["labels"]) and np.array_equal(o["n_pixels"][0], w["n_pixels"])


def test_the_extraction_feeds_the_propagation_and_plane_node_completes_it():
    """plane_extract_batch's labels and planes go straight in; plane_node_batch on a previous frame without planes is plane_extract_batch
    on the raw frame"""
    c, want, g = case(IDS.index("48x40"))
    W, H = 48, 40
    p = [pr["name"] for pr in c["pairs"]].index("small-motion")
    pr = c["pairs"][p]
    X = G.plane_extract_params(**dict(c["cam"], hypotheses=256, min_pixels=W * H // 20))
    ex = G.plane_extract_batch(c["depth"], params=X, want_labels=True)
    assert ex["n_planes"][pr["i"]] == 3
    o = G.plane_propagate_batch(c["depth"], c["intensity"], ex["labels"], ex["n_planes"], ex["abcd_all"], ex["cov16_all"], [pr["i"]], [pr["j"]],
                                pr["pose"][None], cov=pp.SMALL_COV[None], params=G.plane_propagate_params(**c["cam"]))
    assert o["status"][0] == G.FGO_PP_OK and o["n_planes"][0] == 3 and sorted(o["source"][0][:3]) == [0, 1, 2]
    assert o["num_added"][0] > 0.9 * W * H and o["search_rest"][0] == 0
    z = [pr_["name"] for pr_ in c["pairs"]].index("no-planes")
    pz = c["pairs"][z]
    node = G.plane_node_batch(c["depth"], c["intensity"], c["labels"], c["n_planes"], c["abcd"], c["cov16"], [pz["i"]], [pz["j"]], pz["pose"][None],
                              cov=pp.SMALL_COV[None], params=G.plane_propagate_params(**c["cam"]), extract_params=X)
    k = int(ex["n_planes"][pz["j"]])
    assert node["search_rest"][0] == 2 and node["n_planes"][0] == node["n_new"][0] == k == 3 and np.all(node["source"][0][:k] == -1)
    for f in ("abcd_all", "cov16_all", "cov_ut6_all", "n_pixels", "rmse", "centroid"):
        assert node[f][0][:k].tobytes() == ex[f][pz["j"]][:k].tobytes(), f
    assert np.array_equal(node["labels"][0], ex["labels"][pz["j"]])
