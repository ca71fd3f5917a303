"""The surface of the Python binding against tests/golden/binding_surface.json, without a GPU: what every batch wrapper returns
for empty input (the ordered keys, and per key the type, dtype, shape and whether it is a view), the signature of every public
function and Graph method, and the package's public names.

The golden file was written by `python -m tests.binding_surface` at commit 1a7fdf6 ("Build the map kernels' cell index once;
share their call plumbing"), the last one in which the binding was the single module graph_slam_amd/__init__.py, before it was
split: it says what the binding did then, never what the tree does now.  A wrapper whose result changes on purpose gets its
entry rewritten by hand, in the commit that changes it."""
import json
import os

import pytest

import graph_slam_amd as G
from tests import binding_surface

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_surface.json")))


@pytest.fixture(scope="module")
def surface():
    return json.loads(json.dumps(binding_surface.record(G)))        # through JSON, as the golden file went


def test_the_recorder_covers_every_batch_wrapper():
    wrappers = ("preint_batch", "two_view_ba_batch", "plane_check_vro_batch", "imu_check_vro_batch", "vro_ransac_batch",
                "plane_extract_batch", "plane_propagate_batch", "plane_node_batch", "match_features_batch", "vro_adjust_batch",
                "map_fuse_batch", "map_clean", "map_normals", "map_render_batch")
    assert {k.split("(")[0] for k in GOLDEN["results"]} == set(wrappers)
    assert len(GOLDEN["public_names"]) == 108


@pytest.mark.parametrize("call", sorted(GOLDEN["results"]))
def test_results_are_what_they_were(surface, call):
    assert surface["results"][call] == GOLDEN["results"][call]


def test_signatures_are_what_they_were(surface):
    have = surface["signatures"]
    assert {k: have.get(k) for k in GOLDEN["signatures"]} == GOLDEN["signatures"]


def test_every_public_name_is_still_there(surface):
    assert set(GOLDEN["public_names"]) <= set(surface["public_names"])
    assert [n for n in GOLDEN["public_names"] if not hasattr(G, n)] == []
