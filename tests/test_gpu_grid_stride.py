"""Every kernel that strides beyond its capped grid, run past its grid at small shapes.

grid_for() (csrc/batch_call.hpp) caps a launch at 2^20 workgroups and 25 kernels of the mapping and place-recognition path stride
over what the grid does not cover.  At the default cap a second trip of such a loop needs hundreds of millions of items, so the
other tests run every one of these kernels with exactly one trip per workgroup.  fgo_debug_grid_cap lowers the cap: under caps 1, 2
and 3 an input of at least 5 workgroups' worth of items gives one workgroup 5 trips or more, then unequal trip counts (3 and 2),
then 2, 2 and 1.  Under each cap every output and every counter of a call must be (a) bit-identical to the same call under the
default cap and (b) equal to the entry point's numpy restatement exactly as its own GPU test compares them (the helpers of those
tests are reused), so that a fault common to both runs does not hide.  The launches_* functions below restate the launch sites as
(kernel, items, per_group); every test asserts from them that ceil(items / per_group) is at least 5 and exceeds the cap for each
launch it means to stride, and from the hook's return value that the cap is in force.  Before every capped call the same entry
point runs on other data of the same shapes (under_caps says why): without that, k_map_finalise with its stride doubled passed,
because the rows it skipped still held what the default-cap call had written to the same recycled allocation.

What the loops carry from one trip to the next, read from the kernels before anything ran (W = the workgroup):

  kernel               trip condition (uniform over W?)            barriers inside   carried over a trip            cleared by
  k_mc_quantise        p = blk*256+tid < n, += grid*256 (per lane) none              nothing                        -
  k_map_cells_gather   s likewise (per lane)                       none              nothing; wave_count counts the active lanes only
  k_mc_link            s likewise (per lane)                       none              nothing (union-find is global, lock-free)
  k_mc_flatten         base = blk*256 < n (uniform)                none; __ballot    todo, r: set from p every trip; p >= n gives
                                                                   loop is uniform   todo = false, so ragged and empty lanes only vote
                                                                   over the wave
  k_mc_roots           base likewise (uniform)                     none; shuffles    kept: set every trip; wave_count sits in a
                                                                   by every lane     divergent branch and counts its active lanes
  k_mc_label           base likewise (uniform)                     2, both reached   s_h (LDS), h             h = LLONG_MAX at the top; s_h rewritten
                                                                   by every thread                            after the trailing barrier
  k_mc_hist            p per lane; grid = min(grid, 1024)          none inside (the  s_bin (LDS) ON PURPOSE: flushed once after the loop
                                                                   two are outside)
  k_mc_mask/compact    p per lane                                  none              nothing
  k_mn_quantise        p per lane                                  none              nothing
  k_mn_search          s = blk*W+tid < n, += grid*W (per lane),    none              the lane's list D/I in dynamic LDS, cnt, wd, wi
                       W = 256, 128 or 64                                            cnt = 0, wd = LLONG_MAX, wi = ~0 at the top; only
                                                                                     entries below cnt are ever read
  k_map_init/pack      k per lane                                  none              nothing
  k_map_finalise       j per lane                                  none              nothing
  k_map_insert<AGG,FR> b = blk < n_tiles, += grid (uniform)        3, all outside    s_key/s_sum/s_cnt (LDS table), s_tot, n_oor
                                                                   the lane loops    all cleared at the top of a trip, behind the
                                                                                     trailing barrier of the one before; n_oor = 0
  k_render_tiles       b = blk < views*strips, += grid (uniform)   3 + the 2 of      s_z (strip z-buffer, then the reduction's words),
                                                                   mr_block_add      c[] -- s_z[0 .. npx) = EMPTY and c[] = 0 at the top
  k_render_init        k per lane                                  none              nothing
  k_render_points      b = blk < views*ceil(n/256) (uniform)       the 2 of          s_red, c[] -- c[] = 0 at the top; s_red rewritten
  k_render_resolve     b = blk < views*ceil(NP/256) (uniform)      mr_block_add      behind mr_block_add's trailing barrier
  k_place_norms        f per lane                                  none              nothing
  k_place_assign       fb = blk < ceil(F/256), += grid (uniform)   2 per centre      s_cen, s_nb: restaged per chunk behind the barrier at
                                                                   chunk, uniform    the chunk's top; d1/w1 reset at the top of a trip
  k_place_stats        k < span, span from gridDim.x (per lane;    none; shuffles    changed, inertia ON PURPOSE: one flush after the loop
                       whole waves loop alike: span % 256 == 0)    after the loop
  k_place_sums         i per lane                                  none              nothing
  k_place_hist         n = blk < n_frames, += grid (uniform)       4 + 16 in the     s_cnt, s_scan -- s_cnt[0 .. (V+1)/2) = 0 at the top,
                                                                   fixed-trip scan   s_scan rewritten, behind the trailing barrier
  k_place_weigh        n = blk*4+wave (uniform over the WAVE)      none; shuffles    acc = 0 at the top
                                                                   inside a wave
  k_place_score        a = blk < n_frames, += grid (uniform)       5, the wave loop  s_v (the table, then the merge lists), ms/mb/md
                                                                   between holds     s_v[0 .. V) = 0 and (ms, mb, md) = (-1, INT_MAX, 0)
                                                                   none              at the top, behind the trailing barrier

mr_block_add is called by every lane of the workgroup in all three render kernels (the callers' `if (i < n)` / `if (pix < NP)` close
before it), and its two barriers are unconditional.  No loop was found whose barrier a thread could miss.

Two kernels cannot be given a ragged last group: k_map_init and k_map_pack run over a power-of-two table.  k_place_stats takes 4096
features to a workgroup, so it has a training case of its own (20 557 features); k_place_norms over the CENTRES has V / 256 groups:
two in the query's vocabulary of 300 words, where it strides under cap 1 alone, and it is the same kernel as over the features.

k_mc_hist at its own cap (1024 workgroups, first striding past 262 144 points) runs with the hook untouched on 300 000 points; the
restatement takes about a second there, so the whole call -- the floor bin, its count and n_floor_removed among the rest -- is
compared with tests/map_clean_reference.py, not with a histogram of its own.
"""
import functools

import numpy as np
import pytest

import graph_slam_amd as G
from tests import map_clean_reference as mc
from tests import map_fuse_reference as mf
from tests import map_normals_reference as mn
from tests import map_render_reference as mr
from tests import place_reference as pl
from tests import test_gpu_map_clean as t_clean
from tests import test_gpu_map_fuse as t_fuse
from tests import test_gpu_map_normals as t_normals
from tests import test_gpu_map_render as t_render
from tests import test_gpu_place as t_place

pytestmark = pytest.mark.gpu

CAPS = (1, 2, 3)
DEFAULT_CAP = 1 << 20
MIN_GROUPS = 5


class grid_cap:
    """the cap in force for a block, proved by the hook's return value, and the default back afterwards"""

    def __init__(self, cap):
        self.cap = cap

    def __enter__(self):
        assert G.lib.fgo_debug_grid_cap(0) == DEFAULT_CAP
        assert G.lib.fgo_debug_grid_cap(self.cap) == self.cap

    def __exit__(self, *exc):
        assert G.lib.fgo_debug_grid_cap(0) == DEFAULT_CAP


def under_caps(run, scrub):
    """run() under the default cap, then under every cap of CAPS: yields (cap, outputs), every one bit-identical to the default's.
    A call stages its arrays in device allocations of its own, and the allocator hands it the blocks that the call before gave
    back: an item that a kernel skipped would find the right value there, left behind by the same call under the default cap.  So
    scrub() -- the same entry point with the same shapes on other data -- runs before every capped call and leaves other values."""
    assert G.lib.fgo_debug_grid_cap(0) == DEFAULT_CAP
    base = run()
    for cap in CAPS:
        scrub()
        with grid_cap(cap):
            got = run()
        same(got, base, cap)
        yield cap, got


def same(a, b, what=""):
    """two outputs of a wrapper are bit-identical: the arrays byte for byte, the numbers as their bytes"""
    assert list(a) == list(b), what
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)
        elif a[k] is None:
            assert b[k] is None, (what, k)
        else:
            assert type(a[k]) is type(b[k]) and np.array(a[k]).tobytes() == np.array(b[k]).tobytes(), (what, k, a[k], b[k])


def groups(items, per_group):
    return -(-items // per_group)


def strides(table, targets, ragged_exempt=()):
    """every targeted launch of the table has at least MIN_GROUPS workgroups' worth of items -- more than every cap -- and a ragged
    last group; returns the table as text"""
    names = {k for k, _, _ in table}
    assert set(targets) <= names, set(targets) - names
    for kernel, items, per in table:
        if kernel in targets:
            assert groups(items, per) >= MIN_GROUPS and all(groups(items, per) > cap for cap in CAPS), (kernel, items, per)
            assert per == 1 or items % per != 0 or kernel in ragged_exempt, (kernel, items, per)
    return ", ".join("%s %d/%d=%d" % (k, i, p, groups(i, p)) for k, i, p in table)


# ---- the launch sites, restated: (kernel, items, per_group) ------------------------------------------------------------------------
def launches_map_clean(n):
    names = ("k_mc_quantise", "k_map_cells_gather", "k_mc_link", "k_mc_flatten", "k_mc_roots", "k_mc_label", "k_mc_hist", "k_mc_mask",
             "k_mc_compact")
    return [(k, n, 256) for k in names]                          # k_mc_hist: min(grid, 1024) workgroups of the same grid


def normals_width(k):
    W = 256
    while W > 64 and k * W * 12 > 65536:
        W //= 2
    return W


def launches_map_normals(n, k):
    return [("k_mn_quantise", n, 256), ("k_map_cells_gather", n, 256), ("k_mn_search<%d>" % normals_width(k), n, normals_width(k))]


def launches_map_fuse(form, n_frames, ns, table_log2, n_voxels):
    fr = 128 if form == "frames" else 1
    px = 512 // fr
    slots = 1 << table_log2
    return [("k_map_init", 4 * slots, 2048), ("k_map_insert<%s>" % form, groups(n_frames, fr) * groups(ns, px), 1),
            ("k_map_pack", slots, 1024), ("k_map_finalise", n_voxels, 256)]


def launches_map_render(form, n_views, n_points, W, H, chunk=None):
    """of one launch round; in the global form the views go in chunks and the smallest chunk is listed"""
    if form == "tiles":
        return [("k_render_tiles", n_views * groups(H, max(1, 8192 // W)), 1)]
    v = n_views % chunk or chunk
    return [("k_render_init", v * W * H, 2048), ("k_render_points", v * groups(n_points, 256), 1), ("k_render_resolve", v * groups(W * H, 256), 1)]


def launches_vocab_train(F, V):
    return [("k_place_norms", F, 256), ("k_place_norms(centres)", V, 256), ("k_place_assign", F, 256), ("k_place_stats", F, 4096),
            ("k_place_sums", F * 128, 2048)]


def launches_place_query(F, V, N):
    return [("k_place_norms", F, 256), ("k_place_norms(centres)", V, 256), ("k_place_assign", F, 256), ("k_place_hist", N, 1),
            ("k_place_weigh", N, 4), ("k_place_score", N, 1)]


# ---- map_clean ------------------------------------------------------------------------------------------------------------------
CLEAN_P = dict(tolerance=0.03, min_cluster_size=40, remove_floor=1, floor_res=0.05, floor_span=1.0, floor_clearance=0.04)
LATE = 3 * 256                                                   # from here on a point is in a later trip under every cap of CAPS


@functools.lru_cache(maxsize=None)
def clean_cloud(up_sign):
    """1 229 points = 4 x 256 + 205: a floor sheet with a column standing on it (one cluster, part of it floor), a blob in the air
    (kept), a small blob and loners (dropped by min_cluster_size) and points out of range, in shuffled order so that every cluster
    spans the 256-point groups; the lowest kept point sits in the last group"""
    rng = np.random.default_rng(2031)
    gx, gy = np.meshgrid(np.arange(26), np.arange(20), indexing="ij")
    sheet = np.stack([0.02 * gx.reshape(-1), 0.02 * gy.reshape(-1), rng.uniform(0.0, 0.006, gx.size)], 1)              # 520
    column = rng.uniform([0.20, 0.16, 0.0], [0.28, 0.24, 0.5], (380, 3))
    blob = rng.uniform([1.0, 1.0, 0.7], [1.08, 1.08, 0.78], (260, 3))
    small = rng.uniform([-1.0, 0.5, 0.3], [-0.99, 0.51, 0.31], (25, 3))
    loners = np.stack([3.0 + 0.2 * np.arange(35), np.full(35, -2.0), rng.uniform(0.0, 1.0, 35)], 1)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1e30, 0, 0], [0, 0, -np.inf], [0, -1e300, 0], [40000.0, 0, 0], [0, 0, np.nan],
                    [np.inf, np.inf, 0], [0, 33000.0, 0]])
    x = np.concatenate([sheet, column, blob, small, loners, bad])
    x = x[rng.permutation(len(x))]
    lowest = np.array([0.24, 0.20, -0.004])                      # inside the sheet's reach, below all of it
    x[1100] = lowest
    assert len(x) == 1229
    x[:, 2] *= up_sign
    x.setflags(write=False)
    P = dict(CLEAN_P, up_sign=up_sign)
    return x, P, mc.clean(x, **P)


@pytest.mark.parametrize("up_sign", [1, -1])
def test_map_clean_past_its_grid(up_sign):
    x, P, want = clean_cloud(up_sign)
    n = len(x)
    print(strides(launches_map_clean(n), [k for k, _, _ in launches_map_clean(n)]))
    # what the case is for, read off the restatement
    stage = want["reason"] != 1
    stage &= want["reason"] != 2
    h = up_sign * np.rint(x[:, 2] * 2.0 ** 20)
    assert int(np.nanargmin(np.where(stage, h, np.inf))) == 1100 >= LATE                  # the smallest height: a later trip
    floor_pts = np.nonzero(want["reason"] == 3)[0]
    assert want["floor_bin_points"] > 100 and len(np.unique(floor_pts // 256)) == 5       # the floor is filled from every group
    assert want["n_out_of_range"] == 9 and (np.nonzero(want["reason"] == 1)[0] // 256 >= 1).any()
    assert want["n_clusters_kept"] == 2 and want["n_clusters"] - want["n_clusters_kept"] >= 30 and (want["reason"] == 2).sum() >= 60
    for c in np.nonzero(want["cluster_size"] >= 40)[0]:
        assert len(np.unique(np.nonzero(want["label"] == c)[0] // 256)) == 5              # a kept cluster spans every group
    assert 0 < want["n_floor_removed"] < want["n_after_clusters"] and want["n_kept"] > 300
    other = (x[::-1] * [1.0, -1.0, 1.0] + [0.3, 0.1, 0.0])                                  # the same heights in another order elsewhere
    for cap, got in under_caps(lambda: G.map_clean(x, params=G.map_clean_params(**P)), lambda: G.map_clean(other, params=G.map_clean_params(**P))):
        t_clean._equal(got, want)


def test_map_clean_histogram_at_its_own_cap():
    """300 000 points: ceil(n / 256) = 1172 workgroups' worth for the 1024 of k_mc_hist, the hook untouched.  A rough floor sheet and
    three columns on it; the restatement takes about a second at this size, so the whole call is compared with it"""
    assert G.lib.fgo_debug_grid_cap(0) == DEFAULT_CAP
    n = 300000
    assert groups(n, 256) > 1024
    rng = np.random.default_rng(2032)
    P = dict(tolerance=0.03, min_cluster_size=200, floor_res=0.1, floor_span=2.0, floor_clearance=0.1)
    gx, gy = np.meshgrid(np.arange(500), np.arange(480), indexing="ij")
    sheet = np.stack([0.02 * gx.reshape(-1), 0.02 * gy.reshape(-1), rng.uniform(-0.03, 0.03, gx.size)], 1)            # 240 000
    b = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(50), indexing="ij"), -1).reshape(-1, 3) * 0.02      # 20 000 each
    blobs = [b + [2.0 + 2.0 * k, 3.0, 0.0] + rng.uniform(-0.002, 0.002, b.shape) for k in range(3)]
    x = np.concatenate([sheet] + blobs)
    x = x[rng.permutation(len(x))]
    assert len(x) == n
    want = mc.clean(x, **P)
    got = G.map_clean(x, params=G.map_clean_params(**P))
    assert (got["floor_bin"], got["floor_bin_points"], got["n_floor_removed"]) == (want["floor_bin"], want["floor_bin_points"], want["n_floor_removed"])
    t_clean._equal(got, want)
    assert want["floor_bin_points"] > 100000 and want["n_floor_removed"] > want["floor_bin_points"] and want["n_kept"] > 30000


# ---- map_normals ----------------------------------------------------------------------------------------------------------------
NORMALS_CASES = {256: dict(k=21, n=1229), 128: dict(k=42, n=1229), 64: dict(k=43, n=350, max_radius=0.32)}


@functools.lru_cache(maxsize=None)
def normals_cloud(W):
    """the first points of the corner cloud, with loners far above and below it (the last and the first cells in key order: few
    neighbours, in the first and in the last trip of the search) and points out of range"""
    c = dict(NORMALS_CASES[W])
    n = c.pop("n")
    loners = np.array([[0.0, 0.0, 9.0], [0.05, 0.0, 9.0], [0.0, 0.0, -9.0], [0.3, 0.3, 9.5], [0.1, -0.2, 8.0], [0.12, -0.2, 8.0], [0.1, -0.18, 8.0],
                       [0.11, -0.21, 8.02]])
    bad = np.array([[np.nan, 0, 1], [0, np.inf, 1], [1e30, 0, 1], [0, 0, -1e300], [float(1 << 14), 0, 1]])
    x = np.concatenate([mn.corner()[:n - len(loners) - len(bad)], loners, bad])
    x = x[np.random.default_rng(2033).permutation(n)]
    x.setflags(write=False)
    return x, c, mn.normals(x, **c)


@pytest.mark.parametrize("W", [256, 128, 64])
def test_map_normals_past_its_grid(W):
    x, P, want = normals_cloud(W)
    n, k = len(x), P["k"]
    assert normals_width(k) == W and [normals_width(v) for v in (21, 22, 42, 43, 64)] == [256, 128, 128, 64, 64]
    table = launches_map_normals(n, k)
    print(strides(table, ["k_mn_search<%d>" % W] + (["k_mn_quantise", "k_map_cells_gather"] if groups(n, 256) >= MIN_GROUPS else [])))
    # the search runs in sorted order: the rank of every point among the cell keys
    ok = want["status"] != 1
    cell = want["Q"] // mn.quanta(dict(mn.DEFAULTS, **P)["cell"])
    key = np.where(ok, mf.make_key(cell[:, 0], cell[:, 1], cell[:, 2]), np.iinfo(np.int64).max)
    rank = np.empty(n, np.int64)
    rank[np.argsort(key, kind="stable")] = np.arange(n)
    short = ok & (want["n_neighbours"] < k)
    full = ok & (want["n_neighbours"] == k)
    late = rank >= 3 * W
    assert (short & late).any() and (full & late).any() and (short & ~late).any() and full.sum() > n // 2
    assert want["n_few"] >= 2 and want["n_out_of_range"] == 5
    # a short list right behind a full one of the same lane: the thread's previous point is W ranks back
    by_rank = np.argsort(rank)
    prev_full = np.zeros(n, bool)
    prev_full[by_rank[W:]] = full[by_rank[:-W]]
    assert (short & prev_full).any()
    other = x[::-1] * [-1.0, 1.0, 1.0] + [0.0, 0.5, -0.25]
    for cap, got in under_caps(lambda: t_normals._run(x, P), lambda: t_normals._run(other, P)):
        t_normals._ints_equal(got, want)
        t_normals._floats_hold(got, want, P)


# ---- map_fuse_batch -------------------------------------------------------------------------------------------------------------
FUSE_CFG = dict(name="grid_stride", n=7, W=44, H=36, channels=3, params=dict(skip=1, rect=(3, 2, 41, 35), leaf=0.05, table_log2=13))
FUSE_FAR = 5                                                     # the frame whose pose puts every point out of range


@functools.lru_cache(maxsize=None)
def fuse_case():
    """7 frames of 38 x 33 sampled pixels that look into the same corner (the same voxels from every frame), colour, a table of 2^13
    slots; frame 5 stands 10^9 m away: every valid point of its tiles is out of range"""
    c = mf.make_case(FUSE_CFG)
    c["pose_w"][FUSE_FAR, 0] = 1e9
    c["want"] = mf.fuse(c["depth"], c["pose_w"], c["color"], c["extrinsic"], **c["params"])
    return c


@pytest.mark.parametrize("form", ["plain", "lds", "frames"])
def test_map_fuse_past_its_grid(form):
    c = fuse_case()
    w = c["want"]
    n, ns = FUSE_CFG["n"], 38 * 33
    assert w["n_sampled"] == n * ns and n % 128 != 0
    table = launches_map_fuse(form, n, ns, 13, w["n_voxels"])
    print(strides(table, [k for k, _, _ in table], ragged_exempt=("k_map_init", "k_map_pack")))
    if form != "frames":
        assert ns % 512 != 0 and FUSE_FAR * groups(ns, 512) >= 3 * 3                      # the far frame's tiles: later trips
    else:
        assert ns % 4 != 0
    assert w["status"] == mf.MAP_OK and w["n_out_of_range"] > 1000 and w["frame_points"][FUSE_FAR] == 0
    assert (w["count"] >= 5).sum() > 500 and w["n_voxels"] + w["n_dropped"] < (1 << 13) * 3 // 4      # shared voxels; the table has room
    with t_render._env(FGO_MAP_INSERT=form):
        other = dict(c, depth=c["depth"][::-1].copy(), pose_w=c["pose_w"][::-1] + [0.31, -0.27, 0.13, 0, 0, 0, 0], color=255 - c["color"])
        for cap, got in under_caps(lambda: t_fuse._run(c), lambda: t_fuse._run(other)):
            t_fuse._equal(got, w)


# ---- map_render_batch -----------------------------------------------------------------------------------------------------------
RENDER_W, RENDER_H, RENDER_N, RENDER_V = 176, 144, 1333, 3


@functools.lru_cache(maxsize=None)
def render_case():
    """3 views of 176 x 144 (4 strips each) over 1 333 points = 5 x 256 + 53; every view is turned another way, so that it draws
    other points on other pixels; non-finite points in the last tile of points; measured depth for the five depth counters"""
    rng = np.random.default_rng(2034)
    W, H, n = RENDER_W, RENDER_H, RENDER_N
    P = dict(fx=160.0, fy=160.0, cx=0.5 * (W - 1), cy=0.5 * (H - 1), splat=1, agree_tol=0.4, z_min=1.5, z_max=5.5)
    x = mr.random_cloud(n, W, H, P, rng, margin=40.0)
    x[[1290, 1301, 1332]] = [[np.nan, 0, 1], [0, np.inf, 2], [1.0, 1.0, -np.inf]]
    color = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    poses = np.stack([np.concatenate([[0.01, -0.02, 0.03], mf.quat_axis(2, 0.05)]), np.concatenate([[0.3, 0.0, -0.2], mf.quat_axis(1, 0.12)]),
                      np.concatenate([[-0.2, 0.1, 0.4], mf.quat_axis(0, -0.1)])])
    depth = rng.integers(0, 8000, (RENDER_V, H, W)).astype(np.uint16)
    c = dict(xyz=x, pose_w=poses, color=color, width=W, height=H, depth=depth, **P)
    c["want"] = mr.render(**c)
    return c


def render_other():
    """the render case with the views turned elsewhere, other colours and other measured depth: the same shapes"""
    c = render_case()
    return dict(c, pose_w=c["pose_w"][::-1] + [0.4, -0.3, 0.2, 0, 0, 0, 0], color=255 - c["color"], depth=c["depth"][::-1, ::-1].copy())


def render_zwords(chunk):
    return str(chunk * RENDER_W * RENDER_H + 100)


def check_render_case():
    w = render_case()["want"]
    for f in mr.VIEW_FIELDS:
        assert (w[f] > 0).all() and len(set(w[f].tolist())) == RENDER_V, f                # a count carried over would show
    assert w["n_nonfinite"] == 3
    for a in range(RENDER_V):
        for b in range(a):
            assert (w["index"][a] != w["index"][b]).mean() > 0.2                         # the views draw different points
    return w


@pytest.mark.parametrize("form", ["tiles", "global"])
def test_map_render_past_its_grid(form):
    c = render_case()
    w = mr.with_form(check_render_case(), {"tiles": mr.TILES, "global": mr.GLOBAL}[form], RENDER_W)
    table = launches_map_render(form, RENDER_V, RENDER_N, RENDER_W, RENDER_H, chunk=2)
    print(strides(table, [k for k, _, _ in table]))
    assert form == "global" or groups(RENDER_H, 8192 // RENDER_W) >= 2                    # strips per view
    env = dict(FGO_MAP_RENDER=form)
    if form == "global":
        env["FGO_MAP_RENDER_ZWORDS"] = render_zwords(2)                                   # chunks of 2 views and of 1
    with t_render._env(**env):
        for cap, got in under_caps(lambda: t_render._run(c), lambda: t_render._run(render_other())):
            t_render._equal(got, w)
            assert got["form"] == w["form"]


@pytest.mark.parametrize("form", ["tiles", "global"])
def test_a_view_does_not_move_between_trips(form):
    """view i of the batch under cap 1 -- every tile of every view in one workgroup's trips -- equals view i rendered alone under the
    default cap"""
    c = render_case()
    env = dict(FGO_MAP_RENDER=form)
    if form == "global":
        env["FGO_MAP_RENDER_ZWORDS"] = render_zwords(3)                                   # all views in one chunk
    with t_render._env(**env):
        t_render._run(render_other())                                                      # see under_caps
        with grid_cap(1):
            batch = t_render._run(c)
        assert G.lib.fgo_debug_grid_cap(0) == DEFAULT_CAP
        for v in range(RENDER_V):
            one = t_render._run(dict(c, pose_w=c["pose_w"][v:v + 1], depth=c["depth"][v:v + 1]))
            for f in t_render.ARRAYS + ("rt",) + mr.VIEW_FIELDS:
                assert one[f][0].tobytes() == batch[f][v].tobytes(), (v, f)
            assert one["n_nonfinite"] == batch["n_nonfinite"]


# ---- vocab_train ----------------------------------------------------------------------------------------------------------------
TRAIN_CASES = {"chunks": dict(F=1233, V=150, n_iters=3), "small": dict(F=1233, V=7, n_iters=3), "stats": dict(F=20557, V=7, n_iters=2)}
TRAIN_TARGETS = {"chunks": ("k_place_norms", "k_place_assign", "k_place_sums"), "small": ("k_place_norms", "k_place_assign", "k_place_sums"),
                 "stats": ("k_place_norms", "k_place_assign", "k_place_sums", "k_place_stats")}


@functools.lru_cache(maxsize=None)
def train_case(name):
    c = TRAIN_CASES[name]
    desc = t_place.clustered(2035, c["F"], 200, noise=40)          # does not converge in n_iters
    return desc, pl.train(desc, n_words=c["V"], n_iters=c["n_iters"])


@pytest.mark.parametrize("name", list(TRAIN_CASES))
def test_vocab_train_past_its_grid(name):
    c = TRAIN_CASES[name]
    desc, want = train_case(name)
    print(strides(launches_vocab_train(c["F"], c["V"]), TRAIN_TARGETS[name]))
    assert (name == "chunks") == (c["V"] > 128)                                          # PL_TC = 128: two centre chunks, or one
    assert want["iterations"] == c["n_iters"] >= 2 and 0 < want["changed_last"] < c["F"]      # k_place_stats has seen prev != NULL
    opts = G.vocab_options(n_words=c["V"], n_iters=c["n_iters"])
    for cap, got in under_caps(lambda: G.vocab_train(desc, opts), lambda: G.vocab_train(255 - desc[::-1], opts)):
        assert np.array_equal(got["centres"], want["centres"]) and np.array_equal(got["count"], want["count"])
        assert got["count"].dtype == np.int64 and got["count"].sum() == c["F"]
        for k in t_place.TRAIN_KEYS:
            assert got[k] == want[k], (cap, k, got[k], want[k])


# ---- place_query_batch ----------------------------------------------------------------------------------------------------------
QUERY_SIZES = (150, 0, 257, 64, 300, 1, 200, 130, 90, 65, 77, 2, 40, 63, 120, 10, 33, 85)       # 18 frames, 1 687 features
QUERY_V, QUERY_GAP = 300, 3


@functools.lru_cache(maxsize=None)
def query_scene():
    """18 frames over one world of 300 landmarks, frame f at place f % 5: a revisit is 5 frames back, behind min_gap = 3"""
    rng = np.random.default_rng(2036)
    world = rng.integers(0, 256, (300, 128))
    frames = []
    for f, n in enumerate(QUERY_SIZES):
        ids = (40 * (f % 5) + rng.permutation(max(120, n))[:n]) % 300
        frames.append(np.clip(world[ids] + rng.integers(-8, 9, (n, 128)), 0, 255).astype(np.uint8))
    fp = np.concatenate([[0], np.cumsum(QUERY_SIZES)]).astype(np.int64)
    desc = np.concatenate(frames)
    centres = pl.train(desc, n_words=QUERY_V, n_iters=2)["centres"]
    return fp, desc, centres


def run_query(frames=None, weights=None, other=False, **kw):
    fp, desc, centres = query_scene()
    if other:                                                    # the same shapes on other data: see under_caps
        desc, centres = 255 - desc[::-1], centres[::-1]
    if frames is not None:
        desc = np.concatenate([desc[fp[f]:fp[f + 1]] for f in frames] + [np.zeros((0, 128), np.uint8)])
        fp = np.concatenate([[0], np.cumsum([fp[f + 1] - fp[f] for f in frames])]).astype(np.int64)
    return G.place_query_batch(fp, desc, centres, weights=weights, options=G.place_options(**kw), want_words=True, want_dot=True)


@pytest.mark.parametrize("top_k", [2, 64])
def test_place_query_past_its_grid(top_k):
    fp, desc, centres = query_scene()
    N, F = len(QUERY_SIZES), int(fp[-1])
    print(strides(launches_place_query(F, QUERY_V, N), ("k_place_norms", "k_place_assign", "k_place_hist", "k_place_weigh", "k_place_score")))
    assert 0 in QUERY_SIZES and len(set(QUERY_SIZES)) == N and QUERY_V > 128 and top_k in (2, 64) and 2 < N - QUERY_GAP < 64
    for cap, got in under_caps(lambda: run_query(top_k=top_k, min_gap=QUERY_GAP), lambda: run_query(other=True, top_k=top_k, min_gap=QUERY_GAP)):
        want = pl.query(fp, desc, centres, weights=got["weights"], top_k=top_k, min_gap=QUERY_GAP)      # the table the device used
        t_place.assert_equal(got, want, "cap %d" % cap)
        assert np.abs(got["weights"].astype(np.int64) - pl.default_weights(got["df"], N)).max() <= 1
        assert (got["n_cand"][:QUERY_GAP] == 0).all() and (got["dot_matrix"][:QUERY_GAP] == -1).all()      # an empty database
        assert got["n_cand"].max() == (2 if top_k == 2 else got["n_cand"].max()) and got["n_cand"].max() >= 2
        assert got["n_cand"][QUERY_SIZES.index(0)] == 0


def test_a_frame_does_not_move_between_trips():
    """frame i of the batch under cap 1 -- all frames in one workgroup's trips -- against the default cap: its words, distances and
    norm equal those of the frame queried alone, and its candidates, scores and dots those of the batch cut off behind it (with
    given weights a frame's row depends on the frames up to it and on nothing else)"""
    fp = query_scene()[0]
    N = len(QUERY_SIZES)
    q = (np.random.default_rng(2037).integers(1, 300, QUERY_V)).astype(np.int32)
    run_query(weights=q[::-1], other=True, top_k=4, min_gap=QUERY_GAP)
    with grid_cap(1):
        batch = run_query(weights=q, top_k=4, min_gap=QUERY_GAP)
    assert G.lib.fgo_debug_grid_cap(0) == DEFAULT_CAP
    assert batch["n_cand"].max() == 4
    for i in range(N):
        one = run_query(frames=[i], weights=q, top_k=4, min_gap=QUERY_GAP)
        assert one["norm2"][0] == batch["norm2"][i], i
        for key in ("word", "word_d"):
            assert np.array_equal(one[key], batch[key][fp[i]:fp[i + 1]]), (i, key)
    for i in (QUERY_GAP, 7, N - 1):
        head = run_query(frames=list(range(i + 1)), weights=q, top_k=4, min_gap=QUERY_GAP)
        for key in ("n_cand", "cand_frame", "cand_dot", "cand_score", "norm2"):
            assert head[key][i].tobytes() == batch[key][i].tobytes(), (i, key)
        assert np.array_equal(head["dot_matrix"][i], batch["dot_matrix"][i, :i + 1])
