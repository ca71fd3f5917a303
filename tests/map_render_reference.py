"""Numpy restatement of fgo_map_render_batch (include/fgo.h), written from the stated semantics and not from the kernels: every
product, quotient and sum is a numpy ufunc of its own (numpy has no fused multiply-add), np.rint for the quantum, and the z-buffer is
np.minimum.at on a flat uint64 image, per view and per offset of the footprint.  PCL and VTK are not in the reference tree, so this
file IS the yardstick of csrc/kernels_map_render.hip; tests/test_map_render_reference_cpu.py holds it to a brute force on the CPU.

render() returns the outputs of the call.  The case makers build the calls of tests/test_gpu_map_render.py; CASES lists them and
case(name) makes (and keeps) one of them with its expected outputs."""
import functools

import numpy as np

from tests import map_fuse_reference as mf

QBITS = 20                    # the quantum is 2^-20 m
TWO20 = float(1 << QBITS)
STRIP = 8192                  # pixels of a strip of the tiles form
TILES, GLOBAL = 0, 1
DEFAULT_FORM = TILES          # the form the library runs without FGO_MAP_RENDER
DEFAULTS = dict(fx=250.5773, fy=250.5773, cx=90.0, cy=70.0, z_scale=0.001, z_min=0.1, z_max=50.0, splat=0, radius=0.0, max_half=8,
                agree_tol=0.05, background=(0, 0, 26))
VIEW_FIELDS = ("n_valid", "n_drawn", "n_pixels", "n_meas", "n_both", "n_agree", "n_closer", "n_through")
RESULT_FIELDS = ("n_points", "n_nonfinite", "form", "tile_rows")
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def view_rt(pose7, extrinsic7=None, offset7=None):
    """the 12 doubles of rt_out: the fusion's pose_rt, then the offset composed on the right, every operation on its own"""
    rt1 = mf.pose_rt(pose7, extrinsic7)
    if offset7 is None:
        return rt1
    o = np.asarray(offset7, np.float64)
    R1, t1, Ro, to = rt1[:9].reshape(3, 3), rt1[9:], mf.quat_matrix(o[3:]), o[:3]
    R = np.empty((3, 3)); t = np.empty(3)
    for i in range(3):
        for j in range(3):
            R[i, j] = (R1[i, 0] * Ro[0, j] + R1[i, 1] * Ro[1, j]) + R1[i, 2] * Ro[2, j]
        t[i] = ((R1[i, 0] * to[0] + R1[i, 1] * to[1]) + R1[i, 2] * to[2]) + t1[i]
    return np.concatenate([R.reshape(-1), t])


def form_fields(form, W):
    """(form, tile_rows) of the result: an image wider than a strip runs in the global form"""
    if form == TILES and W <= STRIP:
        return TILES, max(1, STRIP // W)
    return GLOBAL, 0


def project(x, finite, rt, P, W, H):
    """one view: valid, drawn (masks over the points), zq, and the clipped-to-nothing-yet footprint: u0, v0, h (int64)"""
    R, t = rt[:9].reshape(3, 3), rt[9:]
    n = len(x)
    with np.errstate(all="ignore"):
        d = [x[:, k] - t[k] for k in range(3)]
        p = [(R[0, k] * d[0] + R[1, k] * d[1]) + R[2, k] * d[2] for k in range(3)]
        z = p[2]
        valid = finite & (z > P["z_min"]) & (z < P["z_max"])
        zs = np.where(valid, z, 1.0)
        zq = np.rint(zs * TWO20).astype(np.int64)
        uf = ((P["fx"] * p[0]) / zs) + P["cx"]
        vf = ((P["fy"] * p[1]) / zs) + P["cy"]
        B = 2.0 ** 30
        inside = valid & (uf > -B) & (uf < B) & (vf > -B) & (vf < B)
        u0 = np.floor(np.where(inside, uf, 0.0) + 0.5).astype(np.int64)
        v0 = np.floor(np.where(inside, vf, 0.0) + 0.5).astype(np.int64)
        s = np.zeros(n, np.int64)
        if P["radius"] > 0:
            s = np.minimum(np.floor((P["fx"] * P["radius"]) / zs), float(P["max_half"])).astype(np.int64)
    h = np.minimum(P["max_half"], P["splat"] + s)
    drawn = inside & (u0 + h >= 0) & (u0 - h <= W - 1) & (v0 + h >= 0) & (v0 - h <= H - 1)
    return valid, drawn, zq, u0, v0, h


def render(xyz, pose_w, color=None, extrinsic=None, view_offset=None, width=176, height=144, depth=None, form=None, **params):
    P = dict(DEFAULTS, **params)
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    n, W, H = len(x), width, height
    pose_w = np.asarray(pose_w, np.float64).reshape(-1, 7)
    V = len(pose_w)
    ch = 0 if color is None else (1 if color.ndim == 1 else color.shape[1])
    col = None if color is None else np.asarray(color, np.uint8).reshape(n, ch)
    finite = np.all(np.isfinite(x), 1)
    rt = np.stack([view_rt(pose_w[v], extrinsic, view_offset) for v in range(V)]) if V else np.zeros((0, 12))
    tq = int(np.rint(P["agree_tol"] * TWO20))
    index_all = np.arange(n, dtype=np.uint64)
    zq_out = np.full((V, H, W), -1, np.int32); index_out = np.full((V, H, W), -1, np.int32)
    color_out = None if not ch else np.empty((V, H, W, ch), np.uint8)
    counts = {f: np.zeros(V, np.int64) for f in VIEW_FIELDS}
    for v in range(V):
        valid, drawn, zq, u0, v0, h = project(x, finite, rt[v], P, W, H)
        img = np.full(H * W, EMPTY, np.uint64)
        word = (zq.astype(np.uint64) << np.uint64(32)) | index_all
        hmax = int(h[drawn].max()) if drawn.any() else -1
        for dv in range(-hmax, hmax + 1):
            for du in range(-hmax, hmax + 1):
                uu, vv = u0 + du, v0 + dv
                m = drawn & (h >= abs(du)) & (h >= abs(dv)) & (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
                np.minimum.at(img, (vv[m] * W + uu[m]), word[m])
        covered = img != EMPTY
        wz = (img >> np.uint64(32)).astype(np.int64); wi = (img & np.uint64(0xFFFFFFFF)).astype(np.int64)
        zq_out[v] = np.where(covered, wz, -1).reshape(H, W)
        index_out[v] = np.where(covered, wi, -1).reshape(H, W)
        if ch:
            c = np.tile(np.asarray(P["background"], np.uint8)[:ch], (H * W, 1))
            c[covered] = col[wi[covered]]
            color_out[v] = c.reshape(H, W, ch)
        counts["n_valid"][v] = valid.sum(); counts["n_drawn"][v] = drawn.sum(); counts["n_pixels"][v] = covered.sum()
        if depth is not None:
            zm = depth[v].reshape(-1).astype(np.float64) * P["z_scale"]
            meas = (zm > P["z_min"]) & (zm < P["z_max"])
            mq = np.rint(zm * TWO20).astype(np.int64)
            both = meas & covered
            dq = (mq - wz)[both]
            counts["n_meas"][v] = meas.sum(); counts["n_both"][v] = both.sum()
            counts["n_agree"][v] = np.sum(np.abs(dq) <= tq); counts["n_closer"][v] = np.sum(dq < -tq); counts["n_through"][v] = np.sum(dq > tq)
    out = dict(counts, zq=zq_out, index=index_out, color=color_out if (color is None or color.ndim == 2) else color_out[..., 0], rt=rt)
    if V == 0:
        out.update(n_points=0, n_nonfinite=0, form=0, tile_rows=0)
    else:
        f, rows = form_fields(DEFAULT_FORM if form is None else form, W)
        out.update(n_points=n, n_nonfinite=int(np.sum(~finite)), form=f, tile_rows=rows)
    return out


# ---- the cases: dicts of render()'s arguments

def cam_point(u, v, z, P):
    """the point of the camera frame (identity pose) whose uf, vf are (nearly) u, v at depth z"""
    return [(u - P["cx"]) * z / P["fx"], (v - P["cy"]) * z / P["fy"], z]


def tiny():
    """8 x 6, one view at the identity, fx = fy = 4, cx = 3.5, cy = 2.5: p = (a z / 4, b z / 4, z) lands on uf = a + 3.5, vf = b + 2.5
    exactly when a, b and z are small dyadic numbers -- every row can be checked by hand"""
    P = dict(fx=4.0, fy=4.0, cx=3.5, cy=2.5, z_min=0.5, z_max=4.0)
    x = np.array([
        [0.0, 0.0, 1.0],                 # uf = 3.5, vf = 2.5: uf + 0.5 = 4 exactly -> pixel (4, 3)
        [-0.75, -0.5, 2.0],              # uf = 2.0, vf = 1.5 -> (2, 2)
        [-0.75, -0.5, 1.0],              # uf = 0.5, vf = 0.5 -> (1, 1)
        [0.0, 0.0, 0.5],                 # z == z_min: excluded
        [0.0, 0.0, 4.0],                 # z == z_max: excluded
        [0.0, 0.0, -1.0],                # behind the camera
        [-1.0 - 2.0 ** -40, 0.0, 1.0],   # uf just below -0.5 -> u0 = -1: off the left edge
        [1.0, 0.0, 1.0],                 # uf = 7.5 -> u0 = 8: off the right edge
        [0.0, -0.75 - 2.0 ** -40, 1.0],  # vf just below -0.5 -> v0 = -1: off the top
        [0.0, 0.75, 1.0],                # vf = 5.5 -> v0 = 6: off the bottom
        [np.nan, 0.0, 1.0],              # non-finite
        [0.0, np.inf, 1.0],              # non-finite
        [0.875, 0.625, 1.0],             # uf = 7.0, vf = 5.0 -> the last pixel (7, 5)
        [-0.875, -0.625, 1.0],           # uf = 0.0, vf = 0.0 -> the first pixel (0, 0)
        [0.0, 0.0, 3.0],                 # behind the first row's point on pixel (4, 3): loses
    ])
    color = (np.arange(len(x) * 3).reshape(-1, 3) * 5 % 256).astype(np.uint8)
    return dict(xyz=x, pose_w=IDENT[None], color=color, width=8, height=6, **P)


def ties():
    """two points with equal zq on one pixel (z differs by less than a quantum), exact duplicates, and a unique winner elsewhere"""
    P = dict(fx=4.0, fy=4.0, cx=3.5, cy=2.5, z_min=0.5, z_max=4.0)
    x = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 1.0 + 2.0 ** -23], [0.0, 0.0, 1.0], [0.25, 0.0, 1.0], [0.25, 0.0, 1.0], [0.25, 0.0, 1.0],
                  [-0.5, 0.25, 1.5], [-0.5, 0.25, 1.25]])
    color = np.arange(10, 10 + len(x), dtype=np.uint8)
    return dict(xyz=x, pose_w=IDENT[None], color=color, width=8, height=6, **P)


def footprints(radius=0.0):
    """splat = 2 at the four corners and the four edges of 20 x 14, a centre off-image whose footprint reaches in, one far off; with
    a radius: a near point that hits max_half and a far point with s = 0"""
    P = dict(fx=8.0, fy=8.0, cx=9.5, cy=6.5, z_min=0.25, z_max=64.0, splat=2, max_half=5, radius=radius)
    uv = [(0, 0), (19, 0), (0, 13), (19, 13), (10, 0), (10, 13), (0, 7), (19, 7), (-2, 5), (21, 15), (-3, 7), (10, 16), (25, 25), (10, 7)]
    z = [1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 1.25, 1.75, 2.25, 2.75, 1.0, 40.0]
    x = [cam_point(u, v, zz, P) for (u, v), zz in zip(uv, z)]
    if radius > 0:
        x += [cam_point(4, 4, 0.3, P), cam_point(15, 9, 60.0, P)]         # s = floor(8 r / 0.3) > max_half; s = floor(8 r / 60) = 0
    return dict(xyz=np.array(x), pose_w=IDENT[None], color=None, width=20, height=14, **P)


def random_cloud(n, W, H, P, rng, z_lo=1.0, z_hi=6.0, margin=6.0):
    """n points of the camera frame whose centres fall on the image and a margin round it"""
    u = rng.uniform(-margin, W + margin, n); v = rng.uniform(-margin, H + margin, n); z = rng.uniform(z_lo, z_hi, n)
    return np.stack([(u - P["cx"]) * z / P["fx"], (v - P["cy"]) * z / P["fy"], z], 1)


def strips(W, H, n=3000, splat=1, seed=5, channels=3, **kw):
    """an image of W x H covered by a random cloud: with splat >= 1 footprints straddle every strip boundary of the tiles form"""
    rng = np.random.default_rng(seed + 7 * W + H)
    P = dict(fx=0.9 * max(W, H), fy=0.9 * max(W, H), cx=0.5 * (W - 1), cy=0.5 * (H - 1), splat=splat, **kw)
    x = random_cloud(n, W, H, P, rng, margin=3.0)
    if channels == 0:
        color = None
    else:
        color = rng.integers(0, 256, (n, 3) if channels == 3 else n).astype(np.uint8)
    pose = np.concatenate([[0.01, -0.02, 0.03], mf.quat_axis(2, 0.05)])
    return dict(xyz=x, pose_w=pose[None], color=color, width=W, height=H, **P)


CHASE_EYE, CHASE_TARGET, CHASE_UP = (0.0, -2.0, -5.0), (0.0, 0.0, 5.0), (0.0, -0.98, 0.199)


def chase_offset():
    """look_at(CHASE_*) of the package, restated: the test of look_at compares the two"""
    e, t, up = (np.array(v) for v in (CHASE_EYE, CHASE_TARGET, CHASE_UP))
    z = (t - e) / np.linalg.norm(t - e)
    x = np.cross(-up, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 1)
    w = 0.5 * np.sqrt(1.0 + np.trace(R))
    q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    return np.concatenate([e, q / np.linalg.norm(q)])


def many_views(channels, V=300, n=2000, W=44, H=36, offset=True):
    """V poses on a sweep round a cloud of n points, with the quarter-turn extrinsic of the fusion's tests and the chase camera"""
    rng = np.random.default_rng(91 + channels)
    x = rng.uniform(-1.5, 1.5, (n, 3)) + np.array([0.0, 0.0, 6.0])
    x[::97] = np.nan
    poses = np.zeros((V, 7))
    for v in range(V):
        a = -0.4 + 0.8 * v / max(V - 1, 1)
        poses[v] = np.concatenate([[2.0 * a, 0.1 * np.sin(9 * a), 0.5 * a * a], mf.quat_mul(mf.quat_axis(1, -0.3 * a), mf.quat_axis(0, 0.05 * np.cos(7 * a)))])
    color = None if channels == 0 else rng.integers(0, 256, (n, 3) if channels == 3 else n).astype(np.uint8)
    P = dict(fx=40.0, fy=40.0, cx=21.5, cy=17.5, splat=1, z_max=30.0)
    return dict(xyz=x, pose_w=poses, color=color, extrinsic=mf.QUARTER, view_offset=chase_offset() if offset else None, width=W, height=H, **P)


def many_points():
    rng = np.random.default_rng(17)
    P = dict(fx=150.0, fy=150.0, cx=87.5, cy=71.5)
    x = random_cloud(70000, 176, 144, P, rng)
    return dict(xyz=x, pose_w=IDENT[None], color=rng.integers(0, 256, 70000).astype(np.uint8), width=176, height=144, **P)


def one_pixel(n=20000):
    """n points on the optical axis with distinct zq, in random order: all on the pixel nearest (cx, cy)"""
    rng = np.random.default_rng(23)
    z = 1.0 + rng.permutation(n) * 2.0 ** -12
    x = np.stack([np.zeros(n), np.zeros(n), z], 1)
    return dict(xyz=x, pose_w=IDENT[None], color=None, width=9, height=7, fx=10.0, fy=10.0, cx=4.0, cy=3.0)


CASES = {
    "tiny": tiny,
    "ties": ties,
    "footprints": footprints,
    "footprints_radius": lambda: footprints(radius=0.25),
    "strips_176x144": lambda: strips(176, 144, n=6000, splat=1),
    "strips_200x83": lambda: strips(200, 83, n=4000, splat=2),
    "height_1": lambda: strips(300, 1, n=600, splat=1, channels=1),
    "width_1": lambda: strips(1, 300, n=600, splat=1, channels=0),
    "widest_tiles": lambda: strips(STRIP, 2, n=3000, splat=1, channels=1),
    "one_column_more": lambda: strips(STRIP + 1, 2, n=3000, splat=1, channels=1),
    "many_views_rgb": lambda: many_views(3),
    "many_views_grey": lambda: many_views(1),
    "many_views_plain": lambda: many_views(0, offset=False),
    "many_points": many_points,
    "one_pixel": one_pixel,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """the arguments of a case and, under "want", their rendering in the default form; made once"""
    c = CASES[name]()
    c["want"] = render(**c)
    return c


def depth_check():
    """A cloud a few centimetres from the camera and depth words of ONE quantum (z_scale = 2^-20, so that mq = w exactly): the
    measured image is the restatement's own zq shifted by 0, +-tq and +-(tq + 1) quanta and, on every sixth covered pixel, an invalid
    word; the uncovered pixels carry a valid word (measured, not covered) or 0"""
    W, H, n = 60, 50, 1500
    rng = np.random.default_rng(41)
    P = dict(fx=55.0, fy=55.0, cx=29.5, cy=24.5, z_scale=2.0 ** -QBITS, z_min=0.001, z_max=0.06, agree_tol=0.001, splat=1)
    x = random_cloud(n, W, H, P, rng, z_lo=0.02, z_hi=0.05, margin=2.0)
    c = dict(xyz=x, pose_w=np.stack([IDENT, np.concatenate([[0.001, 0.0, -0.002], mf.quat_axis(1, 0.02)])]), color=None, width=W, height=H, **P)
    zq = render(**c)["zq"].astype(np.int64)
    tq = int(np.rint(P["agree_tol"] * TWO20))
    assert tq == 1049
    shifts = np.array([0, tq, -tq, tq + 1, -(tq + 1), 0])
    k = np.arange(zq.size).reshape(zq.shape) % 6
    w = zq + shifts[k]
    w[k == 5] = 65535                                   # zm = 0.0625 > z_max: not valid
    w = np.where(zq >= 0, w, np.where(k % 2 == 0, 30000, 0))
    assert w.min() >= 0 and w.max() <= 65535
    c["depth"] = w.astype(np.uint16)
    return c


CASES["depth_check"] = depth_check


def with_form(want, form, W):
    """the expected outputs of a call that ran in `form`: only the two result fields differ"""
    f, rows = form_fields(form, W)
    return dict(want, form=f, tile_rows=rows)
