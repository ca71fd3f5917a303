"""Numpy restatement of fgo_map_fuse_batch (include/fgo.h), written from the stated semantics and not from the kernel: every
product, quotient and sum is a numpy ufunc of its own (numpy has no fused multiply-add), np.rint for the quantum, int64 floor
division for the voxel index, np.unique on the keys and np.add.at on int64 for the sums.  PCL's VoxelGrid is not in the reference
tree, so this file IS the yardstick of csrc/kernels_map_fuse.hip; tests/test_map_fuse_reference_cpu.py pins it on the CPU.

fuse() returns the outputs of the call and, under "debug", what the CPU tests need: the unquantised world points of the stored
points and their keys.  The scene maker renders the three-wall corner of tests/plane_extract_reference.py from poses along a short
trajectory; CONFIGS lists the calls of tests/test_gpu_map_fuse.py and case(name) makes (and keeps) one of them."""
import functools
import math

import numpy as np

from tests import plane_extract_reference as px

MAP_OK, MAP_TRUNCATED, MAP_FULL = 0, 1, 2
QBITS = 20                    # the quantum is 2^-20 m
IMAX = 1 << 20                # |i_k| < 2^20
DEFAULTS = dict(fx=250.5773, fy=250.5773, cx=90.0, cy=70.0, z_scale=0.001, z_min=0.1, z_max=5.0, skip=2, rect=(0, 0, 0, 0), leaf=0.02,
                min_points=1, table_log2=0)
RESULT_FIELDS = ("status", "table_log2", "n_sampled", "n_valid", "n_out_of_range", "n_voxels", "n_dropped")


def quat_matrix(q):
    """q normalised (the sum of squares taken left to right), then the nine expressions of the header; Python floats round every
    operation on its own"""
    x, y, z, w = (float(v) for v in q)
    n = math.sqrt(((x * x + y * y) + z * z) + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                     [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                     [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]])


def pose_rt(pose7, extrinsic7=None):
    """the 12 doubles of rt_out: R row-major, then t"""
    pose7 = np.asarray(pose7, np.float64)
    R, t = quat_matrix(pose7[3:]), pose7[:3].copy()
    if extrinsic7 is not None:
        e = np.asarray(extrinsic7, np.float64)
        Re, te = quat_matrix(e[3:]), e[:3]
        Rw = R
        R = np.empty((3, 3))
        for i in range(3):
            for j in range(3):
                R[i, j] = (Rw[i, 0] * Re[0, j] + Rw[i, 1] * Re[1, j]) + Rw[i, 2] * Re[2, j]
        t = np.array([((Rw[i, 0] * te[0] + Rw[i, 1] * te[1]) + Rw[i, 2] * te[2]) + t[i] for i in range(3)])
    return np.concatenate([R.reshape(-1), t])


def sample_grid(W, H, P):
    """the sampled columns and rows"""
    su, sv, eu, ev = P["rect"]
    if (su, sv, eu, ev) == (0, 0, 0, 0):
        eu, ev = W, H
    return np.arange(su, eu, P["skip"]), np.arange(sv, ev, P["skip"])


def auto_table_log2(n_sampled):
    """the smallest T >= 4 with 2^T >= 2 n_sampled"""
    T = 4
    while (1 << T) < 2 * n_sampled:
        T += 1
    return T


def leaf_quanta(leaf):
    return int(np.rint(leaf * float(1 << QBITS)))


def make_key(ix, iy, iz):
    return ((iz + IMAX) << 42) | ((iy + IMAX) << 21) | (ix + IMAX)


def split_key(key):
    key = np.asarray(key, np.int64)
    m = (1 << 21) - 1
    return np.stack([(key & m) - IMAX, ((key >> 21) & m) - IMAX, (key >> 42) - IMAX], -1)


def world_points(depth_f, rt, P, us, vs):
    """one frame: the world points of its sampled pixels (v-major), and the valid mask"""
    w = depth_f[np.ix_(vs, us)].reshape(-1)
    u = np.tile(us, len(vs)).astype(np.float64)
    v = np.repeat(vs, len(us)).astype(np.float64)
    z = w.astype(np.float64) * P["z_scale"]
    valid = (z > P["z_min"]) & (z < P["z_max"])
    p0 = ((u - P["cx"]) * z) / P["fx"]
    p1 = ((v - P["cy"]) * z) / P["fy"]
    R, t = rt[:9].reshape(3, 3), rt[9:]
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.stack([((R[k, 0] * p0 + R[k, 1] * p1) + R[k, 2] * z) + t[k] for k in range(3)], 1)
    return x, valid


def quantise(x, L):
    """Q, i, r of the points x (m x 3) and the mask of those in range"""
    with np.errstate(invalid="ignore", over="ignore"):
        y = x * float(1 << QBITS)
        ok = np.all(np.isfinite(x), 1) & np.all(np.abs(y) < 2.0 ** 62, 1)
    Q = np.zeros(x.shape, np.int64)
    Q[ok] = np.rint(y[ok]).astype(np.int64)
    i = Q // L
    r = Q - i * L
    ok &= np.all(np.abs(i) < IMAX, 1)
    return Q, i, r, ok


def fuse(depth, pose_w, color=None, extrinsic=None, max_voxels=None, **params):
    P = dict(DEFAULTS, **params)
    depth = np.asarray(depth, np.uint16)
    n, H, W = depth.shape
    pose_w = np.asarray(pose_w, np.float64).reshape(n, 7)
    ch = 0 if color is None else (1 if color.ndim == 3 else color.shape[3])
    us, vs = sample_grid(W, H, P)
    L = leaf_quanta(P["leaf"])
    rt = np.stack([pose_rt(pose_w[f], extrinsic) for f in range(n)]) if n else np.zeros((0, 12))
    keys, rs, cols, xs = [], [], [], []
    frame_points = np.zeros(n, np.int64)
    n_oor = 0
    for f in range(n):
        x, valid = world_points(depth[f], rt[f], P, us, vs)
        _, i, r, ok = quantise(x, L)
        n_oor += int(np.sum(valid & ~ok))
        keep = valid & ok
        frame_points[f] = int(keep.sum())
        keys.append(make_key(i[keep, 0], i[keep, 1], i[keep, 2])); rs.append(r[keep]); xs.append(x[keep])
        if ch:
            cols.append(color[f].reshape(H, W, ch)[np.ix_(vs, us)].reshape(-1, ch)[keep].astype(np.int64))
    keys = np.concatenate(keys) if n else np.zeros(0, np.int64)
    rs = np.concatenate(rs) if n else np.zeros((0, 3), np.int64)
    uniq, inv = np.unique(keys, return_inverse=True)
    cnt = np.zeros(len(uniq), np.int64); S = np.zeros((len(uniq), 3), np.int64); Cs = np.zeros((len(uniq), ch), np.int64)
    np.add.at(cnt, inv, 1)
    np.add.at(S, inv, rs)
    if ch and n:
        np.add.at(Cs, inv, np.concatenate(cols))
    keep = cnt >= P["min_points"]
    key, cnt, S, Cs = uniq[keep], cnt[keep], S[keep], Cs[keep]
    nf = cnt.astype(np.float64)[:, None]
    xyz = ((split_key(key) * L).astype(np.float64) + S.astype(np.float64) / nf) * 2.0 ** -QBITS
    col = ((2 * Cs + cnt[:, None]) // (2 * cnt[:, None])).astype(np.uint8)
    n_sampled = n * len(us) * len(vs)
    nv = len(key)
    m = nv if max_voxels is None else min(nv, max_voxels)
    out = dict(status=MAP_OK if m == nv else MAP_TRUNCATED, table_log2=P["table_log2"] or auto_table_log2(n_sampled), n_sampled=n_sampled,
               n_valid=int(frame_points.sum()), n_out_of_range=n_oor, n_voxels=nv, n_dropped=int(np.sum(~keep)),
               xyz=xyz[:m], color=col[:m] if ch else None, count=cnt[:m].astype(np.int32), key=key[:m], frame_points=frame_points, rt=rt,
               debug=dict(x=np.concatenate(xs) if n else np.zeros((0, 3)), key=keys))
    return out


# ---- the scene maker

def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def quat_axis(axis, angle):
    q = np.zeros(4)
    q[axis] = np.sin(0.5 * angle); q[3] = np.cos(0.5 * angle)
    return q


ROOM_LO, ROOM_HI = np.array([-40.0, -40.0, -40.0]), np.array([1.6, 1.1, 2.2])      # the corner of plane_extract_reference.corner_scene


def corner_pose(rng=None, shift=np.zeros(3), wobble=1.0):
    """a pose (t, q_xyzw) inside the room that looks into its corner: front wall, right wall and floor in view"""
    d = np.zeros(5) if rng is None else wobble * rng.uniform(-1, 1, 5)
    q = quat_mul(quat_axis(1, np.deg2rad(40.0 + 4.0 * d[0])), quat_axis(0, np.deg2rad(-25.0 + 3.0 * d[1])))
    return np.concatenate([0.1 * d[2:] - shift, q])


def render_frame(pose7, W, H, cam, sigma, rng, shift=np.zeros(3), extrinsic=None):
    """the depth words and the wall index of the room's corner (moved by -shift) seen from the camera at pose7 (x extrinsic)"""
    rt = pose_rt(pose7, extrinsic)
    planes = px.room_planes(ROOM_LO - shift, ROOM_HI - shift, rt[:9].reshape(3, 3), rt[9:])
    return px.render(planes, W, H, cam, sigma, rng)


SIGMA_Z = 0.014
SHIFT = np.array([1.0, 0.7, 1.5])                      # puts the world's origin inside the view: the walls at x = 0.6, y = 0.4, z = 0.7
QUARTER = np.array([0.02, -0.01, 0.03, 0.0, 0.0, math.sqrt(0.5), math.sqrt(0.5)])     # Pu2c: a quarter turn about z and a small offset

# name, frames, W, H, channels, params; flags: empty (a frame of zeros), one_pose, extrinsic, shift (of the world; default SHIFT)
CONFIGS = [
    dict(name="tiny", n=1, W=7, H=5, channels=0, params=dict(skip=1, leaf=0.05)),
    dict(name="small_skip1", n=6, W=44, H=36, channels=3, params=dict(skip=1, rect=(3, 2, 41, 35), leaf=0.05)),
    dict(name="small_skip3", n=6, W=44, H=36, channels=1, params=dict(skip=3, rect=(5, 1, 44, 34), leaf=0.05)),
    dict(name="big_across_origin", n=3, W=176, H=144, channels=3, params=dict(skip=2)),
    dict(name="empty_frame", n=4, W=44, H=36, channels=0, params=dict(skip=1, leaf=0.05), empty=1),
    dict(name="one_pose_leaf8", n=5, W=44, H=36, channels=3, params=dict(skip=1, leaf=8.0), one_pose=True, shift=(-3.0, -3.0, -3.0)),
    dict(name="fine_leaf", n=3, W=44, H=36, channels=1, params=dict(skip=1, leaf=2.0 ** -10)),
    dict(name="extrinsic_quarter_turn", n=4, W=44, H=36, channels=0, params=dict(skip=1, leaf=0.05), extrinsic=True),
    dict(name="many_tiny", n=150, W=7, H=5, channels=1, params=dict(skip=1, leaf=0.05)),     # more frames than a tile groups (128)
    dict(name="min_points3", n=6, W=44, H=36, channels=3, params=dict(skip=1, leaf=0.05, min_points=3)),
]


def make_case(cfg, seed=20263):
    """depth (n x H x W), pose_w (n x 7), color (n x H x W [x 3]) or None, extrinsic or None, params"""
    rng = np.random.default_rng(seed + sum(map(ord, cfg["name"])))
    n, W, H, ch = cfg["n"], cfg["W"], cfg["H"], cfg["channels"]
    cam = px.camera(W, H)
    ext = QUARTER if cfg.get("extrinsic") else None
    shift = np.array(cfg.get("shift", SHIFT))                       # one_pose_leaf8: the whole view inside one voxel of 8 m
    base = corner_pose(None, shift)
    poses = np.stack([base if cfg.get("one_pose") else corner_pose(rng, shift) for _ in range(n)])
    depth = np.stack([render_frame(poses[f], W, H, cam, SIGMA_Z, rng, shift, ext)[0] for f in range(n)])
    if "empty" in cfg:
        depth[cfg["empty"]] = 0
    color = None
    if ch:
        color = rng.integers(0, 256, (n, H, W) if ch == 1 else (n, H, W, 3)).astype(np.uint8)
    return dict(depth=depth, pose_w=poses, color=color, extrinsic=ext, params=dict(cam, **cfg["params"]))


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of a configuration and their fused map, made once"""
    c = make_case(next(c for c in CONFIGS if c["name"] == name))
    c["want"] = fuse(c["depth"], c["pose_w"], c["color"], c["extrinsic"], **c["params"])
    return c


def read_ply(path):
    """the vertices of an ASCII PLY written by write_ply: xyz (m x 3) and rgb (m x 3)"""
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    m = int(next(ln for ln in lines[:end] if ln.startswith("element vertex")).split()[2])
    rows = np.array([[float(v) for v in ln.split()] for ln in lines[end + 1:end + 1 + m]]).reshape(m, 6)
    return lines[:end + 1], rows[:, :3], rows[:, 3:].astype(np.int64)
