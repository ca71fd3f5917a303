"""The map calls of libfgo.so, one wrapper per call -- voxel-grid fusion of depth frames, cluster filtering and floor removal,
surface normals, z-buffer rendering -- with the cameras to render from and the writers of the files to look at."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import (FGO_MAP_FULL, FgoError, MapCleanParams, MapCleanResult, MapNormalsParams, MapNormalsResult, MapParams, MapRenderParams,
                   MapRenderResult, MapRenderView, MapResult, call, fields, opt, ptr, records)


def map_params(**kw):
    """fgo_map_params_default, with the given fields replaced (rect: su, sv, eu, ev)"""
    return _abi.params(MapParams, **kw)


def map_fuse_batch(depth, pose_w, color=None, extrinsic=None, params=None, max_voxels=None, want_keys=False, want_rt=False, device=0):
    """fgo_map_fuse_batch: the voxel-grid map of all depth frames in one call.  depth is n x H x W (or H x W for one frame) of uint16
    depth words, pose_w n x 7 (t, q_xyzw: Graph.get_poses), color None, n x H x W (grey) or n x H x W x 3 (uint8), extrinsic the 7
    numbers of Pu2c or None.  max_voxels defaults to the bound n_sampled.  Returns a dict: xyz (m x 3), color (m x channels, None
    without colour), count (m, int32), frame_points (n, int64), with want_keys key (m, int64) and with want_rt rt (n x 12), each
    trimmed to m = min(n_voxels, max_voxels), in ascending key; and the result fields status (FGO_MAP_*), table_log2, n_sampled,
    n_valid, n_out_of_range, n_voxels, n_dropped."""
    d = np.ascontiguousarray(depth, np.uint16)
    if d.ndim == 2:
        d = d[None]
    if d.ndim != 3:
        raise FgoError("map_fuse_batch: depth is n x H x W")
    n, h, w = d.shape
    ps = np.ascontiguousarray(pose_w, np.float64).reshape(-1, 7)
    if len(ps) != n:
        raise FgoError("map_fuse_batch: pose_w needs one row of 7 per frame")
    col, ch = None, 0
    if color is not None:
        col = np.ascontiguousarray(color, np.uint8)
        if col.shape == (h, w) or col.shape == (h, w, 3):
            col = col[None]
        if col.shape not in ((n, h, w), (n, h, w, 1), (n, h, w, 3)):
            raise FgoError("map_fuse_batch: color is n x H x W or n x H x W x 3")
        ch = 3 if col.shape[-1] == 3 and col.ndim == 4 else 1
    ext = None if extrinsic is None else np.ascontiguousarray(extrinsic, np.float64).reshape(7)
    if params is None:
        params = map_params()
    if max_voxels is None:                                        # the bound n_sampled; a bad argument is the library's to refuse
        su, sv, eu, ev = params.rect
        if (su, sv, eu, ev) == (0, 0, 0, 0):
            eu, ev = w, h
        k = max(params.skip, 1)
        max_voxels = n * max(-(-(eu - su) // k), 0) * max(-(-(ev - sv) // k), 0)
    cap = max(int(max_voxels), 0)
    xyz = np.zeros((cap, 3)); cout = np.zeros((cap, ch), np.uint8) if ch else None
    cnt = np.zeros(cap, np.int32); key = np.zeros(cap, np.int64) if want_keys else None
    fpts = np.zeros(n, np.int64); rt = np.zeros((n, 12)) if want_rt else None
    res = MapResult()
    call("fgo_map_fuse_batch", device, n, w, h, ptr(d), opt(col), ch, ptr(ps), opt(ext), C.byref(params), int(max_voxels), C.byref(res),
         ptr(xyz), opt(cout), ptr(cnt), opt(key), ptr(fpts), opt(rt))
    out = fields(res)
    m = 0 if res.status == FGO_MAP_FULL else min(res.n_voxels, cap)
    out.update(xyz=xyz[:m], color=None if cout is None else cout[:m], count=cnt[:m], frame_points=fpts)
    if key is not None:
        out["key"] = key[:m]
    if rt is not None:
        out["rt"] = rt
    return out


def map_clean_params(**kw):
    """fgo_map_clean_params_default, with the given fields replaced"""
    return _abi.params(MapCleanParams, **kw)


def map_clean(xyz, color=None, count=None, params=None, device=0):
    """fgo_map_clean: cluster filtering and floor removal of a cloud in one call.  xyz is n x 3 (map_fuse_batch's "xyz", or any
    cloud), color (n or n x channels) and count (n) ride along when given.  Returns a dict: label (n, int32; -1 out of range), reason
    (n, uint8: 0 kept, 1 out of range, 2 cluster size, 3 floor), cluster_size (n_clusters, int32), index (n_kept, int64, ascending),
    xyz (n_kept x 3, the floor at zero of the up axis), color and count gathered through index (None when not given); and the
    result fields n_points, n_out_of_range, n_cells, n_clusters, n_clusters_kept, n_after_clusters, n_floor_removed, n_kept,
    floor_bin, floor_bin_points, floor_height."""
    x = np.ascontiguousarray(xyz, np.float64)
    if x.ndim != 2 or x.shape[1] != 3:
        raise FgoError("map_clean: xyz is n x 3")
    n = len(x)
    col = None if color is None else np.asarray(color)
    if col is not None and (col.ndim not in (1, 2) or len(col) != n):
        raise FgoError("map_clean: color needs one row per point")
    cnt = None if count is None else np.asarray(count)
    if cnt is not None and cnt.shape != (n,):
        raise FgoError("map_clean: count needs one entry per point")
    if params is None:
        params = map_clean_params()
    label = np.zeros(n, np.int32); reason = np.zeros(n, np.uint8); csize = np.zeros(n, np.int32)
    index = np.zeros(n, np.int64); out_xyz = np.zeros((n, 3))
    res = MapCleanResult()
    call("fgo_map_clean", device, n, ptr(x), C.byref(params), C.byref(res), ptr(label), ptr(reason), ptr(csize), ptr(index), ptr(out_xyz))
    out = fields(res)
    index = index[:res.n_kept]
    out.update(label=label, reason=reason, cluster_size=csize[:res.n_clusters], index=index, xyz=out_xyz[:res.n_kept],
               color=None if col is None else col[index], count=None if cnt is None else cnt[index])
    return out


def map_normals_params(**kw):
    """fgo_map_normals_params_default, with the given fields replaced (viewpoint: 3 numbers)"""
    return _abi.params(MapNormalsParams, **kw)


def map_normals(xyz, params=None, want_neighbours=False, want_scatter=False, device=0):
    """fgo_map_normals: the k nearest neighbours of every point of a cloud and the surface normal and curvature fitted to them, in
    one call.  xyz is n x 3 (map_clean's "xyz", or any cloud).  Returns a dict: normal (n x 3, unit, turned towards the viewpoint),
    curvature (n), eigenvalues (n x 3, ascending), n_neighbours (n, int32), status (n, uint8: 0 valid, 1 out of range, 2 fewer than 3
    neighbours, 3 all neighbours coincide; NaN in the floating outputs unless 0); with want_neighbours neighbour (n x k, int32, the
    point itself included, padded with -1) and dist2 (n x k, int64, squared distances in quanta of 2^-20 m), with want_scatter
    scatter (n x 6, int64); and the result fields n_points, n_out_of_range, n_cells, n_valid, n_few, n_degenerate."""
    x = np.ascontiguousarray(xyz, np.float64)
    if x.ndim != 2 or x.shape[1] != 3:
        raise FgoError("map_normals: xyz is n x 3")
    n = len(x)
    if params is None:
        params = map_normals_params()
    k = max(int(params.k), 0)
    normal = np.zeros((n, 3)); curv = np.zeros(n); eig = np.zeros((n, 3))
    nn = np.zeros(n, np.int32); status = np.zeros(n, np.uint8)
    nb = np.zeros((n, k), np.int32) if want_neighbours else None
    d2 = np.zeros((n, k), np.int64) if want_neighbours else None
    sc = np.zeros((n, 6), np.int64) if want_scatter else None
    res = MapNormalsResult()
    call("fgo_map_normals", device, n, ptr(x), C.byref(params), C.byref(res), ptr(normal), ptr(curv), ptr(eig), ptr(nn), ptr(status),
         opt(nb), opt(d2), opt(sc))
    out = fields(res)
    out.update(normal=normal, curvature=curv, eigenvalues=eig, n_neighbours=nn, status=status)
    if want_neighbours:
        out.update(neighbour=nb, dist2=d2)
    if want_scatter:
        out["scatter"] = sc
    return out


def map_render_params(**kw):
    """fgo_map_render_params_default, with the given fields replaced (background: 3 numbers)"""
    return _abi.params(MapRenderParams, **kw)


def map_render_batch(xyz, pose_w, color=None, extrinsic=None, view_offset=None, width=176, height=144, params=None, depth=None,
                     want_zq=True, want_index=False, want_color=None, want_rt=False, device=0):
    """fgo_map_render_batch: the cloud drawn from every pose in one call, by a z-buffer.  xyz is n x 3 (map_fuse_batch's "xyz", or any
    cloud), color None, n (grey) or n x 3 (uint8), pose_w V x 7 (t, q_xyzw: Graph.get_poses, or a list of look_at poses), extrinsic
    the 7 numbers of Pu2c or None, view_offset a further pose composed on the right or None (look_at((0, -2, -5), (0, 0, 5),
    (0, -0.98, 0.199)) is the reference's chase camera), depth None or V x H x W uint16 measured depth words to check the map
    against.  want_color defaults to whether color is given.  Returns a dict: with want_zq zq (V x H x W, int32: the depth in quanta
    of 2^-20 m, -1 where nothing was drawn), with want_index index (V x H x W, int32, the drawn point or -1), with want_color color
    (V x H x W x channels, uint8; V x H x W for grey), with want_rt rt (V x 12); the per-view counts n_valid, n_drawn, n_pixels,
    n_meas, n_both, n_agree, n_closer, n_through (V, int64); and the result fields n_points, n_nonfinite, form, tile_rows."""
    x = np.ascontiguousarray(xyz, np.float64)
    if x.ndim != 2 or x.shape[1] != 3:
        raise FgoError("map_render_batch: xyz is n x 3")
    n = len(x)
    ps = np.ascontiguousarray(pose_w, np.float64)
    if ps.ndim == 1 and ps.size == 7:
        ps = ps[None]
    if ps.ndim != 2 or ps.shape[1] != 7:
        raise FgoError("map_render_batch: pose_w is V x 7")
    nv, w, h = len(ps), int(width), int(height)
    col, ch, grey = None, 0, False
    if color is not None:
        col = np.ascontiguousarray(color, np.uint8)
        grey = col.ndim == 1
        if col.shape not in ((n,), (n, 1), (n, 3)):
            raise FgoError("map_render_batch: color is n or n x 3")
        ch = 3 if col.ndim == 2 and col.shape[1] == 3 else 1
    if want_color is None:
        want_color = ch > 0
    if want_color and ch == 0:
        raise FgoError("map_render_batch: want_color needs color")
    ext = None if extrinsic is None else np.ascontiguousarray(extrinsic, np.float64).reshape(7)
    off = None if view_offset is None else np.ascontiguousarray(view_offset, np.float64).reshape(7)
    dm = None
    if depth is not None:
        dm = np.ascontiguousarray(depth, np.uint16)
        if dm.shape == (h, w):
            dm = dm[None]
        if dm.shape != (nv, h, w):
            raise FgoError("map_render_batch: depth is V x H x W")
    if params is None:
        params = map_render_params()
    hh, ww = max(h, 0), max(w, 0)                                  # a bad size is the library's to refuse
    zq = np.zeros((nv, hh, ww), np.int32) if want_zq else None
    index = np.zeros((nv, hh, ww), np.int32) if want_index else None
    cout = np.zeros((nv, hh, ww, ch), np.uint8) if want_color else None
    rt = np.zeros((nv, 12)) if want_rt else None
    views = (MapRenderView * max(nv, 1))()
    res = MapRenderResult()
    call("fgo_map_render_batch", device, n, ptr(x), opt(col), ch, nv, ptr(ps), opt(ext), opt(off), w, h, C.byref(params), opt(dm),
         C.byref(res), views, opt(zq), opt(index), opt(cout), opt(rt))
    out = fields(res)
    out.update(records(views, nv))
    if zq is not None:
        out["zq"] = zq
    if index is not None:
        out["index"] = index
    if cout is not None:
        out["color"] = cout[..., 0] if grey else cout
    if rt is not None:
        out["rt"] = rt
    return out


def look_at_matrix(eye, target, up):
    """R = [x y z] (columns) of look_at: z = normalise(target - eye), x = normalise((-up) x z), y = z x x.  x is made orthogonal to
    z once more after the cross product, so that R stays orthonormal to rounding when up is close to the line of sight."""
    eye, target, up = (np.asarray(v, np.float64).reshape(3) for v in (eye, target, up))
    z = target - eye
    nz = np.linalg.norm(z)
    x = np.cross(-up, z)
    nx = np.linalg.norm(x)
    if not (nz > 0 and nx > 0 and np.isfinite(nz) and np.isfinite(nx)):
        raise FgoError("look_at: target equals eye, or up is parallel to the line of sight")
    z = z / nz; x = x / nx
    x = x - (x @ z) * z
    x = x / np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], 1)


def look_at(eye, target, up):
    """the pose7 (t, q_xyzw) of a camera at eye that looks at target, in the camera convention of the map calls (x right, y down,
    z forward): R = look_at_matrix(eye, target, up), t = eye.  As pose_w of map_render_batch it is a camera in the world (a list of
    them: an arc flown round the map); as view_offset it is a camera placed relative to every pose:
    look_at((0, -2, -5), (0, 0, 5), (0, -0.98, 0.199)) is the chase camera of the reference's mapping/map_video.cpp:119-127."""
    R = look_at_matrix(eye, target, up)
    # the quaternion of R by the branch with the largest denominator
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * np.sqrt(1.0 + tr)
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(R))); j = (i + 1) % 3; k = (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0, 0.0, 0.0, (R[k, j] - R[j, k]) / s]
        q[i] = 0.25 * s; q[j] = (R[j, i] + R[i, j]) / s; q[k] = (R[k, i] + R[i, k]) / s
    q = np.asarray(q)
    return np.concatenate([np.asarray(eye, np.float64).reshape(3), q / np.linalg.norm(q)])


def write_ppm(path, image):
    """a binary PPM (P6) for an H x W x 3 uint8 image, a binary PGM (P5) for H x W: one frame of map_render_batch's "color", to be
    looked at without an image library"""
    im = np.asarray(image)
    if im.dtype != np.uint8 or not (im.ndim == 2 or (im.ndim == 3 and im.shape[2] == 3)):
        raise FgoError("write_ppm: image is H x W x 3 or H x W, uint8")
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P6" if im.ndim == 3 else b"P5", im.shape[1], im.shape[0]))
        f.write(np.ascontiguousarray(im).tobytes())


def write_ply(path, xyz, color=None, normals=None):
    """an ASCII PLY in the layout of the reference's headerPLY (mapping/mapping_PCD.cpp:169-181): float x y z, uchar red green blue.
    color is m x 3, m or m x 1 (grey, repeated three times) or None (255).  With normals (m x 3: map_normals' "normal") the vertex
    also has float nx ny nz after z, the XYZ+RGB+normal cloud of pcd2mesh.cpp:65-67; without, the file is what it always was."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    m = len(xyz)
    if color is None:
        rgb = np.full((m, 3), 255, np.uint8)
    else:
        rgb = np.asarray(color, np.uint8).reshape(m, -1)
        if rgb.shape[1] == 1:
            rgb = np.repeat(rgb, 3, 1)
        if rgb.shape[1] != 3:
            raise FgoError("write_ply: color is m x 3 or m")
    nrm = None
    if normals is not None:
        nrm = np.asarray(normals, np.float64)
        if nrm.shape != (m, 3):
            raise FgoError("write_ply: normals is m x 3")
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % m)
        if nrm is not None:
            f.write("property float nx\nproperty float ny\nproperty float nz\n")
        f.write("property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        if nrm is None:
            for p, c in zip(xyz, rgb):
                f.write("%.9g %.9g %.9g %d %d %d\n" % (p[0], p[1], p[2], c[0], c[1], c[2]))
        else:
            for p, v, c in zip(xyz, nrm, rgb):
                f.write("%.9g %.9g %.9g %.9g %.9g %.9g %d %d %d\n" % (p[0], p[1], p[2], v[0], v[1], v[2], c[0], c[1], c[2]))

