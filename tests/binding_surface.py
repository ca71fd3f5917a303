"""Recorder of the Python binding's surface (test infrastructure, no GPU): what every batch wrapper returns for empty input with
every want_* switched on -- the ordered keys and per key the type, dtype, shape and whether the array is a view -- the signature
of every public function and Graph method, and the sorted public names of the package.  All fourteen wrappers get FGO_OK from
the library for empty input before its first HIP call, so this runs anywhere.

`python -m tests.binding_surface > tests/golden/binding_surface.json` writes the golden file; tests/test_binding_surface_cpu.py
says which commit it was written at and compares the tree with it."""
import inspect
import json

import numpy as np


def describe(v):
    if isinstance(v, dict):
        return {"type": "dict", "items": [[k, describe(x)] for k, x in v.items()]}
    if isinstance(v, np.ndarray):
        return {"type": "ndarray", "dtype": v.dtype.str, "shape": list(v.shape), "view": v.base is not None}
    if isinstance(v, (tuple, list)):
        return {"type": type(v).__name__, "items": [describe(x) for x in v]}
    return {"type": type(v).__name__}


def calls(G):
    """name -> thunk, one per wrapper (and the two composed ones), each on empty input"""
    z = np.zeros
    u8, u16, i8, i32, i64 = np.uint8, np.uint16, np.int8, np.int32, np.int64
    ptr0 = z(1, i64)
    none = z(0, i64)
    info = z((0, 21))
    pose = z((0, 7))
    frames = dict(depth=z((1, 4, 6), u16), intensity=z((1, 4, 6), u8), labels=z((1, 4, 6), i8), n_planes=z(1, i32),
                  abcd=z((1, 2, 4)), cov16=z((1, 2, 16)), frame_i=none, frame_j=none, pose_ij=pose)
    feats = dict(feat_ptr=ptr0, desc=z((0, 128), u8), xyz=z((0, 3)), uv=z((0, 2)), frame_i=none, frame_j=none)
    return {
        "preint_batch": lambda: G.preint_batch(ptr0, z((0, 3)), z((0, 3)), 0.005),
        "two_view_ba_batch": lambda: G.two_view_ba_batch(ptr0, z((0, 3)), z((0, 2)), z((0, 2)), z(9)),
        "plane_check_vro_batch": lambda: G.plane_check_vro_batch(pose, ptr0, z((0, 4)), z((0, 16)), ptr0, z((0, 4)), z((0, 16)), info=info),
        "plane_check_vro_batch(cov)": lambda: G.plane_check_vro_batch(pose, ptr0, z((0, 4)), z((0, 16)), ptr0, z((0, 4)), z((0, 16)),
                                                                      cov=z((0, 6, 6))),
        "imu_check_vro_batch": lambda: G.imu_check_vro_batch(pose, z((0, G.PREINT_DOUBLES)), none, info=info, bias_i=z((0, 6)),
                                                             imu_q_cam=np.array([0.0, 0, 0, 1]), want_dw=True, want_cov=True),
        "imu_check_vro_batch(plain)": lambda: G.imu_check_vro_batch(pose, z((0, G.PREINT_DOUBLES)), none, cov=z((0, 6, 6))),
        "vro_ransac_batch": lambda: G.vro_ransac_batch(ptr0, z((0, 3)), z((0, 3)), want_hyp_counts=True),
        "vro_ransac_batch(plain)": lambda: G.vro_ransac_batch(ptr0, z((0, 3)), z((0, 3)), want_info=False, want_cov=False,
                                                              want_inliers=False),
        "plane_extract_batch": lambda: G.plane_extract_batch(z((0, 4, 6), u16), want_labels=True, want_hyp_counts=True),
        "plane_propagate_batch": lambda: G.plane_propagate_batch(info=info, **frames),
        "plane_propagate_batch(plain)": lambda: G.plane_propagate_batch(cov=z((0, 6, 6)), want_labels=False, want_pred=False,
                                                                        want_planes=False, want_ut6=False, **frames),
        "plane_node_batch": lambda: G.plane_node_batch(info=info, **frames),
        "match_features_batch": lambda: G.match_features_batch(pose_ij=pose, guided=z(0, bool), want_dist=True, **feats),
        "vro_adjust_batch": lambda: G.vro_adjust_batch(pose_ij=pose, **feats),
        "map_fuse_batch": lambda: G.map_fuse_batch(z((0, 4, 6), u16), pose, color=z((0, 4, 6, 3), u8), extrinsic=[0, 0, 0, 0, 0, 0, 1.0],
                                                   want_keys=True, want_rt=True),
        "map_fuse_batch(plain)": lambda: G.map_fuse_batch(z((0, 4, 6), u16), pose),
        "map_clean": lambda: G.map_clean(z((0, 3)), color=z((0, 3), u8), count=z(0, i32)),
        "map_clean(plain)": lambda: G.map_clean(z((0, 3))),
        "map_normals": lambda: G.map_normals(z((0, 3)), want_neighbours=True, want_scatter=True),
        "map_render_batch": lambda: G.map_render_batch(z((0, 3)), pose, color=z((0, 3), u8), extrinsic=[0, 0, 0, 0, 0, 0, 1.0],
                                                       view_offset=[0, 0, 0, 0, 0, 0, 1.0], width=6, height=4,
                                                       depth=z((0, 4, 6), u16), want_index=True, want_rt=True),
        "map_render_batch(grey)": lambda: G.map_render_batch(z((0, 3)), z((0, 7)), color=z(0, u8), width=6, height=4),
    }


def signatures(G):
    out = {}
    for name in sorted(vars(G)):
        f = getattr(G, name)
        if inspect.isfunction(f):
            out[name] = str(inspect.signature(f))
    for cls in (G.Graph, G.Preintegrator):
        for name, f in sorted(vars(cls).items()):
            if inspect.isfunction(f):
                out["%s.%s" % (cls.__name__, name)] = str(inspect.signature(f))
    return out


def record(G):
    return {"results": {name: describe(call()) for name, call in calls(G).items()},
            "signatures": signatures(G),
            "public_names": sorted(n for n in vars(G) if not n.startswith("__"))}


if __name__ == "__main__":
    import graph_slam_amd
    print(json.dumps(record(graph_slam_amd), indent=1))
