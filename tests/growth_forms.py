"""Graphs that grow IN PLACE (refresh_factors, structure_grow.cpp) through the forms the linearisation can take afterwards: duplicate
groups forming and gaining members in either orientation, a variable crossing the hub threshold, a one-slice hub becoming a
multi-slice hub, plane / point hubs, variables of every kind claiming phantom slots, priors arriving later, the masked ISAM2
linearisation losing its precondition, and the hub buffers overflowing.

Three parts, used by tests/test_growth_forms_cpu.py (no device), tests/test_gpu_growth_forms.py and tests/growth_forms_child.py:
  * builders: a case is a topology only -- per step the variables (kind, fixed), binary factors (i, j, kind) and priors it adds;
  * ledger(): what the structure phase must make of every step, recomputed in numpy from the rules of plan_hubs / refresh_factors
    (half-edge degrees, hub entries 0 if d <= T else min(64, ceil(d / 512)), duplicate groups, reserve, band, hub_cap) -- the
    figures fgo_debug_linearize_census is compared with, exactly;
  * realise() / drive(): measurements for a topology (seeded) and the run on the device, one record per step."""
import numpy as np

from tests.util import pose_mul, pose_inv, noisy, random_info, info_ut, quat_rot, SR4000_CALIB

POSE, PLANE, POINT = 0, 1, 2                          # variable kinds (VK_*)
SE3, BETWEEN, PLANEF, REPROJ = 0, 1, 2, 3             # factor kinds (FK_*)
HUB_SLICE, HUB_MAX_SLICES, HUB_MAX_VARS, HUB_DEG_MAX = 512, 64, 1024, 1024      # device_plan.hpp
HUB_CAP_EXTRA, EDGE_CAP_EXTRA = 256, 4096             # structure_upload.cpp / structure_tables.cpp: hub entries / edges the growth reserve adds room for
SOFT_PRIOR = info_ut(np.diag([1e6] * 6))              # as tests/test_gpu_isam2.py
BPS = np.concatenate([[0.05, -0.02, 0.1], [0.5, 0.5, 0.5, 0.5]])     # body_P_sensor of tests.util.mixed_graph


def _step(vars=(), factors=(), priors=()):
    return dict(vars=list(vars), factors=list(factors), priors=list(priors))


def _case(name, sem, growth, steps, hub_deg=None, tune="", thr=1e9, linearize_every_step=True, seed=0, note=""):
    return dict(name=name, sem=sem, growth=growth, steps=steps, hub_deg=hub_deg, tune=tune, thr=thr,
                linearize_every_step=linearize_every_step, seed=seed, note=note)


# ---- g2o semantics -----------------------------------------------------------------------------------------------------------
def _lookback_pairs(lo, hi, lookback):
    return [(k - d, k, SE3) for k in range(lo, hi) for d in range(1, lookback + 1) if k - d >= 0]


def case_dup_in_place(twin=False, hub_deg=None):
    """12 poses, odometry + look-back 2, pose 0 fixed.  In place: a second edge on a free pair (same orientation), a third one
    reversed, a second edge on a pair whose other end is fixed (no slot: diagonal only), a second edge on another pair (two groups).
    twin: the first group is already in the build and gains a (reversed) member."""
    build = _step([(POSE, k == 0) for k in range(12)], _lookback_pairs(1, 12, 2))
    if twin:
        build["factors"].append((3, 4, SE3))
        steps = [build, _step(factors=[(4, 3, SE3)])]
    else:
        steps = [build, _step(factors=[(3, 4, SE3)]), _step(factors=[(4, 3, SE3)]), _step(factors=[(0, 1, SE3)]), _step(factors=[(7, 5, SE3)])]
    name = ("dup_twin" if twin else "dup_in_place") + ("_hub2" if hub_deg else "")
    return _case(name, "g2o", (8, 8), steps, hub_deg=hub_deg, tune="hub_deg=%d" % hub_deg if hub_deg else "", seed=11)


def case_hub_by_new_vertices():
    """8 poses; every new pose carries odometry to its predecessor and one edge to pose 7 (pose 8's predecessor IS pose 7: a duplicate
    group of two).  Pose 7 has 1 + 2 + (m - 1) half-edges after m new poses: 64 after 62 (no hub), 65 after one more (one slice)."""
    build = _step([(POSE, k == 0) for k in range(8)], _lookback_pairs(1, 8, 1))

    def grow(lo, hi):
        return _step([(POSE, False)] * (hi - lo), [f for k in range(lo, hi) for f in ((k - 1, k, SE3), (7, k, SE3))])
    return _case("hub_by_new_vertices", "g2o", (80, 96), [build, grow(8, 70), grow(70, 71)], seed=12)


def case_slices_by_duplicates():
    """9-pose star (centre 0, free; pose 1 fixed) + a sparse ring.  Repeated edges on the eight spokes, the orientation alternating on
    every spoke, take the centre through 64, 65, 512, 513, 1024, 1025 half-edges: 0, 1, 1, 2, 2, 3 slices."""
    build = _step([(POSE, k == 1) for k in range(9)], [(0, k, SE3) for k in range(1, 9)] + [(1, 2, SE3), (4, 5, SE3), (7, 8, SE3)])
    steps, t, deg = [build], 0, 8
    for target in (64, 65, 512, 513, 1024, 1025):
        fs = []
        while deg < target:
            k = 1 + t % 8
            fs.append((k, 0, SE3) if (t // 8 + t) % 2 == 0 else (0, k, SE3))
            t += 1; deg += 1
        steps.append(_step(factors=fs))
    return _case("slices_by_duplicates", "g2o", (8, 8), steps, seed=13)


def case_chain_hub2():
    """30-pose chain with look-back 3, built at 24 poses and grown by 3 twice, every variable of degree above 2 a one-slice hub"""
    build = _step([(POSE, k == 0) for k in range(24)], _lookback_pairs(1, 24, 3))
    steps = [build] + [_step([(POSE, False)] * 3, _lookback_pairs(lo, lo + 3, 3)) for lo in (24, 27)]
    return _case("chain_hub2", "g2o", (16, 8), steps, hub_deg=2, tune="hub_deg=2", seed=14)


def case_hub_cap(by_one):
    """300-pose odometry chain with hub_deg = 2: no hubs.  Duplicates on the 255 pairs (1,2) .. (255,256) make the poses 1 .. 256 hubs:
    256 entries = hub_cap, in place.  Then duplicates on the rest (by_one: on the single pair (256,257): 257 entries) overflow the
    buffers: one rebuild.  by_one goes on with the rest, in place again on the rebuilt structure."""
    build = _step([(POSE, k == 0) for k in range(300)], _lookback_pairs(1, 300, 1))
    first = _step(factors=[(k, k + 1, SE3) for k in range(1, 256)])
    rest = [(0, 1, SE3)] + [(k, k + 1, SE3) for k in range(256, 299)]
    steps = [build, first] + ([_step(factors=rest[1:2]), _step(factors=rest[:1] + rest[2:])] if by_one else [_step(factors=rest)])
    return _case("hub_cap_257" if by_one else "hub_cap_overflow", "g2o", (8, 8), steps, hub_deg=2, tune="hub_deg=2", seed=15)


# ---- GTSAM semantics ---------------------------------------------------------------------------------------------------------
def case_mixed_in_place():
    """6 key frames, 1 plane, 2 points with between / plane / reprojection factors and a pose prior; in place: key frames, a new plane
    and a new point (phantom slots of kind 1 and 2), a point prior and a second pose prior (nothing else: the prior re-upload alone),
    factors to the old and the new landmarks"""
    P, PL, PT = (POSE, False), (PLANE, False), (POINT, False)
    s0 = _step([P] * 6 + [PL, PT, PT],
               [(a, b, BETWEEN) for a, b, _ in _lookback_pairs(1, 6, 2)] + [(k, 6, PLANEF) for k in (0, 2, 4, 5)] +
               [(k, 7, REPROJ) for k in (0, 1, 3)] + [(k, 8, REPROJ) for k in (2, 4, 5)], [0])
    s1 = _step([P, P], [(5, 9, BETWEEN), (4, 9, BETWEEN), (9, 10, BETWEEN), (5, 10, BETWEEN), (9, 6, PLANEF), (9, 7, REPROJ), (10, 8, REPROJ)])
    s2 = _step([PL, PT], [(3, 11, PLANEF), (5, 11, PLANEF), (10, 11, PLANEF), (5, 12, REPROJ), (9, 12, REPROJ), (10, 12, REPROJ)])
    s3 = _step(priors=[12, 4])
    s4 = _step([P], [(10, 13, BETWEEN), (9, 13, BETWEEN), (13, 6, PLANEF), (13, 11, PLANEF), (13, 7, REPROJ), (13, 12, REPROJ)])
    return _case("mixed_in_place", "gtsam", (12, 24), [s0, s1, s2, s3, s4], seed=21)


def _landmark_hub(name, lm_kind, f_kind, targets, seed):
    """8 key frames that all observe one landmark (variable 8); new key frames observe it until its degree is targets[0], targets[1];
    repeated factors on the existing (pose, landmark) pairs -- duplicate groups -- take it to the later targets"""
    s0 = _step([(POSE, False)] * 8 + [(lm_kind, False)], [(k - 1, k, BETWEEN) for k in range(1, 8)] + [(k, 8, f_kind) for k in range(8)],
               [0] + ([8] if lm_kind == POINT else []))
    steps, n, deg, last = [s0], 9, 8, 7
    for target in targets[:2]:
        vs, fs = [], []
        while deg < target:
            vs.append((POSE, False)); fs += [(last, n, BETWEEN), (n, 8, f_kind)]
            last = n; n += 1; deg += 1
        steps.append(_step(vs, fs))
    cams = [k for k in range(n) if k != 8]
    t = 0
    for target in targets[2:]:
        fs = []
        while deg < target:
            fs.append((cams[t % len(cams)], 8, f_kind)); t += 1; deg += 1
        steps.append(_step(factors=fs))
    return _case(name, "gtsam", (96, 128), steps, seed=seed)


def case_plane_hub():
    """(the C-ABI has no prior on a plane: the prior of a hub -- lane 0 of slice 0 only -- is pinned by the point hub)"""
    return _landmark_hub("plane_hub", PLANE, PLANEF, (64, 65, 512, 513), 22)


def case_point_hub():
    """the point carries a prior; beyond the degree 65 the issue asks for, 512 / 513 as for the plane: a prior on a multi-slice hub"""
    return _landmark_hub("point_hub", POINT, REPROJ, (64, 65, 512, 513), 23)


def case_masked_then_not():
    """40 poses of priors and between factors (look-back 3), updates at threshold 0.02: built at 34, three updates with a new pose each
    (maskable), one with a new pose and a duplicate between factor on the old pair (20, 21) (no longer maskable), two more"""
    s0 = _step([(POSE, False)] * 34, [(a, b, BETWEEN) for a, b, _ in _lookback_pairs(1, 34, 3)], [0])
    steps = [s0]
    for k in range(34, 40):
        steps.append(_step([(POSE, False)], [(a, b, BETWEEN) for a, b, _ in _lookback_pairs(k, k + 1, 3)] + ([(20, 21, BETWEEN)] if k == 37 else [])))
    return _case("masked_then_not", "gtsam", (16, 16), steps, thr=0.02, linearize_every_step=False, seed=24)


INPROC_CASES = [case_dup_in_place, lambda: case_dup_in_place(twin=True), case_hub_by_new_vertices, case_slices_by_duplicates,
                case_mixed_in_place, case_plane_hub, case_point_hub]
HUB2_CASES = [lambda: case_dup_in_place(hub_deg=2), lambda: case_dup_in_place(twin=True, hub_deg=2), case_chain_hub2,
              lambda: case_hub_cap(False), lambda: case_hub_cap(True)]
MASKED_CASES = [case_masked_then_not]


def all_cases():
    return {c["name"]: c for c in (f() for f in INPROC_CASES + HUB2_CASES + MASKED_CASES)}


# ---- the ledger --------------------------------------------------------------------------------------------------------------
def hub_entries(d, T):
    return 0 if d <= T else min(HUB_MAX_SLICES, -(-d // HUB_SLICE))


def _choose_hub_deg(deg, forced):
    if forced:
        return forced
    for T in (64, 128, 256, 512):
        if int((deg > T).sum()) <= HUB_MAX_VARS:
            return T
    return HUB_DEG_MAX


def ledger(case, growth=True):
    """per step: dict(deg, entries, n_hubs, n_hub_vars, n_hub_multi, hub_deg, hub_cap, dup_groups {(a, b): [factor numbers]}, n_dup_groups,
    n_dup_members, n_priors, n_phantom, imu_ncolor, maskable, structure_rebuilt, in_band [per factor of the step: its pair exists in the
    structure or lies in the band of a reserve slot], why (what forced a rebuild)).  growth False: a context that builds from scratch."""
    R, W = case["growth"] if growth else (0, 0)
    kinds, fixed, fac, n_pri = [], [], [], 0
    st, out = None, []                                  # st: the structure as built
    for s, step in enumerate(case["steps"]):
        n_before, e_before = len(kinds), len(fac)
        for kind, fx in step["vars"]:
            kinds.append(kind); fixed.append(bool(fx))
        fac += step["factors"]
        n_pri += len(step["priors"])
        N = len(kinds)
        deg = np.zeros(N, np.int64)
        for i, j, _ in fac:
            deg[i] += 1; deg[j] += 1
        groups = {}
        for e, (i, j, _) in enumerate(fac):
            if i != j and not fixed[i] and not fixed[j]:
                groups.setdefault((min(i, j), max(i, j)), []).append(e)
        dups = {p: m for p, m in groups.items() if len(m) > 1}
        why, in_band = None, []
        if st is None:
            why = "build"
        elif R == 0:
            why = "no reserve"
        else:
            if N > st["N"] + R: why = "reserve exhausted"
            if any(fixed[n_before:]): why = "fixed new variable"
            if len(fac) > st["E_cap"]: why = "edge capacity"
            for i, j, _ in fac[e_before:]:
                a, b = min(i, j), max(i, j)
                ok = i == j or fixed[i] or fixed[j] or (a, b) in st["pairs"] or (b >= st["N"] and b - a <= W)
                in_band.append(bool(ok))
                if not ok: why = "pair outside the structure"
            if why is None and sum(hub_entries(int(d), st["T"]) for d in deg) > st["hub_cap"]:
                why = "hub_cap"
        if why is not None:
            T = _choose_hub_deg(deg, case["hub_deg"])
            st = dict(N=N, T=T, pairs=set(groups), E_cap=len(fac) + (max(EDGE_CAP_EXTRA, len(fac) // 8) if R > 0 else 0),
                      hub_cap=sum(hub_entries(int(d), T) for d in deg) + (HUB_CAP_EXTRA if R > 0 else 0))
        entries = np.array([hub_entries(int(d), st["T"]) for d in deg], np.int64)
        n_hubs = int(entries.sum())
        out.append(dict(deg=deg, entries=entries, n_hubs=n_hubs, n_hub_vars=int((entries > 0).sum()), n_hub_multi=int((entries > 1).sum()),
                        hub_deg=st["T"], hub_cap=st["hub_cap"], dup_groups=dups, n_dup_groups=len(dups),
                        n_dup_members=sum(len(m) for m in dups.values()), n_priors=n_pri, n_phantom=st["N"] + R - N, imu_ncolor=64,
                        maskable=int(case["sem"] == "gtsam" and n_hubs == 0 and len(dups) == 0),
                        structure_rebuilt=int(why is not None), in_band=in_band, why=why))
    return out


CENSUS_KEYS = ("n_hubs", "n_hub_vars", "n_hub_multi", "hub_deg", "hub_cap", "n_dup_groups", "n_dup_members", "n_priors", "n_phantom",
               "imu_ncolor", "maskable", "structure_rebuilt")


# ---- measurements ------------------------------------------------------------------------------------------------------------
def _random_truth(rng, n, spread=3.0):
    out = []
    for _ in range(n):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        ang = rng.uniform(-1.0, 1.0)
        out.append(np.concatenate([rng.normal(size=3) * spread, ax * np.sin(ang / 2), [np.cos(ang / 2)]]))
    return np.array(out)


def realise(case):
    """values (N x 7, as the variables are added), and per factor / prior of the whole run, in the order they are added: meas (7),
    info (21) in the oracle's layout.  g2o: random poses and dense random information, as tests/test_gpu_edgecases.py build();
    GTSAM: a slowly moving camera that keeps every landmark in view, the noise models of tests.util.mixed_graph."""
    rng = np.random.default_rng(case["seed"])
    kinds = [k for st in case["steps"] for k, _ in st["vars"]]
    fixed = [f for st in case["steps"] for _, f in st["vars"]]
    fac = [f for st in case["steps"] for f in st["factors"]]
    pri = [v for st in case["steps"] for v in st["priors"]]
    N = len(kinds)
    values = np.zeros((N, 7)); meas = np.zeros((len(fac), 7)); info = np.zeros((len(fac), 21))
    pmean = np.zeros((len(pri), 7)); pinfo = np.zeros((len(pri), 21))
    if case["sem"] == "g2o":
        truth = _random_truth(rng, N)
        for e, (i, j, _) in enumerate(fac):
            meas[e] = noisy(rng, pose_mul(pose_inv(truth[i]), truth[j]), 0.02, 0.01)
            info[e] = info_ut(random_info(rng))
        values[:] = [truth[v] if fixed[v] else noisy(rng, truth[v], 0.05, 0.015) for v in range(N)]
    else:
        from tests import orc_binding as orc
        truth = np.zeros((N, 7))
        big = case["thr"] < 1.0                          # the ISAM2 case starts far enough for relinearisation waves
        k = 0
        for v in range(N):
            if kinds[v] == POSE:
                w = 0.01 * np.array([np.sin(2.0 * k), np.cos(3.0 * k), np.sin(5.0 * k)])
                t = np.array([0.004 * k, 0.003 * np.sin(k), 0.002 * np.cos(k)]) * (40.0 if big else 1.0)
                truth[v] = np.concatenate([t, w, [np.sqrt(1 - w @ w)]])
                values[v] = noisy(rng, truth[v], 0.02, 0.01)
                if big and 20 <= k < 30:
                    values[v, :3] += rng.normal(size=3) * 0.12
                k += 1
            elif kinds[v] == PLANE:
                n = rng.normal(size=3); n /= np.linalg.norm(n)
                truth[v, :4] = [n[0], n[1], n[2], rng.uniform(2.0, 6.0)]
                values[v, :4] = orc.plane_retract(truth[v, :4], rng.normal(size=3) * 0.05)
            else:
                cam = pose_mul(truth[kinds.index(POSE)], BPS)
                pc = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), rng.uniform(3.0, 5.0)])
                truth[v, :3] = cam[:3] + quat_rot(cam[3:], pc)
                values[v, :3] = truth[v, :3] + rng.normal(size=3) * 0.02
        Wb = info_ut(np.diag([1 / 0.01 ** 2] * 3 + [1 / 0.02 ** 2] * 3))
        for e, (i, j, kind) in enumerate(fac):
            if kind == BETWEEN:
                meas[e] = noisy(rng, pose_mul(pose_inv(truth[i]), truth[j]), 0.01, 0.005); info[e] = Wb
            elif kind == PLANEF:
                meas[e, :4] = orc.plane_retract(orc.plane_transform(truth[j, :4], truth[i]), rng.normal(size=3) * 0.01)
                info[e, :6] = [1e4, 0, 0, 1e4, 0, 1e4]
            else:
                meas[e, :2] = orc.reproj(truth[i], truth[j, :3], np.zeros(2), SR4000_CALIB, BPS, jac=False) + rng.normal(size=2) * 0.5
                info[e, 0] = 1.0
        for q, v in enumerate(pri):
            if kinds[v] == POSE:
                pmean[q] = truth[v]; pinfo[q] = SOFT_PRIOR
            else:
                pmean[q, :3] = truth[v, :3]
                w6 = np.zeros((6, 6)); w6[:3, :3] = np.eye(3) / 0.014 ** 2
                pinfo[q] = info_ut(w6)
    return dict(kinds=np.array(kinds, np.int32), fixed=np.array(fixed, np.uint8), values=values, ei=np.array([f[0] for f in fac], np.int32),
                ej=np.array([f[1] for f in fac], np.int32), fkind=np.array([f[2] for f in fac], np.int32), meas=meas, info=info,
                prior_ids=np.array(pri, np.int32), prior_mean=pmean, prior_info=pinfo)


def counts(case, upto):
    """(variables, factors, priors) after the steps 0 .. upto"""
    st = case["steps"][:upto + 1]
    return sum(len(s["vars"]) for s in st), sum(len(s["factors"]) for s in st), sum(len(s["priors"]) for s in st)


# ---- the run on the device ---------------------------------------------------------------------------------------------------
def _add(gr, G, case, d, values, v0, v1, e0, e1, p0, p1):
    """variables [v0, v1) with the given values, factors [e0, e1), priors [p0, p1), in that order"""
    for v in range(v0, v1):
        if d["kinds"][v] == POSE:
            gr.add_poses(values[v:v + 1], d["fixed"][v:v + 1], ids=[v])
        elif d["kinds"][v] == PLANE:
            gr.add_plane(v, values[v, :4])
        else:
            gr.add_point(v, values[v, :3])
    e = e0
    while e < e1:
        kind = d["fkind"][e]
        if kind in (SE3, BETWEEN):                        # runs of pose-pose factors in one call
            f = e
            while f < e1 and d["fkind"][f] == kind: f += 1
            gr.add_edges(d["ei"][e:f], d["ej"][e:f], d["meas"][e:f], d["info"][e:f],
                         tangent_order=G.FGO_TANGENT_G2O if kind == SE3 else G.FGO_TANGENT_GTSAM)
            e = f
            continue
        if kind == PLANEF:                                # the C-ABI takes the covariance: information diag(1e4)
            gr.add_plane_factor(int(d["ei"][e]), int(d["ej"][e]), d["meas"][e, :4], [1e-4, 0, 0, 1e-4, 0, 1e-4])
        else:
            gr.add_reproj(int(d["ei"][e]), int(d["ej"][e]), d["meas"][e, :2], 1.0)
        e += 1
    for q in range(p0, p1):
        v = int(d["prior_ids"][q])
        if d["kinds"][v] == POSE:
            gr.add_prior(v, d["prior_mean"][q], d["prior_info"][q])
        else:
            gr.add_prior_point(v, d["prior_mean"][q, :3], 0.014)


def drive(case, d=None):
    """runs the case on the device; one record per step: census, the values read back, chi2 / H / b of linearize(dense=True) there,
    the same from a context with growth off that holds the same graph and values from scratch (t_chi2 / t_H / t_b), for an ISAM2
    case the update's figures; the last step also a second linearize() (r_*).  Cases with linearize_every_step False read the
    system after the last step only."""
    import graph_slam_amd as G
    d = d or realise(case)
    gtsam = case["sem"] == "gtsam"
    gr = G.Graph()
    if gtsam:
        gr.isam2_reserve(*case["growth"])
        gr.set_calibration(SR4000_CALIB, BPS)
    else:
        gr.set_growth(*case["growth"])
    recs, done = [], (0, 0, 0)
    for s in range(len(case["steps"])):
        now = counts(case, s)
        _add(gr, G, case, d, d["values"], done[0], now[0], done[1], now[1], done[2], now[2])
        done = now
        rec = {}
        if gtsam:
            st = gr.isam2_update(case["thr"])
            rec["update"] = dict(relin=int(st.reserved[1]), chi0=st.chi2_initial, chi1=st.chi2_final, rebuilt=int(st.structure_rebuilt))
        last = s == len(case["steps"]) - 1
        if case["linearize_every_step"] or last:
            rec["values"] = gr.get_poses()
            rec["chi2"], rec["H"], rec["b"] = gr.linearize(dense=True)
            rec["census"] = gr.linearize_census()
            tw = G.Graph()
            if gtsam:
                tw.isam2_reserve(0)
                tw.set_calibration(SR4000_CALIB, BPS)
            else:
                tw.set_growth(0, 0)
            _add(tw, G, case, d, rec["values"], 0, now[0], 0, now[1], 0, now[2])
            rec["t_chi2"], rec["t_H"], rec["t_b"] = tw.linearize(dense=True)
            rec["t_census"] = tw.linearize_census()
            tw.close()
            if last:
                rec["r_chi2"], rec["r_H"], rec["r_b"] = gr.linearize(dense=True)
        else:
            rec["values"] = gr.get_poses()
            rec["census"] = gr.linearize_census()
        recs.append(rec)
    gr.close()
    return recs
