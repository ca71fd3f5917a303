"""Digests of every table of the symbolic phase (`struct Symbolic`, csrc/fgo_internal.hpp) over a list of graphs and settings:
the case list, the runner and the writer of tests/golden/symbolic_digests.json and tests/golden/ordering_digests.json (the cases that
pin the paths of the nested dissection, REACHES below: one line per case, so that adding cases stays readable in a diff).
tests/test_symbolic_digest_cpu.py compares the tree against those files, case by case and field by field.

    python tests/symbolic_digest.py --write        regenerate both golden files (each records the commit it was written at)

A golden file is written from a tree whose symbolic*.cpp and ordering*.cpp are the committed ones, BEFORE a change that must leave the
order or the tables as they are, and is not edited afterwards.  `tools/symstats` with FGO_DIGEST=1 prints the digests; every run is a fresh
process, because tune() and the settings of the ordering and the symbolic phase are read once per process."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "symbolic_digests.json")
GOLDEN_ORDERING = os.path.join(ROOT, "tests", "golden", "ordering_digests.json")
THREADS = (1, 5)                      # FGO_HOST_THREADS: both must give the one golden entry
WORLDS = (None, 2, 4)                 # FGO_WORLD

# ---- graphs.  Synthetic ones by the tool's own arguments <poses> <look-back> <loops> <leaf> <task work> <chain work>; the others as
# edge files (FGO_EDGES: int64 [n, E, ei[E], ej[E]]; vertex 0 is the fixed pose and takes no part).
SYNTH = {
    "synth600": (("600", "5", "4", "64", "5000", "1000000000"), {}),
    "synth20000": (("20000", "5", "4", "64", "5000", "1000000000"), {}),
    "leaf8": (("3000", "5", "4", "8", "5000", "1000000000"), {}),
    # task work 1: no light sub-trees, every panel width (tests/test_gpu_tri1_two_waves.py)
    "width1": (("300", "5", "4", "64", "1", "1000000000"), {"FGO_SYNTH_SEED": "3"}),
    # The column-group lists (g2_*) are built for levels of 80 000 targets and more (acc2_min = 8000 groups of ten): no graph that a
    # quick test can afford has one, so this case lowers the threshold to levels of 1 000 targets.
    "synth20000-acc2": (("20000", "5", "4", "64", "5000", "1000000000"), {"FGO_TUNE": "acc2_min=100"}),
    # ---- the paths of the nested dissection (csrc/ordering*.cpp) that the graphs above leave alone: they are dissected by index cuts
    # (vertex index = time), are cliques, or fall apart into leaf-sized pieces.  Relabelled at random, or with nd_time=0, a graph with loop
    # closures takes the level-structure cuts.
    "shuffled3000": (("3000", "5", "4", "8", "5000", "1000000000"), {"FGO_SHUFFLE": "1"}),      # level cuts, cover refinement, no cut, a disconnected region
    "shuffled20000": (("20000", "5", "4", "64", "5000", "1000000000"), {"FGO_SHUFFLE": "1"}),   # the same on a deeper top tree
    "levels-starts4": (("3000", "5", "4", "8", "5000", "1000000000"), {"FGO_TUNE": "nd_time=0,nd_starts=4"}),   # third / fourth start; the winner rebuilt by a BFS
    "levels-starts1": (("3000", "5", "4", "8", "5000", "1000000000"), {"FGO_TUNE": "nd_time=0,nd_starts=1"}),
    "levels-nocover": (("3000", "5", "4", "8", "5000", "1000000000"), {"FGO_TUNE": "nd_time=0,nd_cover=0"}),    # the trimmed separator as it is
    "recovered3000": (("3000", "10", "0", "16", "5000", "1000000000"), {"FGO_SHUFFLE": "2"}),   # a band graph relabelled: index cuts under recovered labels
    "time-weight": (("3000", "5", "4", "16", "5000", "1000000000"), {"FGO_TUNE": "nd_time_weight=0.5"}),        # the weighted balance window
    "time-keep1": (("3000", "5", "4", "16", "5000", "1000000000"), {"FGO_TUNE": "nd_time_keep=1"}),             # one candidate cut instead of eight
}
EDGE_ARGS = ("600", "5", "4", "64", "5000", "1000000000")
# The star's hub target collects 6 000 early updates, above the default hub threshold (ride_hub = 4096): hub pieces with the defaults.
# (graph -> environment; EDGE_CASES: case -> (graph, leaf, environment) for a leaf size or settings of its own)
EDGE_GRAPHS = {"star": {}, "complete120": {}, "bundle": {}}
EDGE_CASES = {
    "torus40": ("torus40", "16", {}),                                  # level cuts on a mesh: the nd_min_side penalty decides
    "islands": ("islands", "8", {}),                                   # index cuts that nothing crosses
    "islands-levels": ("islands", "8", {"FGO_TUNE": "nd_time=0"}),     # a disconnected region: large components and binned small ones
    "clique400": ("clique400", "64", {}),                              # a set above 384 vertices goes through the leaf ordering as it is
}
# What each case of the nested dissection is there for: path counter (csrc/fgo_internal.hpp OrderingPath) -> the least it must show
REACHES = {
    "shuffled3000": {"level_cuts": 1, "level_cuts_cover": 1, "no_cut": 1, "disconnected": 1, "restore_copy": 1},
    "shuffled20000": {"level_cuts": 1, "level_cuts_cover": 1, "disconnected": 1, "restore_copy": 1},
    "levels-starts4": {"level_cuts": 1, "restore_bfs": 1},
    "levels-starts1": {"level_cuts": 1},
    "levels-nocover": {"level_cuts": 1},
    "recovered3000": {"index_cuts": 1, "time_mode": 2},
    "time-weight": {"index_cuts": 1},
    "time-keep1": {"index_cuts": 1},
    "torus40": {"level_cuts": 1},
    "islands": {"index_cuts_clean": 1},
    "islands-levels": {"level_cuts": 1, "disconnected": 1},
    "clique400": {"leaf_large": 1},
}
VARIANTS = {                           # on synth600, synth20000 and the star
    "no_panels": {"FGO_NO_PANELS": "1"},
    "ride0": {"FGO_TUNE": "ride=0"},
    "merge_multi0": {"FGO_TUNE": "merge_multi=0"},
    "merge_by_level0": {"FGO_TUNE": "merge_by_level=0"},
    "analyse_only": {"FGO_ANALYSE_ONLY": "1"},
}
VARIANT_GRAPHS = ("synth600", "synth20000", "star")


def star_edges():
    """hub 1 tied to vertices 2 .. 6001, plus a chain along the leaves"""
    leaves = np.arange(2, 6002, dtype=np.int64)
    ei = np.concatenate([np.ones(len(leaves), np.int64), leaves[:-1]])
    ej = np.concatenate([leaves, leaves[1:]])
    return 6002, ei, ej


def complete_edges(n=120):
    i, j = np.triu_indices(n, 1)
    return n + 1, (i + 1).astype(np.int64), (j + 1).astype(np.int64)


def bundle_edges(cameras=40, points=3000, views=4, seed=12345):
    """bundle-like bipartite graph: chained cameras 1 .. 40, points behind them, each seen by `views` cameras of a window of eight
    (a linear congruential generator of our own: the graph must not depend on the numpy version)"""
    state = seed
    ei = list(range(1, cameras))
    ej = list(range(2, cameras + 1))
    for p in range(points):
        seen = set()
        state = (state * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        first = (state >> 33) % (cameras - 7)
        while len(seen) < views:
            state = (state * 6364136223846793005 + 1442695040888963407) % (1 << 64)
            seen.add(first + (state >> 33) % 8)
        for c in sorted(seen):
            ei.append(1 + c)
            ej.append(1 + cameras + p)
    return 1 + cameras + points, np.array(ei, np.int64), np.array(ej, np.int64)


def torus_edges(side=40):
    """side x side grid, wrapped around both ways"""
    v = np.arange(side * side, dtype=np.int64)
    r, c = v // side, v % side
    right, down = r * side + (c + 1) % side, ((r + 1) % side) * side + c
    return side * side + 1, np.concatenate([v, v]) + 1, np.concatenate([right, down]) + 1


def islands_edges(bands=(700, 300, 40), pairs=30, singles=50):
    """band graphs (edges i - i+1 and i - i+3) one after the other, then isolated pairs, then isolated vertices"""
    ei, ej, first = [], [], 1
    for m in bands:
        for d in (1, 3):
            ei += range(first, first + m - d)
            ej += range(first + d, first + m)
        first += m
    ei += range(first, first + 2 * pairs, 2)
    ej += range(first + 1, first + 2 * pairs, 2)
    return first + 2 * pairs + singles, np.array(ei, np.int64), np.array(ej, np.int64)


def write_edge_files(directory):
    """-> {graph name: path}"""
    paths = {}
    for name, make in (("star", star_edges), ("complete120", complete_edges), ("bundle", bundle_edges), ("torus40", torus_edges),
                       ("islands", islands_edges), ("clique400", lambda: complete_edges(400))):
        n, ei, ej = make()
        paths[name] = os.path.join(str(directory), name + ".edges")
        np.concatenate([np.array([n, len(ei)], np.int64), ei, ej]).tofile(paths[name])
    return paths


def cases():
    """-> {case name: (graph name, arguments, environment without FGO_EDGES / FGO_HOST_THREADS)}"""
    graphs = dict(SYNTH)
    graphs.update({g: (EDGE_ARGS, env) for g, env in EDGE_GRAPHS.items()})
    base = {g: (g, a, dict(e)) for g, (a, e) in graphs.items()}
    base.update({c: (g, EDGE_ARGS[:3] + (leaf,) + EDGE_ARGS[4:], dict(e)) for c, (g, leaf, e) in EDGE_CASES.items()})
    for g in VARIANT_GRAPHS:
        for v, venv in VARIANTS.items():
            args, env = graphs[g]
            env = dict(env)
            for k, val in venv.items():
                env[k] = env[k] + "," + val if k == "FGO_TUNE" and k in env else val
            base["%s-%s" % (g, v)] = (g, args, env)
    out = {}
    for name, (g, args, env) in base.items():
        for w in WORLDS:
            out[name if w is None else "%s-world%d" % (name, w)] = (g, args, dict(env) if w is None else dict(env, FGO_WORLD=str(w)))
    return out


def run_case(exe, case, edge_files, threads):
    """-> {"digest": {member: value | [elements, fnv64]}, "count": {name: n}, "path": {name: n}} of one fresh process ("path": which paths
    of the nested dissection the order came by -- not part of the golden file)"""
    graph, args, env = case
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("FGO_")}, FGO_DIGEST="1", FGO_HOST_THREADS=str(threads), **env)
    if graph in edge_files:
        env["FGO_EDGES"] = edge_files[graph]
    out = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    res = {"digest": {}, "count": {}, "path": {}}
    for line in out.stdout.splitlines():
        w = line.split()
        if w and w[0] == "digest":
            res["digest"][w[1]] = int(w[2]) if len(w) == 3 else [int(w[2]), w[3]]
        elif w and w[0] in ("count", "path"):
            res[w[0]][w[1]] = int(w[2])
    return res


def in_ordering_file(name):
    """a case that pins a path of the nested dissection (any world) lives in GOLDEN_ORDERING"""
    return name.split("-world")[0] in REACHES


def load_golden():
    """-> {"written_at_commit": [commit per file], "cases": {case name: entry}} of both files"""
    both = {"written_at_commit": [], "cases": {}}
    for path in (GOLDEN, GOLDEN_ORDERING):
        with open(path) as f:
            g = json.load(f)
        assert not set(g["cases"]) & set(both["cases"]) and all(in_ordering_file(n) == (path == GOLDEN_ORDERING) for n in g["cases"]), path
        both["written_at_commit"].append(g["written_at_commit"])
        both["cases"].update(g["cases"])
    return both


def main():
    import tempfile
    from tests.util import build_symstats
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    src = os.path.join("graph_slam_amd", "csrc")
    dirty = subprocess.run(["git", "status", "--porcelain", "--", src], capture_output=True, text=True, cwd=ROOT, check=True).stdout
    dirty = [l for l in dirty.splitlines() if "symbolic" in l or "ordering" in l]
    if dirty:
        sys.exit("the ordering or the symbolic phase differs from the commit: %s" % dirty)
    commit = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, cwd=ROOT, check=True).stdout.strip()
    exe = build_symstats()
    golden = {"cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        files = write_edge_files(tmp)
        for name, case in cases().items():
            first = run_case(exe, case, files, THREADS[0])
            for t in THREADS[1:]:
                assert run_case(exe, case, files, t) == first, (name, t)
            del first["path"]
            golden["cases"][name] = first
            print(name, "levels", first["digest"]["level_ptr"][0] - 1, "scratch", first["digest"]["n_scratch"], "ride items", first["digest"]["ride_items"][0],
                  "g2_a", first["digest"]["g2_a"][0], first["count"])
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump({"written_at_commit": commit, "cases": {n: c for n, c in golden["cases"].items() if not in_ordering_file(n)}}, f, indent=0, sort_keys=True)
        f.write("\n")
    with open(GOLDEN_ORDERING, "w") as f:
        lines = ["%s: %s" % (json.dumps(n), json.dumps(c, sort_keys=True)) for n, c in sorted(golden["cases"].items()) if in_ordering_file(n)]
        f.write('{"written_at_commit": "%s", "cases": {\n%s\n}}\n' % (commit, ",\n".join(lines)))


if __name__ == "__main__":
    main()
