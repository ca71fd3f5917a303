"""Every table of the symbolic phase, to the bit: `tools/symstats` with FGO_DIGEST=1 prints a digest of every member of `struct Symbolic`
and tests/golden/symbolic_digests.json and ordering_digests.json hold what the commits named in those files gave (tests/symbolic_digest.py: the case list and the
writer).  The member names are read from csrc/fgo_internal.hpp, so a table added later cannot escape the comparison.  The tool also
prints which paths of the nested dissection the order came by: they must not depend on the thread count, and a case that pins one of
those paths must take it.  CPU only."""
import os
import re

import pytest

from tests import symbolic_digest as sd
from tests.util import build_symstats

CASES = sd.cases()
EXEMPT = {"cus"}                                   # an input


def symbolic_members():
    """data members of `struct Symbolic`, in declaration order"""
    text = open(os.path.join(sd.ROOT, "graph_slam_amd", "csrc", "fgo_internal.hpp")).read()
    body = text[text.index("struct Symbolic {"):]
    body = body[body.index("{") + 1:body.index("\n};")]
    names = []
    for line in body.splitlines():
        line = line.split("//")[0].strip()
        if not line or line.startswith("static") or "(" in line:
            continue
        decl = re.sub(r"<[^<>]*>", "", line.rstrip(";"))          # (no nested template arguments in this struct)
        decl = re.sub(r"=[^,]*", "", decl)
        words = decl.replace(",", " ").split()
        assert words[0] in ("std::vector", "IntList", "int", "int64_t"), line
        names += words[1:]
    return names


@pytest.fixture(scope="module")
def golden():
    return sd.load_golden()


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return build_symstats(), sd.write_edge_files(tmp_path_factory.mktemp("symbolic_digest"))


def test_the_header_parser_finds_the_members():
    names = symbolic_members()
    assert len(names) == len(set(names)) and len(names) >= 62
    for n in ("cus", "nb", "perm", "iperm", "op_b", "g2_a", "row_col", "task_cols", "ride_items", "pcol_fchunkn", "acc_start", "nops", "max_col_blocks"):
        assert n in names


def test_the_golden_file_covers_the_cases_and_the_code_that_moves(golden):
    assert len(golden["written_at_commit"]) == 2 and all(re.fullmatch(r"[0-9a-f]{40}", c) for c in golden["written_at_commit"])
    assert sorted(golden["cases"]) == sorted(CASES)
    g = golden["cases"]
    assert g["star"]["digest"]["n_scratch"] > 0                                           # hub pieces
    assert any(c["digest"]["ride_items"][0] > 0 for n, c in g.items() if n.endswith("-world4"))
    assert any(c["digest"]["g2_a"][0] > 0 for c in g.values())
    assert any(c["count"]["leaf_levels"] > 0 for c in g.values())
    assert any(c["count"]["generic_levels"] > 0 for c in g.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_equal_the_golden_digests(golden, tool, name):
    exe, edge_files = tool
    want = golden["cases"][name]
    members = [m for m in symbolic_members() if m not in EXEMPT]
    paths = []
    for threads in sd.THREADS:
        got = sd.run_case(exe, CASES[name], edge_files, threads)
        paths.append(got["path"])
        missing = [m for m in members if m not in got["digest"]]
        assert not missing, "tools/symstats prints no digest of %s" % missing
        assert sorted(want["digest"]) == sorted(members), "the golden file does not hold the members of struct Symbolic"
        differ = [m for m in members if got["digest"][m] != want["digest"][m]]
        assert not differ, "%s, %d host threads: %s differ from the golden digests" % (name, threads, differ)
        assert got["count"] == want["count"]
    assert len(paths[0]) >= 13 and all(p == paths[0] for p in paths), "the paths of the dissection depend on the thread count: %s" % paths
    for path, least in sd.REACHES.get(re.sub(r"-world\d+$", "", name), {}).items():
        assert paths[0][path] >= least, "%s does not take the path it pins: %s = %d" % (name, path, paths[0][path])


def test_the_path_table_names_cases():
    assert set(sd.REACHES) <= set(CASES) and set(sd.EDGE_CASES) <= set(sd.REACHES)
