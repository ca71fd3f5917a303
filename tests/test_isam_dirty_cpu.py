"""The host walk of a partial ISAM2 update (graph_slam_amd/csrc/isam_dirty.cpp) against a dense recomputation from its definition:
tools/isam_dirty_check.cpp, a stand-alone program that generates its own cases (the eight-byte scan of the moved flags and its tail,
phantom slots, a chain, a star, two roots, a task of several columns, fixed variables, nothing to do, the full-sweep threshold, IMU
factors, 300 random graphs) and runs several consecutive calls per case on the same flag arrays, which it compares whole -- so an entry
that one call leaves set shows in the next.  CPU only: the GPU tests see the same code only through what an update computes."""
import os
import re
import subprocess

from tests.util import ROOT


def build_isam_dirty_check():
    """tools/isam_dirty_check, built when missing or older than a source it reads (as tests/util.py::build_symstats); returns its path"""
    csrc = os.path.join(ROOT, "graph_slam_amd", "csrc")
    exe = os.path.join(ROOT, "tools", "isam_dirty_check")
    src = [os.path.join(ROOT, "tools", "isam_dirty_check.cpp"), os.path.join(csrc, "isam_dirty.cpp")]
    deps = src + [os.path.join(csrc, "isam_dirty.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-I" + ROOT, "-o", exe] + src, check=True, cwd=os.path.join(ROOT, "tools"))
    return exe


def test_dirty_sets_match_the_definition_over_consecutive_calls():
    out = subprocess.run([build_isam_dirty_check()], capture_output=True, text=True, timeout=120)
    print(out.stdout[-4000:], out.stderr[-2000:])
    assert out.returncode == 0 and "FAIL" not in out.stdout
    m = re.search(r"(\d+) cases, (\d+) calls \((\d+) with an empty dirty set, (\d+) over the full-sweep threshold\), (\d+) failed", out.stdout)
    assert m, out.stdout[-500:]
    cases, calls, empty, full, failed = map(int, m.groups())
    # 6 scan sizes + 8 shaped cases + 300 seeds, at least four calls each; both special returns occur
    assert cases == 314 and calls >= 4 * cases and empty > 0 and full > 0 and failed == 0
