"""Register and LDS budget of k_panel_tri1 (CPU only: a device-only compile of kernels_factor.hip for gfx950, no GPU).

The kernel is the throughput form of the panel triangle: one wave per panel, 21 f64 MFMA accumulator tiles = 168 registers.  It pays
on the wide levels only while TWO waves share a SIMD (512 registers: 256 each) and eight workgroups the LDS of a CU (160 KB: 20 480 B
each); a form that reaches two waves by spilling to scratch is slower than one wave (profiles/NOTES.md).  The compiler's own
resource remarks (-Rpass-analysis=kernel-resource-usage) are held to that budget."""
import os
import re
import subprocess

import pytest

from graph_slam_amd import build as B

SRC = os.path.join(B.CSRC, "kernels_factor.hip")
# the compile flags of build_libfgo
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-Wall", "-Wno-unused-result", "-fvisibility=hidden", "-DFGO_LOCAL_OPERATORS"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel (mangled name): {remark key: value}} of every kernel in kernels_factor.hip"""
    out = tmp_path_factory.mktemp("tri1_resources") / "kernels_factor.o"
    r = subprocess.run([B._hipcc()] + FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o", str(out)],
                       capture_output=True, text=True, cwd=B.ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    table, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: +(.+?): +(\S+) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = table.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    return table


def test_tri1_fits_two_waves_per_simd_without_scratch(usage):
    names = [k for k in usage if "k_panel_tri1" in k]
    assert len(names) == 1, sorted(usage)
    u = usage[names[0]]
    print("[tri1 resources] %s" % u)
    assert int(u["Occupancy [waves/SIMD]"]) >= 2
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert int(u["VGPRs Spill"]) == 0
    assert int(u["LDS Size [bytes/block]"]) <= 20480
    assert int(u["VGPRs"]) + int(u["AGPRs"]) <= 256
