"""Child runner of tests/test_gpu_tri1_two_waves.py: tests/launch_forms_child.py with the graph list of that test (FGO_TUNE is read
once per process, so the override set that sends every panel through k_panel_tri1 runs in a fresh process).  Records and options are
those of launch_forms_child.

usage: tri1_two_waves_child.py --out DIR [--dense] [--graphs a,b,...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import launch_forms_child as base  # noqa: E402
from tests.narrow_top_child import COMPLETE  # noqa: E402

# (poses, look-back, loop closures, seed) of synth_manhattan3d; with FGO_TASK_WORK=1 every level is a panel level
SYNTH = {"synth300_w1": (300, 5, 4, 3), "synth500_w1": (500, 5, 4, 6)}
W1 = {"FGO_TASK_WORK": "1"}
GRAPHS = [(name, (lambda a=a: base.synth(*a)), W1, "solve") for name, a in SYNTH.items()]
GRAPHS += [("complete%d" % n, (lambda n=n: base.complete(n)), W1, "solve") for n in COMPLETE]
GRAPHS.append(("negdef_w1", base.negdef, W1, "negdef"))

if __name__ == "__main__":
    base.GRAPHS = GRAPHS
    sys.exit(base.main())
