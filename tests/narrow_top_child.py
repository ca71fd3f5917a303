"""Child runner of tests/test_gpu_narrow_top.py: tests/launch_forms_child.py with the graph list of that test (FGO_TUNE is read once
per process, so every override set runs in a fresh process).  Records and options are those of launch_forms_child.

usage: narrow_top_child.py --out DIR [--dense] [--graphs a,b,...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import launch_forms_child as base  # noqa: E402

# complete graphs: pose 0 is fixed, so complete(n) has n - 1 free poses, eliminated as ONE chain of columns.  FGO_TASK_WORK=1 leaves no
# light sub-tree (no leaf task), so the chain is cut into panels of 16 columns from the bottom and the root panel takes the remainder.
COMPLETE = [209, 210, 35, 36, 40, 41]
GRAPHS = [("complete%d" % n, (lambda n=n: base.complete(n)), {"FGO_TASK_WORK": "1"}, "solve") for n in COMPLETE]
# panels of every width 1 .. 16 WITH rows below them (the complete graphs have their only short panel at the root, without rows)
GRAPHS.append(("synth150_w1", lambda: base.synth(150, 5, 4, 250), {"FGO_TASK_WORK": "1"}, "solve"))

if __name__ == "__main__":
    base.GRAPHS = GRAPHS
    sys.exit(base.main())
