"""Child runner of tests/test_gpu_growth_forms.py: FGO_TUNE (hub_deg, isam_masked, ...) is read once per process, so the cases
that need an override set run in a fresh process -- this script.  It drives the named cases of tests/growth_forms.py on the device
and prints one JSON record per case: status, per step the census and the ISAM2 update's figures, and the path of an .npz with the
arrays of every step (values, H, b, chi2, the same from the context with growth off, the repeated linearisation of the last step).
It computes no reference: the parent does.

usage: growth_forms_child.py --out DIR --cases a,b,..."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import growth_forms as GF  # noqa: E402

ARRAYS = ("values", "H", "b", "t_H", "t_b", "r_H", "r_b")
SCALARS = ("chi2", "t_chi2", "r_chi2")


def pack(recs):
    """(json-able per-step list, arrays for the .npz)"""
    steps, arrays = [], {}
    for s, rec in enumerate(recs):
        steps.append({k: rec[k] for k in ("census", "t_census", "update") + SCALARS if k in rec})
        for k in ARRAYS:
            if k in rec:
                arrays["s%d_%s" % (s, k)] = rec[k]
    return steps, arrays


def unpack(steps, path):
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    recs = []
    for s, st in enumerate(steps):
        rec = dict(st)
        for k in ARRAYS:
            if "s%d_%s" % (s, k) in arrays:
                rec[k] = arrays["s%d_%s" % (s, k)]
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", required=True)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    cases = GF.all_cases()
    for name in [s for s in a.cases.split(",") if s]:
        t0 = time.time()
        rec = dict(graph=name, status="ok")
        try:
            steps, arrays = pack(GF.drive(cases[name]))
            rec["npz"] = os.path.join(a.out, name + ".npz")
            np.savez(rec["npz"], **arrays)
            rec["steps"] = steps
        except Exception as e:      # a refusal or a HIP error: reported, the parent fails the case
            rec["status"] = "error: %s: %s" % (type(e).__name__, e)
        rec["seconds"] = time.time() - t0
        print("RECORD " + json.dumps(rec), flush=True)
        if rec["status"] != "ok" and "hip" in rec["status"].lower():
            return 3                 # after a device error nothing more runs in this process
    return 0


if __name__ == "__main__":
    sys.exit(main())
