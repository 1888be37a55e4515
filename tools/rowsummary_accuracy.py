#!/usr/bin/env python3
"""The measured accuracy of the transforms of ``include/pgbart_rowsummary.h`` (host build,
``tests/_rowsummary_host.py``) against NumPy / SciPy on x in [-30, 30]: per transform the largest ``|header / libm - 1|``
of exp (``np.exp``), logistic (``scipy.special.expit``) and probit (``scipy.special.ndtr``) over the inputs of
``tests/test_rowsummary.py``.  Written to ``profiles/rowsummary_accuracy.json``; the test takes 8 x each figure as its
bound.  Runs on the build box (no GPU).

  python tools/rowsummary_accuracy.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_rowsummary import transform_differences, transform_inputs  # noqa: E402


def main() -> int:
    diffs = transform_differences()
    x = transform_inputs()
    out = {"what": "include/pgbart_rowsummary.h (host build): pgb_rowsum_value against np.exp, scipy.special.expit and "
                   "scipy.special.ndtr, the largest |header / libm - 1| per transform; the test's bound is 8 x the figure",
           "inputs": {"n": int(x.size), "min": float(x.min()), "max": float(x.max())},
           "max_rel_diff": diffs, "max": max(diffs.values())}
    path = os.path.join(ROOT, "profiles", "rowsummary_accuracy.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
