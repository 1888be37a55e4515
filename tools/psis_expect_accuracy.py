#!/usr/bin/env python3
"""The measured accuracy of ``pgb_psis_row_expect`` (``include/pgbart_psis.h``, host build:
``tests/_psis_expect_host.py``) against the NumPy / SciPy restatement of the PSIS-weighted expectations
(``tests/_psis_expect_numpy.py``) on the synthetic matrices of ``tests/test_psis_expect.py``: per kind the largest
``|header - restatement| / max(1, |E|)`` over Normal and Poisson functionals on the rows with k <= 0.7 or no fit.
Written to ``profiles/psis_expect_accuracy.json``; the tests take 8 x that figure as their bound.  Runs on the build
box (no GPU).

  python tools/psis_expect_accuracy.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_psis_expect import SIZES, differences  # noqa: E402


def main() -> int:
    cases, worst = [], {"value": 0.0, "pit": 0.0}
    for D in SIZES:
        d = differences(D)
        cases.append({"D": D, "n": d["n"], "rows_left_out": d["left_out"], "max_rel_diff_value": d["value"],
                      "max_rel_diff_pit": d["pit"]})
        for kind in worst:
            worst[kind] = max(worst[kind], d[kind])
    out = {"what": "pgb_psis_row_expect (include/pgbart_psis.h, host build) against tests/_psis_expect_numpy.py on "
                   "tests/test_psis_expect.py's synthetic matrices and functionals, rows with restated k <= 0.7 or no fit; "
                   "|difference| / max(1, |E|); the tests' bound is 8 x max_rel_diff of the kind",
           "max_rel_diff": worst, "cases": cases}
    path = os.path.join(ROOT, "profiles", "psis_expect_accuracy.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
