#!/usr/bin/env python3
"""The measured difference between the chain diagnostics of ``include/pgbart_diag.h`` (host build,
``tests/_diag_host.py``) and the independent NumPy / SciPy restatement of the published definitions
(``tests/_diag_numpy.py``: ``rankdata``, ``ndtri``, autocovariances by FFT, ``np.quantile``, ``np.median``): per
transform and output the largest relative difference over the inputs of ``tests/test_diag.py`` (every kind of column at
every shape).  Written to ``profiles/diag_accuracy.json``; the test takes 8 x each figure as its bound.  Runs on the
build box (no GPU).

  python tools/diag_accuracy.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_diag import KINDS, SHAPES, accuracy_inputs, differences  # noqa: E402


def main() -> int:
    diffs = differences()
    n_cols = sum(a.shape[1] for _, _, a in accuracy_inputs())
    out = {"what": "include/pgbart_diag.h (host build): pgb_diag_column against the NumPy / SciPy restatement of "
                   "tests/_diag_numpy.py, the largest relative difference per transform and output; the test's bound is "
                   "8 x the figure",
           "inputs": {"shapes_chains_x_draws": [list(s) for s in SHAPES] + [[4, 1000]], "kinds": list(KINDS), "columns": n_cols},
           "largest_relative_difference": diffs,
           "max": max(max(rows.values()) for rows in diffs.values())}
    path = os.path.join(ROOT, "profiles", "diag_accuracy.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
