#!/usr/bin/env python3
"""The measured accuracy of ``include/pgbart_psis.h`` (host build, ``tests/_psis_host.py``) against the NumPy / SciPy
restatement of PSIS (``tests/_psis_numpy.py``) on the synthetic matrices of ``tests/test_psis.py``: the largest
absolute difference over ``pareto_k_i`` and ``elpd_loo_i`` on the rows with k <= 0.7.  Written to
``profiles/psis_accuracy.json``; ``tests/test_psis.py`` and ``tests/test_psis_gpu.py`` take 8 x that figure as their
bound.  Runs on the build box (no GPU).

  python tools/psis_accuracy.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _psis_host as host  # noqa: E402
import _psis_numpy as ref  # noqa: E402
from test_psis import synthetic  # noqa: E402


def main() -> int:
    cases, worst = [], 0.0
    for D in (400, 1000, 4000):
        ll = synthetic(D)
        M = ref.tail_length(D)
        e, k = host.psis(ll, M)
        er, kr, T = ref.psis_matrix(ll)
        ok = kr <= 0.7
        dk, de = float(np.max(np.abs(k - kr)[ok])), float(np.max(np.abs(e - er)[ok]))
        cases.append({"D": D, "n": int(ll.shape[1]), "tail_len": M, "rows_left_out": int((~ok).sum()),
                      "max_k_restated": float(kr.max()), "max_abs_diff_k": dk, "max_abs_diff_elpd": de})
        worst = max(worst, dk, de)
    out = {"what": "include/pgbart_psis.h (host build) against tests/_psis_numpy.py on tests/test_psis.py's synthetic "
                   "matrices, rows with restated k <= 0.7; the tests' bound is 8 x max_abs_diff",
           "max_abs_diff": worst, "cases": cases}
    path = os.path.join(ROOT, "profiles", "psis_accuracy.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
