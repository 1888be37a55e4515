#!/usr/bin/env python3
"""The measured accuracy of the Shapley attributions of ``include/pgbart_shap.h`` (host build, ``tests/_shap_host.py``)
against exact ``Fraction`` arithmetic: the largest ``|host - exact| / M`` over every attribution, ``M`` being the sum of
``|coef|`` over the leaf terms of the entry's forest (it bounds every ``|phi_j|``).

* the hand-built pools of ``tests/test_shap.py`` (p <= 5): exact = the definition, all ``2^p`` coalitions through
  ``_predict_exact.walk`` -- and the exact leaf-wise form must agree with it, attribution for attribution;
* chain trees over 16, 32 and 64 distinct columns (left and right chains, with and without linear leaves): ``2^p``
  coalitions cannot be enumerated, exact = the leaf-wise form in ``Fraction`` (the one just held to the definition).

Every entry must also lie below the crude ceiling ``(5000 + T) 2^-53`` (``T`` leaf terms).  Written to
``profiles/shap_accuracy.json``; the tests take 8 x the figure x M as their tolerance.  Runs on the build box (no GPU).

  python tools/shap_accuracy.py
"""
import json
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _shap_host as host  # noqa: E402

U = Fraction(1, 2 ** 53)
CHAINS = [(16, "left", ()), (16, "right", (0, 15)), (32, "left", (3,)), (32, "right", ()), (64, "left", ()), (64, "right", (63,))]


def worst(got, exact, M, T):
    """``(max |got - exact| / M, the entry's T, min T, entries, non-zero exact entries)``; asserts the ceiling."""
    D, K, p, n = got.shape
    top, top_t, nz = Fraction(0), 0, 0
    for d in range(D):
        for k in range(K):
            for i in range(n):
                m = Fraction(float(M[d, k, i]))
                for j in range(p):
                    err = abs(Fraction(float(got[d, k, j, i])) - exact[d, k, j, i])
                    nz += exact[d, k, j, i] != 0
                    if err == 0:
                        continue
                    assert m > 0, (d, k, j, i)
                    assert err / m < (5000 + int(T[d, i])) * U, (d, k, j, i, float(err / m))
                    if err / m > top:
                        top, top_t = err / m, int(T[d, i])
    return float(top), top_t, int(T.min()), int(got.size), int(nz)


def main() -> int:
    cases = {}
    for name, pool, fidx, X in host.pools():
        got, base = host.rows(pool, fidx, X)
        phi, b, _ = host.brute_force(pool, fidx, X)
        lw, lb, _, _ = host.restated(pool, fidx, X, Fraction)
        assert np.all(lw == phi) and np.all(lb == b), name  # the leaf-wise form IS the definition
        M, T = host.magnitude(pool, fidx, X)
        fig, t, tmin, n, nz = worst(got, phi, M, T)
        cases[name] = {"max_err_over_M": fig, "T_at_max": t, "T_min": tmin, "attributions": n, "nonzero": nz,
                       "reference": "all 2^p coalitions"}
    for depth, side, linear in CHAINS:
        pool, fidx, rng = host.chain_pool(depth, K=1, side=side, linear=linear)
        X = host.chain_rows(pool, depth, depth + 2, rng, n=3)
        got, base = host.rows(pool, fidx, X)
        lw, lb, _, _ = host.restated(pool, fidx, X, Fraction)
        M, T = host.magnitude(pool, fidx, X)
        fig, t, tmin, n, nz = worst(got, lw, M, T)
        cases[f"chain-{depth}-{side}{'-linear' if linear else ''}"] = {
            "max_err_over_M": fig, "T_at_max": t, "T_min": tmin, "attributions": n, "nonzero": nz,
            "reference": "leaf-wise form in Fraction"}
    out = {"what": "include/pgbart_shap.h (host build) against exact Fraction arithmetic: the largest |host - exact| / M "
                   "over every attribution, M = the sum of |coef| over the entry's leaf terms; the tests' tolerance is "
                   "8 x max x M; every entry lies below (5000 + T) 2^-53",
           "cases": cases, "max": max(c["max_err_over_M"] for c in cases.values()),
           "T_min": min(c["T_min"] for c in cases.values())}
    path = os.path.join(ROOT, "profiles", "shap_accuracy.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
