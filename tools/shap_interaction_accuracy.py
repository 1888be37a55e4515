#!/usr/bin/env python3
"""The measured accuracy of the SHAP interaction values of ``include/pgbart_shap_interaction.h`` (host build,
``tests/_shap_interaction_host.py``) against exact ``Fraction`` arithmetic: the largest ``|host - exact| / M`` over every
entry of every matrix, ``M`` being ``_shap_host.magnitude``'s sum of ``|coef|`` over the leaf terms of the entry's forest.

* the hand-built pools of ``_shap_host.pools()`` (p <= 5): exact = the definition, all ``2^p`` coalitions through
  ``_predict_exact.walk`` -- and the exact leaf-wise form must agree with it, entry for entry;
* chain trees over 16 and 32 distinct columns (left and right chains, with and without linear leaves on the path):
  ``2^p`` coalitions cannot be enumerated, exact = the leaf-wise form in ``Fraction`` (the one just held to the
  definition).

Every entry must also lie below the crude ceiling ``(5000 + 17 T) 2^-53`` of ``tests/test_shap_interaction.py`` (``T``
leaf terms).  Written to ``profiles/shap_interaction_accuracy.json``; the tests take 8 x the figure x M as their
tolerance.  Needs no GPU.

  python tools/shap_interaction_accuracy.py
"""
import json
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _shap_host as host  # noqa: E402
import _shap_interaction_host as hx  # noqa: E402

U = Fraction(1, 2 ** 53)
CHAINS = [(16, "left", ()), (16, "right", (0, 15)), (32, "left", (3,)), (32, "right", ())]


def worst(got, exact, M, T):
    """``(max |got - exact| / M, the entry's T, min T, entries, non-zero exact entries)``; asserts the ceiling."""
    D, K, p, _, n = got.shape
    top, top_t, nz = Fraction(0), 0, 0
    for d in range(D):
        for k in range(K):
            for i in range(n):
                m = Fraction(float(M[d, k, i]))
                for a in range(p):
                    for b in range(p):
                        err = abs(Fraction(float(got[d, k, a, b, i])) - exact[d, k, a, b, i])
                        nz += exact[d, k, a, b, i] != 0
                        if err == 0:
                            continue
                        assert m > 0, (d, k, a, b, i)
                        assert err / m < (5000 + 17 * int(T[d, i])) * U, (d, k, a, b, i, float(err / m))
                        if err / m > top:
                            top, top_t = err / m, int(T[d, i])
    return float(top), top_t, int(T.min()), int(got.size), int(nz)


def main() -> int:
    cases = {}
    for name, pool, fidx, X in host.pools():
        got, _ = hx.rows(pool, fidx, X)
        Phi, _, _, _ = hx.brute_force(pool, fidx, X)
        assert np.all(hx.restated(pool, fidx, X, Fraction) == Phi), name  # the leaf-wise form IS the definition
        M, T = host.magnitude(pool, fidx, X)
        fig, t, tmin, n, nz = worst(got, Phi, M, T)
        cases[name] = {"max_err_over_M": fig, "T_at_max": t, "T_min": tmin, "entries": n, "nonzero": nz,
                       "reference": "all 2^p coalitions"}
    for depth, side, linear in CHAINS:
        pool, fidx, rng = host.chain_pool(depth, K=1, side=side, linear=linear)
        X = host.chain_rows(pool, depth, depth + 2, rng, n=3)
        got, _ = hx.rows(pool, fidx, X)
        lw = hx.restated(pool, fidx, X, Fraction)
        M, T = host.magnitude(pool, fidx, X)
        fig, t, tmin, n, nz = worst(got, lw, M, T)
        cases[f"chain-{depth}-{side}{'-linear' if linear else ''}"] = {
            "max_err_over_M": fig, "T_at_max": t, "T_min": tmin, "entries": n, "nonzero": nz,
            "reference": "leaf-wise form in Fraction"}
    out = {"what": "include/pgbart_shap_interaction.h (host build) against exact Fraction arithmetic: the largest "
                   "|host - exact| / M over every entry, M = the sum of |coef| over the entry's leaf terms; the tests' "
                   "tolerance is 8 x max x M; every entry lies below (5000 + 17 T) 2^-53",
           "cases": cases, "max": max(c["max_err_over_M"] for c in cases.values()),
           "T_min": min(c["T_min"] for c in cases.values())}
    path = os.path.join(ROOT, "profiles", "shap_interaction_accuracy.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
