#!/usr/bin/env python3
"""ms per call of ``individual_conditional_expectation`` -- one fused ``pgb_predict_ice`` call per sampler -- against
the probe-matrix loop it replaced, on one GPU.

The public call is timed from host arrays to host results, after warming, median of ``--reps``, at two shapes:

* ``plot``   n = 1000, p = 10, m = 50, 500 stored draws, all columns, 30 instances, 100 samples (the reference's
             defaults on a plot-sized fit),
* ``large``  cfg2-shaped: 100 k x 50, m = 200, 1000 draws, ``var_idx=[0, 1]``, 4 instances, 100 samples.

THE BASELINE is the same call of the package found in ``--baseline-root DIR`` (a built checkout of the parent commit),
in a process of its own, two legs (``ice`` / ``ice_again``) so that its run-to-run spread is on record.  Required: the
new call is below the baseline at both shapes by more than the baseline's own spread.

Also recorded, per shape: ``k_ice`` alone between two HIP events (``_timing.walk_timing()``, ``pgb_walk_kernel_ms``) as tree
traversals/s, next to ``k_predict``'s rate for the same traversal count in the same process: one curve's probe matrix,
resident, predicted for as many draws as the sweep has curves x samples.

Writes ``profiles/ice_timing.json`` (``--out``) and prints it as one JSON line.

  python tools/ice_timing.py [--reps 5] [--shapes plot,large] [--baseline-root DIR] [--out FILE]
"""

from __future__ import annotations

import ctypes as C
import json
import os
import sys

import _timing

SHAPES = {
    "plot": dict(n=1000, p=10, m=50, draws=500, var_idx=None, instances=30, samples=100),
    "large": dict(n=100_000, p=50, m=200, draws=1000, var_idx=[0, 1], instances=4, samples=100),
}


LEGS = ("ice", "ice_again")


def _call(op, X, shape):
    from pymc_bart_amd import individual_conditional_expectation

    return individual_conditional_expectation(op, X, var_idx=shape["var_idx"], instances=shape["instances"],
                                              samples=shape["samples"], random_seed=3)


def baseline(names, reps) -> dict:
    """The public call of the package on sys.path, timed twice per round, at every shape."""
    import torch  # noqa: F401

    import pymc_bart_amd

    # (the parent commit has no pymc_bart_amd/ice.py: the mark that the baseline's package is not this tree's)
    out = {"has_ice_module": os.path.exists(os.path.join(os.path.dirname(pymc_bart_amd.__file__), "ice.py"))}
    for name in names:
        shape = SHAPES[name]
        f = _timing.fit(shape)
        out[name] = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, lambda: _call(f.op, f.X, shape)), reps))
        out[name]["chain_seconds"] = round(f.seconds, 1)
    return out


def _kernel_rates(op, X, shape, reps):
    """``k_ice`` alone on the shape's whole sweep, and ``k_predict`` alone on one curve's probe matrix for all the
    sweep's picks (the same number of tree traversals in one launch), both as traversals/s."""
    import numpy as np

    from pymc_bart_amd.utils import _get_posterior_sampler

    s = _get_posterior_sampler(op)
    part = s._chain_samplers[0]
    lib = part._get_backend().lib
    ms_of = lib.lib.pgb_walk_kernel_ms
    ms_of.argtypes = [C.POINTER(C.c_double)]
    n, p = X.shape
    cols = list(range(p)) if shape["var_idx"] is None else shape["var_idx"]
    rng = np.random.default_rng(3)
    chosen = rng.choice(n, replace=False, size=shape["instances"])
    picks = rng.integers(0, s.n_draws, size=(len(cols), len(chosen), shape["samples"]))
    rows = part.resident_rows(X)
    probe = X.copy()
    probe[:, [v for v in range(p) if v != cols[0]]] = X[chosen[0], [v for v in range(p) if v != cols[0]]]
    probe_rows = part.resident_rows(probe)
    with _timing.walk_timing():
        ice, pred = [], []
        for _ in range(reps + 1):
            v = C.c_double(-1.0)
            s.ice_mean(rows, X[chosen], cols, picks)
            ms_of(C.byref(v))
            ice.append(v.value)
            part.sample_posterior(probe_rows, picks.ravel().tolist(), None)
            ms_of(C.byref(v))
            pred.append(v.value)
    ice_ms, pred_ms = float(np.median(ice[1:])), float(np.median(pred[1:]))
    trav_ice = float(picks.size) * n * op.m
    trav_pred = trav_ice
    return {"k_ice_ms": round(ice_ms, 4), "k_ice_traversals": trav_ice,
            "k_ice_gtraversals_per_s": round(trav_ice / ice_ms / 1e6, 2),
            "k_predict_ms": round(pred_ms, 4), "k_predict_traversals": trav_pred,
            "k_predict_gtraversals_per_s": round(trav_pred / pred_ms / 1e6, 2),
            "k_predict_launch": "one curve's probe matrix, resident, every pick of the sweep as a draw"}


def main(argv=None) -> int:
    args = _timing.base_parser("ice_timing.json", "plot,large", baseline=True).parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        _timing.print_baseline(baseline(names, args.reps))
        return 0
    import torch  # noqa: F401

    line = {"metric": "ms_per_call", "reps": args.reps, "shapes": {}}
    new = {}
    for name in names:
        shape = SHAPES[name]
        f = _timing.fit(shape)
        X, op = f.X, f.op
        t = _timing.time_legs({"ice": lambda: _call(op, X, shape)}, args.reps)["ice"]
        new[name] = {"shape": dict(shape, chain_seconds=round(f.seconds, 1)), **t,
                     "kernels_alone": _kernel_rates(op, X, shape, args.reps)}
        print(f"[ice_timing] {name}: {json.dumps(new[name])}", file=sys.stderr, flush=True)
        del X, op, f
    if args.baseline_root:
        base = _timing.run_baseline(__file__, args.baseline_root, ["--reps", str(args.reps), "--shapes", ",".join(names)])
        where = "a checkout of the parent commit, in a process of its own"
    else:
        base, where = None, None
    ok = {}
    for name in names:
        row = new[name]
        if base is not None:
            b = base[name]
            bm = b["median_ms"]
            spread = _timing.spread(b, LEGS)
            row["baseline"] = {"measured_on": where, "has_ice_module": base["has_ice_module"], **b}
            row["baseline_spread_ms"] = round(spread, 3)
            row["speedup"] = round(min(bm.values()) / row["median_ms"], 2)
            ok[name] = bool(row["median_ms"] < min(bm.values()) - spread)
        line["shapes"][name] = row
    line["required"] = {"below_the_baseline_by_more_than_its_spread": ok} if base is not None else None
    line["kernels"] = _timing.kernel_rows("k_ice<")
    _timing.write(args.out, line)
    return 0 if all(ok.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
