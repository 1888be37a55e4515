#!/usr/bin/env python3
"""ms per call of ``partial_dependence`` -- one fused ``pgb_predict_pdp`` call per sampler -- against the per-covariate
``pgb_predict`` loop it replaced, on one GPU.

The public call is timed from host arrays to host results, after warming, median of ``--reps``, at two shapes:

* ``plot``      the reference's defaults on a plot-sized fit: n = 1000, p = 10, m = 50, 500 stored draws, the
                9-quantile grid, 200 samples, all 10 columns;
* ``insample``  cfg2-shaped: 100 k x 50, m = 200, 200 draws, ``xs_interval="insample"``, 8 columns, 50 samples,
                ``summary=`` with ``keep_pd=False`` (the parent commit has no ``keep_pd``: it runs ``summary=`` with its
                matrix kept).

THE BASELINE is the same call of the package found in ``--baseline-root DIR`` (a built checkout of the parent commit),
in a process of its own, two legs (``pdp`` / ``pdp_again``) so that its run-to-run spread is on record.  Required: at
``plot`` the new call is not slower than the baseline beyond that spread.  At ``insample`` the ratio is reported.

Also recorded, per shape: ``k_pdp_walk`` and ``k_pdp_lookup`` alone between stream events (``_timing.walk_timing()``,
``pgb_pdp_kernel_ms``) under ``route=1`` and ``route=2``; at the ``insample`` fit the same for growing row counts -- the
crossover of the two routes; and the kernels' resource rows.

Writes ``profiles/pdp_timing.json`` (``--out``) and prints it as one JSON line.

  python tools/pdp_timing.py [--reps 5] [--shapes plot,insample] [--baseline-root DIR] [--out FILE]
"""

from __future__ import annotations

import ctypes as C
import json
import os
import sys

import _timing

SHAPES = {
    "plot": dict(n=1000, p=10, m=50, draws=500, var_idx=None, xs_interval="quantiles", samples=200, summary=False),
    "insample": dict(n=100_000, p=50, m=200, draws=200, var_idx=list(range(8)), xs_interval="insample", samples=50,
                     summary=True),
}
CROSSOVER_ROWS = (64, 256, 1024, 4096, 16384, 65536)


LEGS = ("pdp", "pdp_again")


def _call(op, X, shape, lean: bool):
    from pymc_bart_amd import partial_dependence

    kw = dict(var_idx=shape["var_idx"], xs_interval=shape["xs_interval"], samples=shape["samples"], random_seed=3)
    if shape["summary"]:
        kw["summary"] = {}
        if lean:
            kw["keep_pd"] = False
    return partial_dependence(op, X, **kw)


def baseline(names, reps) -> dict:
    """The public call of the package on sys.path, timed twice per round, at every shape."""
    import torch  # noqa: F401

    import pymc_bart_amd

    # (the parent commit has no pymc_bart_amd/pdp.py: the mark that the baseline's package is not this tree's)
    out = {"has_pdp_module": os.path.exists(os.path.join(os.path.dirname(pymc_bart_amd.__file__), "pdp.py"))}
    lean = out["has_pdp_module"]
    for name in names:
        shape = SHAPES[name]
        f = _timing.fit(shape)
        out[name] = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, lambda: _call(f.op, f.X, shape, lean)), reps))
        out[name]["chain_seconds"] = round(f.seconds, 1)
    return out


def _kernels_alone(s, rows, cols, picks, reps):
    """``{route: {walk_ms, lookup_ms, routes}}``: the two kernels of one sweep between stream events (medians)."""
    import numpy as np

    lib = s._chain_samplers[0]._get_backend().lib
    ms_of = lib.lib.pgb_pdp_kernel_ms
    ms_of.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    out = {}
    with _timing.walk_timing():
        for route, name in ((1, "direct"), (2, "profile")):
            walk, look, taken = [], [], []
            for _ in range(reps + 1):
                a, b = C.c_double(-1.0), C.c_double(-1.0)
                del taken[:]
                s.pdp_sweep(rows, cols, picks, route=route, taken=taken)
                ms_of(C.byref(a), C.byref(b))
                walk.append(a.value)
                look.append(b.value)
            out[name] = {"k_pdp_walk_ms": round(float(np.median(walk[1:])), 4),
                         "k_pdp_lookup_ms": round(float(np.median(look[1:])), 4) if look[-1] >= 0 else None,
                         "columns_on_the_profile_route": sum(r == 2 for t in taken for r in t[4]), "blocks": len(taken)}
    return out


def _kernel_section(op, X, shape, reps, crossover: bool):
    import numpy as np

    from pymc_bart_amd.partial import pdp_grid
    from pymc_bart_amd.utils import _get_posterior_sampler

    s = _get_posterior_sampler(op)
    p = X.shape[1]
    cols = list(range(p)) if shape["var_idx"] is None else shape["var_idx"]
    grid = pdp_grid(X, shape["xs_interval"], None)
    rng = np.random.default_rng(3)
    picks = np.stack([rng.integers(0, s.n_draws, size=shape["samples"]) for _ in cols])
    part = s._chain_samplers[0]
    res = {"sweep": {"rows": int(grid.shape[0]), "columns": len(cols), "picks": int(picks.shape[1])},
           **_kernels_alone(s, part.resident_rows(grid), cols, picks, reps)}
    if crossover:
        table, first = [], None
        for n in CROSSOVER_ROWS:
            k = _kernels_alone(s, part.resident_rows(X[:n]), cols, picks, reps)
            d = k["direct"]["k_pdp_walk_ms"]
            pr = k["profile"]["k_pdp_walk_ms"] + (k["profile"]["k_pdp_lookup_ms"] or 0.0)
            table.append({"rows": n, "direct_ms": d, "profile_ms": round(pr, 4)})
            if first is None and pr < d:
                first = n
        res["crossover"] = {"by_rows": table, "profile_route_faster_from_rows": first,
                            "rule_shipped": "profile when slots summed over the picks < rows x picks"}
    return res


def main(argv=None) -> int:
    args = _timing.base_parser("pdp_timing.json", "plot,insample", baseline=True).parse_args(argv)
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
        t = _timing.time_legs({"pdp": lambda: _call(op, X, shape, True)}, args.reps)["pdp"]
        new[name] = {"shape": dict(shape, chain_seconds=round(f.seconds, 1)), **t,
                     "kernels_alone": _kernel_section(op, X, shape, args.reps, crossover=name == "insample")}
        print(f"[pdp_timing] {name}: {json.dumps(new[name])}", file=sys.stderr, flush=True)
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
            row["baseline"] = {"measured_on": where, "has_pdp_module": base["has_pdp_module"], **b}
            row["baseline_spread_ms"] = round(spread, 3)
            row["speedup"] = round(min(bm.values()) / row["median_ms"], 2)
            if name == "plot":
                ok[name] = bool(row["median_ms"] <= max(bm.values()) + spread)
        line["shapes"][name] = row
    line["required"] = {"plot_not_slower_than_the_baseline_beyond_its_spread": ok} if base is not None else None
    line["kernels"] = _timing.kernel_rows("k_pdp_")
    _timing.write(args.out, line)
    return 0 if all(ok.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
