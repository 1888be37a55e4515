#!/usr/bin/env python3
"""ms per call of the per-row posterior summary on the device against what a user did before it, on one GPU.

Per shape, on a real chain of ``sample_chain`` (data: ``workloads.cfg2``), from host arrays to host results, the median
of ``--reps`` calls after one warm-up call:

* ``posterior_summary``   ``pymc_bart_amd.posterior_summary(sampler, X)`` with its defaults (quantiles 3 / 50 / 97 %,
                          94 % HDI): per block of rows one ``pgb_predict`` into device scratch and one
                          ``pgb_row_summary`` on it; ``(5 + 2) x n`` doubles reach the host.
* THE BASELINE            ``sample_posterior`` of all draws to the host, then ``mean(0)``, ``np.quantile`` and
                          ``importance.hdi`` column by column.  With ``--baseline-root DIR`` it is timed in a process
                          of its own on the package found in ``DIR`` (a built checkout of the parent commit), twice
                          (``host`` / ``host_again``) so that its run-to-run spread is on record.
* ``k_rowsum``            ``pgb_row_summary`` alone on the resident predictions of the same shape, between two events
                          of the stream.

Shapes: ``plot`` (1000 rows x 10 columns, m = 50, 200 draws) and ``large`` (100 k x 50, m = 200, 1000 draws).  Writes
``profiles/rowsummary_timing.json`` (``--out``; shapes already in the file and not timed now are kept) with the
kernel-resource row of ``k_rowsum`` and prints it as one JSON line.  Nothing is required of the figures: the file says
per shape whether the new call is below the baseline by more than the baseline's own spread.

  python tools/rowsummary_timing.py [--reps 5] [--shapes plot,large] [--baseline-root DIR] [--out FILE]
"""

from __future__ import annotations

import json
import os
import sys

import _timing

SHAPES = {
    "plot": dict(n=1000, p=10, m=50, draws=200),
    "large": dict(n=100_000, p=50, m=200, draws=1000),
}
QUANTILES = (0.03, 0.5, 0.97)
HDI_PROB = 0.94
LEGS = ("host", "host_again")


def _fit(shape):
    from pymc_bart_amd.utils import _get_posterior_sampler

    f = _timing.fit(shape)
    return f.X, _get_posterior_sampler(f.op), f.seconds


def on_the_host(sampler, X):
    """What a user does without the device summary: every draw's predictions to the host, NumPy on top."""
    import numpy as np

    from pymc_bart_amd.importance import hdi

    pred = np.asarray(sampler.sample_posterior(X, list(range(sampler.n_draws)), None))  # (D, K, n)
    flat = pred.reshape(pred.shape[0], -1)
    mean, sd = flat.mean(axis=0), flat.std(axis=0, ddof=1)
    qs = np.quantile(flat, QUANTILES, axis=0)
    band = np.array([hdi(flat[:, c], HDI_PROB) for c in range(flat.shape[1])])
    return mean, sd, qs, band


def baseline(names, reps) -> dict:
    """The host path on the package found on sys.path, timed twice per round, at every shape."""
    import torch  # noqa: F401

    import pymc_bart_amd

    # (the parent commit has no pymc_bart_amd/summary.py: the mark that the baseline's package is not this tree's)
    out = {"has_summary_module": os.path.exists(os.path.join(os.path.dirname(pymc_bart_amd.__file__), "summary.py"))}
    for name in names:
        X, sampler, secs = _fit(SHAPES[name])
        out[name] = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, lambda: on_the_host(sampler, X)), reps))
        out[name]["chain_seconds"] = round(secs, 1)
    return out


def _kernel_alone(sampler, X, reps):
    """``pgb_row_summary`` on the resident predictions of every draw at every row, by stream events; also whether its
    output is what ``posterior_summary`` returned."""
    import numpy as np

    from pymc_bart_amd import summary

    job = summary.SummaryJob(sampler, X, None, QUANTILES, HDI_PROB, "identity", None, None)
    res = _timing.resident_predictions(job)
    lib, mem = res.backend.lib, res.backend.mem
    n, D, K = job.n, job.D, job.K
    rows = 2 + job.q.size + 2
    od = mem.empty((rows * K * n,), np.float64)
    call = lib.rowsummary_entry_point()
    ms = _timing.events_ms(lambda: lib.check(call(mem.ptr(res.pred), D, K * n, K * n, None, job.code, job.q.ctypes.data,
                                                  int(job.q.size), job.hdi_k, mem.ptr(od), mem.stream_ptr),
                                             "pgb_row_summary"), reps)
    return ms, mem.to_host(od).reshape(rows, K, n)


def main(argv=None) -> int:
    args = _timing.base_parser("rowsummary_timing.json", "plot,large", baseline=True).parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        _timing.print_baseline(baseline(names, args.reps))
        return 0
    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import posterior_summary

    line = {"metric": "ms_per_call", "reps": args.reps, "quantiles": list(QUANTILES), "hdi_prob": HDI_PROB,
            "shapes": _timing.kept_shapes(args.out, names)}
    new = {}
    for name in names:
        shape = SHAPES[name]
        X, sampler, secs = _fit(shape)
        last = {}

        def leg():
            last["res"] = posterior_summary(sampler, X, quantiles=QUANTILES, hdi_prob=HDI_PROB)

        t = _timing.time_legs({"posterior_summary": leg}, args.reps)["posterior_summary"]
        k_ms, stats = _kernel_alone(sampler, X, args.reps)
        res = last["res"]
        same = bool(np.array_equal(stats[0].T, res["mean"]) and np.array_equal(np.moveaxis(stats[5:7], 1, 2), res["hdi"]))
        new[name] = {"shape": dict(shape, chain_seconds=round(secs, 1)), **t, "k_rowsum_ms": round(k_ms, 4),
                     "k_rowsum_share_of_the_call": round(k_ms / t["median_ms"], 4),
                     "k_rowsum_columns_per_s": round(X.shape[0] * sampler.n_outputs / k_ms * 1e3, 1),
                     "k_rowsum_equals_the_call_bits": same}
        print(f"[rowsummary_timing] {name}: {json.dumps(new[name])}", file=sys.stderr, flush=True)
        del X, sampler, stats, last
    base = None
    if args.baseline_root:
        base = _timing.run_baseline(__file__, args.baseline_root, ["--reps", str(args.reps), "--shapes", ",".join(names)])
    for name in names:
        row = new[name]
        if base is not None:
            b = base[name]
            bm = b["median_ms"]
            spread = _timing.spread(b, LEGS)
            row["baseline"] = {"measured_on": "a checkout of the parent commit, in a process of its own",
                               "has_summary_module": base["has_summary_module"], **b}
            row["baseline_spread_ms"] = round(spread, 3)
            row["speedup"] = round(min(bm.values()) / row["median_ms"], 2)
            row["below_the_baseline_by_more_than_its_spread"] = bool(row["median_ms"] < min(bm.values()) - spread)
        line["shapes"][name] = row
    line["kernels"] = _timing.kernel_rows(lambda k: k == "k_rowsum")
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
