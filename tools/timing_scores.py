#!/usr/bin/env python3
"""ms per call of the predictive scores on the device against what a user did before them, on one GPU.

Per shape, on a real Normal chain of ``sample_chain`` (data: ``workloads.cfg2``; the shapes of
``tools/rowsummary_timing.py``), from host arrays to host results, the median of ``--reps`` calls after one warm-up call:

* ``predictive_scores``   ``pymc_bart_amd.predictive_scores(sampler, X, y, NormalLikelihood("sigma"), points=...)`` with
                          its defaults (quantiles 5 / 25 / 50 / 75 / 95 %, the 50 % and 90 % intervals): per block of
                          rows one ``pgb_predict`` into device scratch, one ``pgb_ppc_draw`` in place and one
                          ``pgb_row_score``; ``(6 + 2 x 6) x n`` doubles reach the host.
* THE BASELINE            ``posterior_predictive`` of the ``(draws, rows)`` matrix to the host, ``np.sort`` over the
                          draws, then the same formulas in NumPy (the gap form of the pair sum, the counts by
                          comparison) and ``np.quantile``.  With ``--baseline-root DIR`` it is timed in a process of its
                          own on the package found in ``DIR`` (a built checkout of the parent commit), twice (``host`` /
                          ``host_again``) so that its run-to-run spread is on record.
* ``k_rowscore``          ``pgb_row_score`` alone (7 levels) on the resident predictions of the same shape, between two
                          events of the stream, next to ``pgb_row_summary`` alone (7 quantiles, no HDI) on the same matrix.

Shapes: ``plot`` (1000 rows x 10 columns, m = 50, 200 draws) and ``large`` (100 k x 50, m = 200, 1000 draws).  Writes
``profiles/score_timing.json`` (``--out``; shapes already in the file and not timed now are kept) with the
kernel-resource rows of ``k_rowscore`` and ``k_rowsum`` and prints it as one JSON line.  Nothing is required of the
figures: the file says per shape whether the new call is below the baseline by more than the baseline's own spread,
and what ``k_rowscore`` takes relative to ``k_rowsum``.

  python tools/timing_scores.py [--reps 5] [--shapes plot,large] [--baseline-root DIR] [--out FILE]
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
QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)
INTERVALS = (0.5, 0.9)
KERNEL_LEVELS = (0.05, 0.25, 0.5, 0.75, 0.95, 0.025, 0.975)
LEGS = ("host", "host_again")


def _fit(shape):
    from pymc_bart_amd.utils import _get_posterior_sampler

    f = _timing.fit(shape)
    return f.X, f.Y, _get_posterior_sampler(f.op), f.results[0]["sigma"], f.seconds


def on_the_host(sampler, X, y, sigma):
    """What a user does without the device scores: ``y_rep`` to the host, a sort over the draws, NumPy on top."""
    import numpy as np

    from pymc_bart_amd import NormalLikelihood, posterior_predictive

    yrep = posterior_predictive(sampler, X, NormalLikelihood("sigma"), points={"sigma": sigma})   # (D, n)
    D = yrep.shape[0]
    t = np.sort(yrep, axis=0)
    abs_err = np.abs(t - y).mean(axis=0)
    g = np.arange(D - 1, dtype=np.float64)
    pair = (((g + 1.0) * (D - 1.0 - g))[:, None] * np.diff(t, axis=0)).sum(axis=0)
    crps = abs_err - pair / (D * D)
    mean, var = t.mean(axis=0), t.var(axis=0, ddof=1)
    pit = ((t < y).sum(axis=0) + 0.5 * (t == y).sum(axis=0)) / D
    levels = list(QUANTILES) + [lv for c in INTERVALS for lv in ((1 - c) / 2, (1 + c) / 2) if lv not in QUANTILES]
    q = np.quantile(t, levels, axis=0)
    u = y - q[:len(QUANTILES)]
    lv = np.asarray(QUANTILES)[:, None]
    pinball = np.where(u >= 0, lv * u, (lv - 1.0) * u)
    scores = []
    for c in INTERVALS:
        lo, hi = q[levels.index((1 - c) / 2)], q[levels.index((1 + c) / 2)]
        scores.append((hi - lo) + 2 / (1 - c) * (np.maximum(lo - y, 0) + np.maximum(y - hi, 0)))
    return crps, mean, var, pit, pinball, scores


def baseline(names, reps) -> dict:
    """The host path on the package found on sys.path, timed twice per round, at every shape."""
    import torch  # noqa: F401

    import pymc_bart_amd

    # (the parent commit has no pymc_bart_amd/scores.py: the mark that the baseline's package is not this tree's)
    out = {"has_scores_module": os.path.exists(os.path.join(os.path.dirname(pymc_bart_amd.__file__), "scores.py"))}
    for name in names:
        X, y, sampler, sigma, secs = _fit(SHAPES[name])
        out[name] = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, lambda: on_the_host(sampler, X, y, sigma)), reps))
        out[name]["chain_seconds"] = round(secs, 1)
    return out


def _kernels_alone(sampler, X, y, reps):
    """``pgb_row_score`` and ``pgb_row_summary`` (the same 7 levels, no HDI) on the resident predictions of every draw
    at every row, alternating, by stream events; also whether the two agree on mean, variance and quantiles."""
    import numpy as np

    from pymc_bart_amd import summary

    job = summary.SummaryJob(sampler, X, None, KERNEL_LEVELS, None, "identity", None, None)
    res = _timing.resident_predictions(job)
    lib, mem = res.backend.lib, res.backend.mem
    n, D, K = job.n, job.D, job.K
    assert K == 1
    Q = job.q.size
    yd = mem.from_host(np.ascontiguousarray(y, np.float64))
    score_out = mem.empty(((6 + 2 * Q) * n,), np.float64)
    summ_out = mem.empty(((2 + Q + 2) * n,), np.float64)
    score, summ = lib.score_entry_point(), lib.rowsummary_entry_point()
    ms = _timing.events_ms({
        "k_rowscore": lambda: lib.check(score(mem.ptr(res.pred), D, n, n, mem.ptr(yd), job.q.ctypes.data, int(Q),
                                              mem.ptr(score_out), mem.stream_ptr), "pgb_row_score"),
        "k_rowsum": lambda: lib.check(summ(mem.ptr(res.pred), D, n, n, None, 0, job.q.ctypes.data, int(Q), 0,
                                           mem.ptr(summ_out), mem.stream_ptr), "pgb_row_summary")}, reps)
    a, b = mem.to_host(score_out).reshape(-1, n), mem.to_host(summ_out).reshape(-1, n)
    same = bool(np.array_equal(a[:2], b[:2]) and np.array_equal(a[6:6 + Q], b[2:2 + Q]))
    return ms, same


def main(argv=None) -> int:
    args = _timing.base_parser("score_timing.json", "plot,large", baseline=True).parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        _timing.print_baseline(baseline(names, args.reps))
        return 0
    import torch  # noqa: F401

    from pymc_bart_amd import NormalLikelihood, predictive_scores

    line = {"metric": "ms_per_call", "reps": args.reps, "quantiles": list(QUANTILES), "intervals": list(INTERVALS),
            "kernel_levels": list(KERNEL_LEVELS), "shapes": _timing.kept_shapes(args.out, names)}
    new = {}
    for name in names:
        shape = SHAPES[name]
        X, y, sampler, sigma, secs = _fit(shape)
        lik, pts = NormalLikelihood("sigma"), {"sigma": sigma}
        t = _timing.time_legs({"predictive_scores": lambda: predictive_scores(sampler, X, y, lik, points=pts)},
                              args.reps)["predictive_scores"]
        k_ms, same = _kernels_alone(sampler, X, y, args.reps)
        new[name] = {"shape": dict(shape, chain_seconds=round(secs, 1)), **t,
                     "k_rowscore_ms": round(k_ms["k_rowscore"], 4), "k_rowsum_ms": round(k_ms["k_rowsum"], 4),
                     "k_rowscore_relative_to_k_rowsum": round(k_ms["k_rowscore"] / k_ms["k_rowsum"], 3),
                     "k_rowscore_share_of_the_call": round(k_ms["k_rowscore"] / t["median_ms"], 4),
                     "k_rowscore_columns_per_s": round(X.shape[0] / k_ms["k_rowscore"] * 1e3, 1),
                     "mean_var_quantiles_equal_k_rowsums_bits": same}
        print(f"[timing_scores] {name}: {json.dumps(new[name])}", file=sys.stderr, flush=True)
        del X, y, sampler
    base = None
    if args.baseline_root:
        base = _timing.run_baseline(__file__, args.baseline_root, ["--reps", str(args.reps), "--shapes", ",".join(names)])
    for name in names:
        row = new[name]
        if base is not None:
            b = base[name]
            bm = b["median_ms"]
            spread = _timing.spread(b, LEGS)
            row["baseline"] = {"what": "posterior_predictive to the host + np.sort + the same formulas in NumPy + np.quantile",
                               "measured_on": "a checkout of the parent commit, in a process of its own",
                               "has_scores_module": base["has_scores_module"], **b}
            row["baseline_spread_ms"] = round(spread, 3)
            row["speedup"] = round(min(bm.values()) / row["median_ms"], 2)
            row["below_the_baseline_by_more_than_its_spread"] = bool(row["median_ms"] < min(bm.values()) - spread)
        line["shapes"][name] = row
    line["kernels"] = _timing.kernel_rows(lambda k: k in ("k_rowscore", "k_rowsum"))
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
