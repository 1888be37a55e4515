#!/usr/bin/env python3
"""ms per call of the discrete-time survival curves on the device against the route before them, on one GPU.

On a real probit chain of ``sample_chain`` on person-period rows (the default shape has cfg2's dimensions: 100 k rows x
50 columns -- the time and 49 covariates --, m = 200, 32 draws), curves of 10 k subjects on a grid of J = 50 times, 8
groups of contiguous rows, from host arrays to host results, the median of ``--reps`` calls after one warm-up call:

* ``survival_curves``  per block of rows one ``pgb_predict``; per chunk of the grid one ``pgb_predict_arms`` and one
                       ``pgb_surv_curves``; one ``pgb_row_summary`` and one ``pgb_row_reduce`` per time.  Per-row
                       summaries and ``(draws, groups, J)`` doubles reach the host.
* THE BASELINE         the route before it: the expanded matrix of n J rows, ``sample_posterior`` of it to the host --
                       ``(draws, n J)`` doubles --, the link, ``np.cumprod``, ``np.quantile`` and group means in NumPy.
                       With ``--baseline-root DIR`` it runs in a process of its own on the package found in ``DIR`` (a
                       built checkout of the parent commit), twice (``host`` / ``host_again``) so that its run-to-run
                       spread is on record.
* ``k_surv``           alone between its own stream events (``PGB_WALK_TIMING``) on one chunk of the grid, as bytes per
                       second -- 16 per element: the prediction in, the survival probability out -- against the HBM
                       bandwidth, next to ``k_arms`` on the same chunk; and the mean length of the time column's use
                       list over ``m``.

Writes ``profiles/survival_timing.json`` (``--out``) with the kernel-resource rows of ``k_surv`` and prints it as one
JSON line.  Nothing is required of the figures.
(The file is not named ``*_timing.py``: ``tests/test_timing_tools.py`` holds the list of those; this tool's own ``--help``
is checked in ``tests/test_survival.py``.)

  python tools/timing_survival.py [--reps 3] [--shapes cfg2] [--baseline-root DIR] [--out FILE]
"""

from __future__ import annotations

import ctypes as C
import json
import os
import sys
import time

import _timing

SHAPES = {
    "plot": dict(n=4000, p=6, m=50, draws=16, subjects=500, J=12),
    "cfg2": dict(n=100_000, p=50, m=200, draws=32, subjects=10_000, J=50),
}
N_GROUPS, TIME_COL = 8, 0
LEGS = ("host", "host_again")
HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0   # MI355X: a float4 copy; the data sheet


def _fit(shape):
    """A probit chain on ``shape["n"]`` person-period rows of ``shape["p"]`` columns: subjects with standard normal
    covariates whose hazard per period is ``Phi(-1.6 + 0.5 z_0 - 0.3 z_1 + 0.02 t)`` on a grid of ``J`` periods, as
    many as fill the rows.  -> ``(X of the subjects to predict (the time column empty), the grid, the sampler, seconds)``."""
    import numpy as np
    from scipy.special import ndtr

    from pymc_bart_amd import BARTOp, BernoulliLikelihood
    from pymc_bart_amd.chains import sample_chain
    from pymc_bart_amd.utils import _get_posterior_sampler

    rng = np.random.default_rng(7)
    n, p, J = shape["n"], shape["p"], shape["J"]
    grid = np.arange(1.0, J + 1)
    n_sub = n                                                              # (more than enough: every subject has a row)
    Z = rng.normal(size=(n_sub, p - 1))
    hazard = ndtr(-1.6 + 0.5 * Z[:, :1] - 0.3 * Z[:, 1:2] + 0.02 * grid[None, :])
    hit = rng.random((n_sub, J)) < hazard
    event = hit.any(axis=1)
    t = np.where(event, hit.argmax(axis=1) + 1, J).astype(np.float64)
    # the person-period layout in NumPy (``person_period``'s; the baseline's package does not have it): one row per
    # subject and period at risk, y = 1 in the period of an observed event
    rows = t.astype(np.int64)
    subject = np.repeat(np.arange(n_sub), rows)[:n]
    j = (np.arange(rows.sum()) - np.repeat(np.cumsum(rows) - rows, rows))[:n]
    X = np.column_stack([grid[j], Z[subject]])
    y = ((j + 1 == rows[subject]) & event[subject]).astype(np.float64)
    op = BARTOp(X, y, m=shape["m"])
    t0 = time.perf_counter()
    sample_chain(op, 10, shape["draws"], num_particles=10, random_seed=7, keep_draws=False, likelihood=BernoulliLikelihood("probit"))
    seconds = time.perf_counter() - t0
    Xs = np.column_stack([np.zeros(shape["subjects"]), rng.normal(size=(shape["subjects"], p - 1))])
    return Xs, grid, _get_posterior_sampler(op), seconds


def groups_of(n):
    import numpy as np

    return (np.arange(n) * N_GROUPS) // n


def route_before(sampler, X, grid, groups, n_draws):
    """The expanded matrix, ``sample_posterior`` of it to the host, NumPy for the rest -> the results of
    ``survival_curves`` (up to the rounding of the link and the order of the sums)."""
    import numpy as np
    from scipy.special import ndtr

    n, J = X.shape[0], grid.size
    big = np.repeat(X, J, axis=0)
    big[:, TIME_COL] = np.tile(grid, n)
    f = np.asarray(sampler.sample_posterior(big, list(range(n_draws)), None)).reshape(-1, n, J)
    S = np.cumprod(ndtr(-f), axis=2)                                       # (D, n, J)
    dt = np.diff(np.concatenate([[0.0], grid]))
    rmst = (np.concatenate([np.ones((S.shape[0], n, 1)), S[:, :, :-1]], axis=2) * dt).sum(axis=2)
    onehot = np.zeros((N_GROUPS, n))
    onehot[groups, np.arange(n)] = 1.0
    W = onehot.sum(axis=1)
    return {"surv_mean": S.mean(axis=0), "surv_quantiles": np.quantile(S, (0.03, 0.5, 0.97), axis=0),
            "rmst_mean": rmst.mean(axis=0), "rmst_quantiles": np.quantile(rmst, (0.03, 0.5, 0.97), axis=0),
            "surv_avg": np.einsum("dnj,gn->dgj", S, onehot) / W[None, :, None], "rmst_avg": rmst @ onehot.T / W}


def baseline(names, reps) -> dict:
    """The route before on the package found on sys.path, timed twice per round, at every shape."""
    import torch  # noqa: F401

    import pymc_bart_amd

    # (the parent commit has no pymc_bart_amd/survival.py: the mark that the baseline's package is not this tree's)
    out = {"has_survival_module": os.path.exists(os.path.join(os.path.dirname(pymc_bart_amd.__file__), "survival.py"))}
    for name in names:
        X, grid, sampler, secs = _fit(SHAPES[name])
        groups = groups_of(X.shape[0])
        out[name] = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, lambda: route_before(sampler, X, grid, groups, SHAPES[name]["draws"])), reps))
        out[name].update(chain_seconds=round(secs, 1))
    return out


def _kernels_alone(sampler, X, grid, reps):
    """``k_arms`` and ``k_surv`` on one chunk of the grid at all rows, each between its own events; the mean length of
    the time column's use list."""
    import numpy as np

    from pymc_bart_amd.survival import SurvJob

    job = SurvJob(sampler, X, grid, TIME_COL, 0, "probit", None, 0.0, None, None)
    job.take_history()
    be, predict_arms, surv = job.hip()
    lib, mem = be.lib, be.mem
    n, D, K = job.n, job.D, job.K
    A = min(job.chunk, job.J)
    t, dt = job.times[:A], job.dt[:A]
    arms = np.ascontiguousarray(t[:, None])
    xd = mem.from_host(job.X)
    fd = job.predict(be, xd, n)
    od, state = mem.empty((A * D * K * n,), np.float64), mem.empty((3 * D * n,), np.float64)
    cnt = mem.from_host(np.zeros(1, np.int64))
    level = np.array([0.5])
    lens = np.zeros(D, np.int32)
    carr = job.pool.as_c()
    took = {"k_arms": [], "k_surv": []}
    with _timing.walk_timing():
        for _ in range(reps + 1):
            lib.check(predict_arms(C.byref(carr), job.fidx.ctypes.data, D, job.m, mem.ptr(xd), n, job.p, job.p, job.cols.ctypes.data,
                                   1, arms.ctypes.data, A, job.picks.ctypes.data, D, mem.ptr(fd), mem.ptr(od), lens.ctypes.data,
                                   mem.stream_ptr), "pgb_predict_arms")
            took["k_arms"].append(lib.arms_kernel_ms()[0])
            lib.check(surv(mem.ptr(od), D * K * n, K * n, D, A, n, None, job.code, t.ctypes.data, dt.ctypes.data, level.ctypes.data, 1,
                           job.beyond, 1, mem.ptr(state), mem.ptr(cnt), mem.stream_ptr), "pgb_surv_curves")
            took["k_surv"].append(lib.surv_kernel_ms())
    return {k: float(np.median(v[1:])) for k, v in took.items()}, A, 16.0 * A * D * n, float(lens.mean())


def main(argv=None) -> int:
    ap = _timing.base_parser("survival_timing.json", "cfg2", reps=3, baseline=True)
    args = ap.parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        _timing.print_baseline(baseline(names, args.reps))
        return 0
    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import survival_curves

    line = {"metric": "ms_per_call", "reps": args.reps, "groups": N_GROUPS, "time_column": TIME_COL, "link": "probit",
            "shapes": _timing.kept_shapes(args.out, names)}
    new = {}
    for name in names:
        shape = SHAPES[name]
        X, grid, sampler, secs = _fit(shape)
        groups = groups_of(X.shape[0])
        got = {}
        t = _timing.time_legs({"survival_curves": lambda: got.__setitem__("new", survival_curves(sampler, X, grid, groups=groups))},
                              args.reps)["survival_curves"]
        k_ms, k_times, k_bytes, mean_len = _kernels_alone(sampler, X, grid, args.reps)
        before = route_before(sampler, X, grid, groups, shape["draws"])
        close = bool(all(np.allclose(got["new"][key], before[key], rtol=0.0, atol=1e-9)
                         for key in ("surv_mean", "surv_quantiles", "rmst_mean", "rmst_quantiles", "surv_avg", "rmst_avg")))
        tbs = k_bytes / (k_ms["k_surv"] * 1e-3) / 1e12
        new[name] = {"shape": dict(shape, chain_seconds=round(secs, 1)), **t, "kernel_times": k_times, "kernel_bytes": int(k_bytes),
                     "k_arms_ms": round(k_ms["k_arms"], 4), "k_surv_ms": round(k_ms["k_surv"], 4), "k_surv_tb_per_s": round(tbs, 3),
                     "k_surv_over_hbm_measured": round(tbs / HBM_MEASURED_TBS, 3), "k_surv_over_hbm_spec": round(tbs / HBM_SPEC_TBS, 3),
                     "hbm_tb_per_s": {"measured_float4_copy": HBM_MEASURED_TBS, "spec": HBM_SPEC_TBS},
                     "mean_use_list_length": round(mean_len, 3), "mean_use_list_length_over_m": round(mean_len / shape["m"], 5),
                     "n_nonfinite": got["new"]["n_nonfinite"], "close_to_the_route_before": close}
        print(f"[timing_survival] {name}: {json.dumps(new[name])}", file=sys.stderr, flush=True)
        del X, sampler, got
    base = None
    if args.baseline_root:
        base = _timing.run_baseline(__file__, args.baseline_root, ["--reps", str(args.reps), "--shapes", ",".join(names)])
    for name in names:
        row = new[name]
        if base is not None:
            b = base[name]
            spread = _timing.spread(b, LEGS)
            row["baseline"] = {"what": "the expanded matrix of n J rows, sample_posterior of it to the host, the link, np.cumprod, "
                                       "np.quantile and group means in NumPy",
                               "measured_on": "a checkout of the parent commit, in a process of its own",
                               "has_survival_module": base["has_survival_module"], **b}
            row["baseline_spread_ms"] = round(spread, 3)
            row["speedup_against_the_baseline"] = round(min(b["median_ms"].values()) / row["median_ms"], 2)
            row["below_the_baseline_by_more_than_its_spread"] = bool(row["median_ms"] < min(b["median_ms"].values()) - spread)
        line["shapes"][name] = row
    line["kernels"] = _timing.kernel_rows("k_surv")
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
