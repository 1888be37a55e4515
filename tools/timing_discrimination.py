#!/usr/bin/env python3
"""ms per call of the per-draw discrimination measures on the device against the route before them, on one GPU.

On a real probit chain of ``sample_chain`` (the default shape has cfg2's dimensions: 100 k rows x 50 columns, m = 200,
1000 draws), AUC, KS and the counts at 2 thresholds in 8 groups of contiguous rows, from host arrays to host results,
the median of ``--reps`` calls after one warm-up call:

* ``discrimination``   per chunk of draws and block of rows one ``pgb_predict`` and one ``pgb_rank_keys``; per chunk one
                       ``pgb_rank_metrics``.  ``(draws, groups, 2 + 2 T)`` integers reach the host.
* THE BASELINE         the route before it: ``sample_posterior`` to the host -- ``(draws, n)`` doubles --, the link and a
                       rank-sum AUC (``scipy.stats.rankdata``) and the threshold counts per draw and group in NumPy (no
                       KS: the baseline does less).  With ``--baseline-root DIR`` it runs in a process of its own on the
                       package found in ``DIR`` (a built checkout of the parent commit), twice (``host`` /
                       ``host_again``) so that its run-to-run spread is on record.  It is timed at ``--host-draws`` draws
                       (default 32) and the figure for all draws is reported as SCALED, NOT MEASURED.
* the kernels          ``k_rank_keys``, the segmented sort and ``k_rank_count`` alone between their own stream events
                       (``PGB_WALK_TIMING``, ``pgb_rank_kernel_ms``) on ``--kernel-draws`` draws at all rows; the sort as
                       bytes per second -- 16 per key: one read, one write, what a sort cannot do without -- against the
                       copy bandwidth recorded in ``profiles/survival_timing.json``.

Writes ``profiles/discrimination_timing.json`` (``--out``) with the kernel-resource rows of ``k_rank_*`` and prints it as
one JSON line.  Nothing is required of the figures.
(The file is not named ``*_timing.py``: ``tests/test_timing_tools.py`` holds the list of those; this tool's own ``--help``
is checked in ``tests/test_discrimination.py``.)

  python tools/timing_discrimination.py [--reps 3] [--shapes cfg2] [--host-draws 32] [--baseline-root DIR] [--out FILE]
"""

from __future__ import annotations

import ctypes as C
import json
import os
import sys
import time

import _timing

SHAPES = {
    "plot": dict(n=4000, p=6, m=50, draws=16),
    "cfg2": dict(n=100_000, p=50, m=200, draws=1000),
}
N_GROUPS, THRESHOLDS = 8, (0.2, 0.5)
LEGS = ("host", "host_again")


def _fit(shape):
    """A probit chain on ``n`` rows of ``p`` standard normal covariates, ``y ~ Bernoulli(Phi(0.8 x_0 - 0.5 x_1))`` ->
    ``(X, y, the sampler, seconds)``."""
    import numpy as np
    from scipy.special import ndtr

    from pymc_bart_amd import BARTOp, BernoulliLikelihood
    from pymc_bart_amd.chains import sample_chain
    from pymc_bart_amd.utils import _get_posterior_sampler

    rng = np.random.default_rng(7)
    X = rng.normal(size=(shape["n"], shape["p"]))
    y = (rng.random(shape["n"]) < ndtr(0.8 * X[:, 0] - 0.5 * X[:, 1])).astype(np.float64)
    op = BARTOp(X, y, m=shape["m"])
    t0 = time.perf_counter()
    sample_chain(op, 10, shape["draws"], num_particles=10, random_seed=7, keep_draws=False, likelihood=BernoulliLikelihood("probit"))
    return X, y, _get_posterior_sampler(op), time.perf_counter() - t0


def groups_of(n):
    import numpy as np

    return (np.arange(n) * N_GROUPS) // n


def route_before(sampler, X, y, groups, draws):
    """``sample_posterior`` to the host, then per draw and group the link, a rank-sum AUC and the threshold counts ->
    ``auc (D, G)``, ``tp``, ``fp`` ``(D, G, T)``."""
    import numpy as np
    from scipy.special import ndtr
    from scipy.stats import rankdata

    p = ndtr(np.asarray(sampler.sample_posterior(X, list(draws), None))[:, 0, :])          # (D, n)
    D = p.shape[0]
    auc, tp, fp = np.empty((D, N_GROUPS)), np.empty((D, N_GROUPS, 2), np.int64), np.empty((D, N_GROUPS, 2), np.int64)
    members = [np.flatnonzero(groups == g) for g in range(N_GROUPS)]
    for d in range(D):
        for g, rows in enumerate(members):
            v, pos = p[d, rows], y[rows] == 1
            n1, n0 = int(pos.sum()), int((~pos).sum())
            auc[d, g] = (rankdata(v)[pos].sum() - n1 * (n1 + 1) / 2.0) / (n1 * n0)
            for t, level in enumerate(THRESHOLDS):
                tp[d, g, t], fp[d, g, t] = (v[pos] >= level).sum(), (v[~pos] >= level).sum()
    return {"auc": auc, "tp": tp, "fp": fp}


def baseline(names, reps, host_draws) -> dict:
    """The route before on the package found on sys.path, timed twice per round, at every shape."""
    import torch  # noqa: F401

    import pymc_bart_amd

    # (the parent commit has no pymc_bart_amd/discrimination.py: the mark that the baseline's package is not this tree's)
    out = {"has_discrimination_module": os.path.exists(os.path.join(os.path.dirname(pymc_bart_amd.__file__), "discrimination.py"))}
    for name in names:
        X, y, sampler, secs = _fit(SHAPES[name])
        groups, draws = groups_of(X.shape[0]), range(min(host_draws, SHAPES[name]["draws"]))
        out[name] = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, lambda: route_before(sampler, X, y, groups, draws)), reps))
        out[name].update(chain_seconds=round(secs, 1), draws_timed=len(draws))
    return out


def _kernels_alone(sampler, X, y, groups, reps, n_draws):
    """The three steps on ``n_draws`` draws at all rows, each between its own events -> ``({step: ms}, keys)``."""
    import numpy as np

    import importlib

    disc = importlib.import_module("pymc_bart_amd.discrimination")   # (the package's attribute of that name is the function)
    from pymc_bart_amd._stored import Job

    job = Job(sampler)
    job.take_X(X)
    job.take_draws(list(range(n_draws)))
    job.take_history()
    res = _timing.resident_predictions(job)
    be = res.backend
    lib, mem = be.lib, be.mem
    n, D = job.n, job.D
    lay = disc.Layout(y, groups, n)
    keys_fn, ws_query, metrics_fn = lib.rank_entry_points()
    thr = np.asarray(THRESHOLDS, np.float64)
    keys, ws = mem.empty((D * n,), np.float64), mem.empty((int(ws_query(D, n, lay.G)) // 8 + 1,), np.float64)
    dd = mem.from_host(lay.dest)
    out, counts = np.empty((D, lay.G, 2 + 2 * thr.size), np.int64), (C.c_int64 * 2)()
    took = []
    with _timing.walk_timing():
        for _ in range(reps + 1):
            cnt = mem.from_host(np.zeros(2, np.int64))
            lib.check(keys_fn(mem.ptr(res.pred), D, n, n, None, disc.TRANSFORMS["probit"], mem.ptr(dd), n, mem.ptr(keys), mem.ptr(cnt),
                              mem.stream_ptr), "pgb_rank_keys")
            lib.check(metrics_fn(mem.ptr(keys), mem.ptr(ws), D, n, lay.seg_off.ctypes.data, lay.G, thr.ctypes.data, thr.size,
                                 mem.ptr(cnt), out.ctypes.data, counts, mem.stream_ptr), "pgb_rank_metrics")
            took.append(lib.rank_kernel_ms())
    med = np.median(np.asarray(took[1:]), axis=0)
    return dict(zip(("k_rank_keys", "sort", "k_rank_count"), (float(v) for v in med))), D * n


def _copy_bandwidth():
    """The copy bandwidth on record (``profiles/survival_timing.json``), TB/s, or ``None``."""
    try:
        with open(os.path.join(_timing.HERE, "profiles", "survival_timing.json")) as fh:
            return float(next(iter(json.load(fh)["shapes"].values()))["hbm_tb_per_s"]["measured_float4_copy"])
    except (OSError, KeyError, StopIteration, ValueError):
        return None


def main(argv=None) -> int:
    ap = _timing.base_parser("discrimination_timing.json", "cfg2", reps=3, baseline=True)
    ap.add_argument("--host-draws", type=int, default=32, help="the draws the baseline is timed at (its figure for all draws is scaled)")
    ap.add_argument("--kernel-draws", type=int, default=250, help="the draws of the kernels timed alone")
    args = ap.parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        _timing.print_baseline(baseline(names, args.reps, args.host_draws))
        return 0
    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import discrimination

    line = {"metric": "ms_per_call", "reps": args.reps, "groups": N_GROUPS, "thresholds": list(THRESHOLDS), "transform": "probit",
            "shapes": _timing.kept_shapes(args.out, names)}
    new = {}
    copy_tbs = _copy_bandwidth()
    for name in names:
        shape = SHAPES[name]
        X, y, sampler, secs = _fit(shape)
        groups = groups_of(X.shape[0])
        got = {}
        call = lambda: got.__setitem__("new", discrimination(sampler, X, y, groups=groups, thresholds=THRESHOLDS, transform="probit"))  # noqa: E731
        t = _timing.time_legs({"discrimination": call}, args.reps)["discrimination"]
        k_draws = min(args.kernel_draws, shape["draws"])
        k_ms, k_keys = _kernels_alone(sampler, X, y, groups, args.reps, k_draws)
        h_draws = range(min(args.host_draws, shape["draws"]))
        before = route_before(sampler, X, y, groups, h_draws)
        # (the route before applies SciPy's link, the device the library's: two values a rounding apart may change order)
        auc_diff = float(np.abs(got["new"]["auc"][:len(h_draws)] - before["auc"]).max())
        count_diff = int(max(np.abs(got["new"]["tp"][:len(h_draws)] - before["tp"]).max(),
                             np.abs(got["new"]["fp"][:len(h_draws)] - before["fp"]).max()))
        tbs = 16.0 * k_keys / (k_ms["sort"] * 1e-3) / 1e12
        new[name] = {"shape": dict(shape, chain_seconds=round(secs, 1)), **t, "n_chunks": got["new"]["n_chunks"],
                     "auc_mean": [round(float(v), 4) for v in got["new"]["auc_mean"]],
                     "kernel_draws": k_draws, "kernel_keys": int(k_keys), "k_rank_keys_ms": round(k_ms["k_rank_keys"], 4),
                     "sort_ms": round(k_ms["sort"], 4), "k_rank_count_ms": round(k_ms["k_rank_count"], 4),
                     "sort_tb_per_s_at_16_bytes_per_key": round(tbs, 3), "copy_tb_per_s_on_record": copy_tbs,
                     "sort_over_copy": None if copy_tbs is None else round(tbs / copy_tbs, 3),
                     "auc_max_abs_difference_to_the_route_before": auc_diff, "count_max_abs_difference_to_the_route_before": count_diff}
        print(f"[timing_discrimination] {name}: {json.dumps(new[name])}", file=sys.stderr, flush=True)
        del X, sampler, got
    base = None
    if args.baseline_root:
        base = _timing.run_baseline(__file__, args.baseline_root, ["--reps", str(args.reps), "--shapes", ",".join(names),
                                                                   "--host-draws", str(args.host_draws)])
    for name in names:
        row = new[name]
        if base is not None:
            b = {k: v for k, v in base[name].items() if k != "draws_timed"}
            timed, D = base[name]["draws_timed"], SHAPES[name]["draws"]
            spread = _timing.spread(b, LEGS)
            scale = D / timed
            row["baseline"] = {"what": "sample_posterior to the host, the link, scipy.stats.rankdata and the threshold counts per draw "
                                       "and group in NumPy (no KS)",
                               "measured_on": "a checkout of the parent commit, in a process of its own",
                               "has_discrimination_module": base["has_discrimination_module"], "draws_timed": timed, **b}
            row["baseline_spread_ms"] = round(spread, 3)
            best = min(b["median_ms"].values())
            if timed == D:
                row["speedup_against_the_baseline"] = round(best / row["median_ms"], 2)
                row["below_the_baseline_by_more_than_its_spread"] = bool(row["median_ms"] < best - spread)
            else:
                row["baseline_all_draws_ms_scaled_not_measured"] = round(best * scale, 1)
                row["speedup_against_the_scaled_baseline"] = round(best * scale / row["median_ms"], 2)
                # the call of ALL draws against the baseline's MEASURED time for a part of them: no scaling in this line
                row["all_draws_below_the_baseline_of_draws_timed_by_more_than_its_spread"] = bool(row["median_ms"] < best - spread)
        line["shapes"][name] = row
    line["kernels"] = _timing.kernel_rows("k_rank")
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
