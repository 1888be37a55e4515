#!/usr/bin/env python3
"""ms per call of the accumulated local effects on the device against the route before it, on one GPU.

On a real Normal chain of ``sample_chain`` (data: ``workloads.cfg2``; the default shape is cfg2-shaped: 100 k x 50,
m = 200, 32 draws), all 50 columns, 40 bins, from host arrays to host results, the median of ``--reps`` calls after one
warm-up call:

* ``accumulated_local_effects``  per block of rows one ``pgb_predict_ale`` into device scratch and one ``pgb_row_reduce``
                                 per column; ``(draws, bins)`` doubles per column reach the host.
* THE BASELINE                   the route before it: per column two copies of ``X`` with the column set to the upper and
                                 to the lower edge of every row's bin (``np.searchsorted``, as ``pgb_ale_bin`` is defined),
                                 and one ``average_contrast(X_hi, X_lo, groups=bin)`` -- two ``pgb_predict`` walks of all
                                 ``m`` trees of every draw.  It is timed on ``--baseline-cols`` columns (default 5) and
                                 SCALED by the number of columns to the full call: labelled as scaled, not measured, at the
                                 full size.  With ``--baseline-root DIR`` it runs in a process of its own on the package
                                 found in ``DIR`` (a built checkout of the parent commit), twice (``host`` /
                                 ``host_again``) so that its run-to-run spread is on record.
* ``k_ale``                      against ``k_predict`` on the same rows and draws, each between its own stream events
                                 (``PGB_WALK_TIMING``), and the mean length of a use list over ``m``: per column the kernel
                                 visits that share of the trees twice where the baseline visits all of them twice -- the
                                 expected gain of the kernel is that ratio.

Writes ``profiles/ale_timing.json`` (``--out``) with the kernel-resource rows of ``k_ale`` and ``k_ale_bins`` and prints
it as one JSON line.  Nothing is required of the figures.
(The file is not named ``*_timing.py``: ``tests/test_timing_tools.py`` holds the list of those; this tool's own ``--help``
is checked in ``tests/test_ale.py``.)

  python tools/timing_ale.py [--reps 3] [--shapes cfg2] [--baseline-cols 5] [--baseline-root DIR] [--out FILE]
"""

from __future__ import annotations

import ctypes as C
import json
import os
import sys

import _timing

SHAPES = {
    "plot": dict(n=2000, p=10, m=50, draws=16),
    "cfg2": dict(n=100_000, p=50, m=200, draws=32),
}
BINS = 40
LEGS = ("host", "host_again")


def edges_of(x, bins=BINS):
    """``ale_edges`` restated, so that a checkout without the module can run the baseline."""
    import numpy as np

    v = x[np.isfinite(x)]
    distinct = np.unique(v)
    if distinct.size <= bins + 1:
        return distinct
    return np.unique(np.quantile(v, np.linspace(0.0, 1.0, bins + 1), method="inverted_cdf"))


def _fit(shape):
    from pymc_bart_amd.utils import _get_posterior_sampler

    f = _timing.fit(shape)
    return f.X, _get_posterior_sampler(f.op), f.seconds


def route_before(sampler, X, cols):
    """``local_effect`` ``[(D, B)]`` per column by one ``average_contrast`` call on two edge copies of ``X`` (the
    workload's columns hold no NaN: no missing bin)."""
    import numpy as np

    from pymc_bart_amd import average_contrast

    out = []
    for c in cols:
        e = edges_of(X[:, c])
        b = np.searchsorted(e[1:-1], X[:, c], side="left")
        X_hi, X_lo = X.copy(), X.copy()
        X_hi[:, c], X_lo[:, c] = e[b + 1], e[b]
        got = average_contrast(sampler, X_hi, X_lo, groups=b)
        mean = np.zeros((got["mean"].shape[0], e.size - 1))
        mean[:, got["group_labels"]] = got["mean"][:, :, 0]
        out.append(mean)
    return out


def baseline(names, reps, n_cols) -> dict:
    """The route before on the package found on sys.path, timed twice per round, at every shape."""
    import torch  # noqa: F401

    import pymc_bart_amd

    # (the parent commit has no pymc_bart_amd/ale.py: the mark that the baseline's package is not this tree's)
    out = {"has_ale_module": os.path.exists(os.path.join(os.path.dirname(pymc_bart_amd.__file__), "ale.py"))}
    for name in names:
        X, sampler, secs = _fit(SHAPES[name])
        cols = [c for c in range(X.shape[1]) if edges_of(X[:, c]).size >= 2][:n_cols]   # (the columns that vary)
        out[name] = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, lambda: route_before(sampler, X, cols)), reps))
        out[name].update(chain_seconds=round(secs, 1), columns_timed=len(cols))
    return out


def _kernels_alone(sampler, X, reps):
    """``k_ale`` (all columns) and ``k_predict`` on the same rows and draws, each between its own events; the mean
    use-list length over ``m``."""
    import numpy as np

    from pymc_bart_amd.ale import AleJob

    job = AleJob(sampler, X, None, BINS, None, None, None, 0.94)
    be = job.hip_backend("a timing tool runs")
    lib, mem = be.lib, be.mem
    n, D, K, q = min(job.n, 64 * 256), job.D, job.K, job.q   # (16 k rows: q D K n doubles of scratch)
    ale_call = lib.predict_ale_entry_point()
    ms = {}
    for name in ("pgb_walk_kernel_ms", "pgb_ale_kernel_ms"):
        ms[name] = getattr(lib.lib, name)
        ms[name].argtypes = [C.POINTER(C.c_double)]
    xd = mem.from_host(job.X[:n])
    fd, sd, bd = mem.empty((D * K * n,), np.float64), mem.empty((q * D * K * n,), np.float64), mem.empty((q * n,), np.int32)
    edges = np.ascontiguousarray(np.concatenate(job.edges))
    edge_off = np.concatenate([[0], np.cumsum(job.G)]).astype(np.int32)
    carr = job.pool.as_c()
    picks = np.arange(D, dtype=np.int32)
    took = {"k_predict": [], "k_ale": []}
    with _timing.walk_timing():
        for _ in range(reps + 1):
            v = C.c_double()
            lib.check(lib.lib.pgb_predict(C.byref(carr), job.fidx.ctypes.data, D, job.m, mem.ptr(xd), n, job.p, job.p, None, 0,
                                          mem.ptr(fd), mem.stream_ptr), "pgb_predict")
            ms["pgb_walk_kernel_ms"](C.byref(v))
            took["k_predict"].append(v.value)
            lib.check(ale_call(C.byref(carr), job.fidx.ctypes.data, D, job.m, mem.ptr(xd), n, job.p, job.p, job.cols.ctypes.data,
                               q, edges.ctypes.data, edge_off.ctypes.data, picks.ctypes.data, D, mem.ptr(sd), mem.ptr(bd),
                               mem.stream_ptr), "pgb_predict_ale")
            ms["pgb_ale_kernel_ms"](C.byref(v))
            took["k_ale"].append(v.value)
    took = {k: float(np.median(v[1:])) for k, v in took.items()}
    # the use lists, recounted: per (draw, column) the trees of the draw that use the column
    pool = job.pool.decoded() if hasattr(job.pool, "decoded") else job.pool
    uses = np.zeros((pool.n_trees, job.p), bool)
    tree_of = np.searchsorted(np.asarray(pool.node_off), np.arange(pool.total_nodes), side="right") - 1
    split = np.asarray(pool.var) >= 0
    uses[tree_of[split], np.asarray(pool.var)[split]] = True           # (a fit's trees hold no unreachable nodes)
    lin = ~split & (np.asarray(pool.svar) >= 0) & (np.asarray(pool.svar) < job.p)
    uses[tree_of[lin], np.asarray(pool.svar)[lin]] = True
    mean_len = float(uses[job.fidx][:, :, job.cols].sum(axis=1).mean())
    return took, n, q, mean_len


def main(argv=None) -> int:
    ap = _timing.base_parser("ale_timing.json", "cfg2", reps=3, baseline=True)
    ap.add_argument("--baseline-cols", type=int, default=5)
    args = ap.parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        _timing.print_baseline(baseline(names, args.reps, args.baseline_cols))
        return 0
    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import accumulated_local_effects

    line = {"metric": "ms_per_call", "reps": args.reps, "bins": BINS, "shapes": _timing.kept_shapes(args.out, names)}
    new = {}
    for name in names:
        shape = SHAPES[name]
        X, sampler, secs = _fit(shape)
        got = {}
        t = _timing.time_legs({"accumulated_local_effects": lambda: got.__setitem__("new", accumulated_local_effects(
            sampler, X, bins=BINS))}, args.reps)["accumulated_local_effects"]
        k_ms, k_rows, q, mean_len = _kernels_alone(sampler, X, args.reps)
        some = [int(c) for c in got["new"]["cols"][:2]]
        before = route_before(sampler, X, some)
        close = bool(all(np.allclose(got["new"]["local_effect"][j], before[j], rtol=0.0, atol=1e-9) for j in range(len(some))))
        m = shape["m"]
        new[name] = {"shape": dict(shape, chain_seconds=round(secs, 1), columns=int(X.shape[1]), columns_kept=int(q)), **t,
                     "kernel_rows": k_rows, "k_predict_ms": round(k_ms["k_predict"], 4), "k_ale_ms": round(k_ms["k_ale"], 4),
                     "k_ale_over_k_predict": round(k_ms["k_ale"] / k_ms["k_predict"], 3),
                     "k_predict_walks_for_the_same_work": 2 * int(q),
                     "mean_use_list_length": round(mean_len, 3), "mean_use_list_length_over_m": round(mean_len / m, 5),
                     "local_effect_close_to_the_route_before": close}
        print(f"[timing_ale] {name}: {json.dumps(new[name])}", file=sys.stderr, flush=True)
        del X, sampler, got
    base = None
    if args.baseline_root:
        base = _timing.run_baseline(__file__, args.baseline_root, ["--reps", str(args.reps), "--shapes", ",".join(names),
                                                                   "--baseline-cols", str(args.baseline_cols)])
    for name in names:
        row = new[name]
        if base is not None:
            b = base[name]
            scale = row["shape"]["columns_kept"] / b["columns_timed"]
            bm = {k: v * scale for k, v in b["median_ms"].items()}
            spread = _timing.spread(b, LEGS) * scale
            row["baseline"] = {"what": "one average_contrast(X_hi, X_lo, groups=bin) call per column on two edge copies of X",
                               "measured_on": "a checkout of the parent commit, in a process of its own",
                               "has_ale_module": base["has_ale_module"], "scaled": True,
                               "scaled_by": round(scale, 3), "scaled_median_ms": {k: round(v, 1) for k, v in bm.items()}, **b}
            row["baseline_spread_ms_scaled"] = round(spread, 3)
            row["speedup_against_the_scaled_baseline"] = round(min(bm.values()) / row["median_ms"], 2)
            row["below_the_baseline_by_more_than_its_spread"] = bool(row["median_ms"] < min(bm.values()) - spread)
        line["shapes"][name] = row
    line["kernels"] = _timing.kernel_rows("k_ale")
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
