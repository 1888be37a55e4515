#!/usr/bin/env python3
"""ms per call of Friedman's H-statistic on the device against the only route before it, on one GPU.

On a real Normal chain of ``sample_chain`` (data: ``workloads.cfg2``; the default shape is cfg2-shaped: 100 k x 50,
m = 200, 32 draws), all 50 columns and all 1225 pairs, the rows of ``X`` as their own background, from host arrays to
host results, the median of ``--reps`` calls after one warm-up call:

* ``friedman_h``   per chunk of pairs one pass of ``pgb_hstat_background`` over the background rows and one of
                   ``pgb_hstat_rows`` over the evaluation rows; ``(draws, pairs)`` doubles reach the host.
* THE BASELINE     the route before it, from the definition: for a CORNER small enough to run -- ``--baseline-pairs``
                   pairs (default 3), ``--baseline-rows`` evaluation rows and as many background rows (default 256) --
                   the ``rows x rows`` hybrid copies of ``X`` for S = {a}, {b}, {a, b} and one
                   ``average_prediction(H, groups=evaluation row)`` call each, plus one for the plain mean.  Its time is
                   SCALED to the full call by ``(n / rows)^2 * (pairs / baseline pairs)``: stated as scaled, not
                   measured, at the full size.  With ``--baseline-root DIR`` it runs in a process of its own on the
                   package found in ``DIR`` (a built checkout of the parent commit), twice (``host`` / ``host_again``)
                   so that its run-to-run spread is on record.
* the kernels      ``k_hstat_bg`` and ``k_hstat_rows`` (both passes), each between its own stream events
                   (``PGB_WALK_TIMING``) in one more call, summed over its blocks and chunks; the number of chunks;
                   and the mean number of common trees of a pair over ``m``.

Writes ``profiles/hstat_timing.json`` (``--out``) with the kernel-resource rows of ``k_hstat_*`` and prints it as one
JSON line.  Nothing is required of the figures.
(The file is not named ``*_timing.py``: ``tests/test_timing_tools.py`` holds the list of those; this tool's own ``--help``
is checked in ``tests/test_hstat.py``.)

  python tools/timing_hstat.py [--reps 3] [--shapes cfg2] [--baseline-pairs 3] [--baseline-rows 256] [--baseline-root DIR]
"""

from __future__ import annotations

import json
import os
import sys

import _timing

SHAPES = {
    "plot": dict(n=2000, p=10, m=50, draws=16),
    "cfg2": dict(n=100_000, p=50, m=200, draws=32),
}
LEGS = ("host", "host_again")


def _fit(shape):
    from pymc_bart_amd.utils import _get_posterior_sampler

    f = _timing.fit(shape)
    return f.X, _get_posterior_sampler(f.op), f.seconds


def _kernel_totals(lib, call) -> dict:
    """``call()`` with the library's ``pgb_hstat_*`` entry points wrapped: the kernel times of every block and chunk
    (``pgb_hstat_kernel_ms`` after each call) summed, and how many calls there were."""
    tot = {"k_hstat_bg": 0.0, "k_hstat_rows": 0.0, "background_calls": 0, "rows_calls": 0, "finish_calls": 0}
    orig = lib.hstat_entry_points

    def wrapped():
        ws, bg, rows, fin = orig()

        def after(fn, key, slot):
            def run(*a):
                rc = fn(*a)
                tot[key + "_calls"] += 1
                if slot is not None:
                    tot[("k_hstat_bg", "k_hstat_rows")[slot]] += lib.hstat_kernel_ms()[slot]
                return rc
            return run

        return ws, after(bg, "background", 0), after(rows, "rows", 1), after(fin, "finish", None)

    lib.hstat_entry_points = wrapped
    try:
        call()
    finally:
        del lib.hstat_entry_points
    return tot


def route_before(sampler, X, pairs, rows):
    """``var(I_ab)`` ``[(D,)]`` per pair on the corner ``X[:rows]`` (its own background) by ``average_prediction`` on
    hybrid copies of it."""
    import numpy as np

    from pymc_bart_amd import average_prediction

    Xc = np.ascontiguousarray(X[:rows])
    n = Xc.shape[0]
    who = np.repeat(np.arange(n), n)                                   # the evaluation row of every hybrid row

    def pd(S):
        H = np.tile(Xc, (n, 1))                                        # row i * n + r: the background row r ...
        for c in S:
            H[:, c] = np.repeat(Xc[:, c], n)                           # ... with the evaluation row's value on S
        return average_prediction(sampler, H, groups=who)["mean"][:, :, 0]   # (D, n)

    pd0 = average_prediction(sampler, Xc)["mean"][:, 0, 0]
    out = []
    for a, b in pairs:
        inter = pd([a, b]) - pd([a]) - pd([b]) + pd0[:, None]
        out.append(inter.var(axis=1))
    return out


def baseline(names, reps, n_pairs, rows) -> dict:
    """The route before on the package found on sys.path, timed twice per round, at every shape."""
    import torch  # noqa: F401

    import pymc_bart_amd

    # (the parent commit has no pymc_bart_amd/hstat.py: the mark that the baseline's package is not this tree's)
    out = {"has_hstat_module": os.path.exists(os.path.join(os.path.dirname(pymc_bart_amd.__file__), "hstat.py"))}
    for name in names:
        X, sampler, secs = _fit(SHAPES[name])
        pairs = [(0, j) for j in range(1, n_pairs + 1)]
        out[name] = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, lambda: route_before(sampler, X, pairs, rows)), reps))
        out[name].update(chain_seconds=round(secs, 1), pairs_timed=len(pairs), rows_timed=min(rows, X.shape[0]))
    return out


def main(argv=None) -> int:
    ap = _timing.base_parser("hstat_timing.json", "cfg2", reps=3, baseline=True)
    ap.add_argument("--baseline-pairs", type=int, default=3)
    ap.add_argument("--baseline-rows", type=int, default=256)
    args = ap.parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        _timing.print_baseline(baseline(names, args.reps, args.baseline_pairs, args.baseline_rows))
        return 0
    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import friedman_h
    from pymc_bart_amd.sampler import default_backend

    line = {"metric": "ms_per_call", "reps": args.reps, "shapes": _timing.kept_shapes(args.out, names)}
    new = {}
    for name in names:
        shape = SHAPES[name]
        X, sampler, secs = _fit(shape)
        got = {}
        t = _timing.time_legs({"friedman_h": lambda: got.__setitem__("new", friedman_h(sampler, X))}, args.reps)["friedman_h"]
        with _timing.walk_timing():                                    # one more call, its kernels between stream events
            k = _kernel_totals(default_backend().lib, lambda: friedman_h(sampler, X))
        res = got["new"]
        corner = [(0, j) for j in range(1, 3)]
        rows = min(128, X.shape[0])
        before = route_before(sampler, X, corner, rows)
        mine = friedman_h(sampler, X[:rows], cols=[0, 1, 2], pairs=corner)["inter_sd"] ** 2
        close = bool(all(np.allclose(mine[:, j], before[j], rtol=1e-6, atol=1e-12) for j in range(len(corner))))
        common = float(res["n_common_trees"].mean())
        new[name] = {"shape": dict(shape, chain_seconds=round(secs, 1), columns=int(X.shape[1]), pairs=int(res["pairs"].shape[0])),
                     **t, "k_hstat_bg_ms_per_call": round(k["k_hstat_bg"], 3), "k_hstat_rows_ms_per_call": round(k["k_hstat_rows"], 3),
                     "background_calls": k["background_calls"], "rows_calls": k["rows_calls"], "chunks": k["finish_calls"],
                     "mean_common_trees_of_a_pair": round(common, 3), "mean_common_trees_over_m": round(common / shape["m"], 5),
                     "inter_var_close_to_the_route_before_on_a_corner": close}
        print(f"[timing_hstat] {name}: {json.dumps(new[name])}", file=sys.stderr, flush=True)
        del X, sampler, got, res
    base = None
    if args.baseline_root:
        base = _timing.run_baseline(__file__, args.baseline_root, ["--reps", str(args.reps), "--shapes", ",".join(names),
                                                                   "--baseline-pairs", str(args.baseline_pairs),
                                                                   "--baseline-rows", str(args.baseline_rows)])
    for name in names:
        row = new[name]
        if base is not None:
            b = base[name]
            scale = (row["shape"]["n"] / b["rows_timed"]) ** 2 * row["shape"]["pairs"] / b["pairs_timed"]
            bm = {k: v * scale for k, v in b["median_ms"].items()}
            row["baseline"] = {"what": "average_prediction on rows x rows hybrid copies of X, three per pair, on a corner",
                               "measured_on": "a checkout of the parent commit, in a process of its own",
                               "has_hstat_module": base["has_hstat_module"], "scaled": True, "scaled_by": round(scale, 1),
                               "scaled_median_ms": {k: round(v, 1) for k, v in bm.items()}, **b}
            row["speedup_against_the_scaled_baseline"] = round(min(bm.values()) / row["median_ms"], 1)
        line["shapes"][name] = row
    line["kernels"] = _timing.kernel_rows("k_hstat")
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
