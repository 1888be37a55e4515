#!/usr/bin/env python3
"""ms per call of the permutation importance on the device against the route before it, on one GPU.

On a real Normal chain of ``sample_chain`` (data: ``workloads.cfg2``; the default shape is cfg2-shaped: 100 k x 50,
m = 200, 32 draws), all 50 columns, 5 repeats, from host arrays to host results, the median of ``--reps`` calls after one
warm-up call:

* ``permutation_importance``  per block of rows one ``pgb_predict``, one ``pgb_predict_permuted`` into device scratch and
                              the ``pgb_row_reduce`` calls; ``(draws, columns, repeats)`` doubles reach the host.
* THE BASELINE                the route before it: one ``bayes_r2`` call per (column, repeat) on a copy of ``X`` whose
                              column is permuted on the host with the same ``pgb_perm_index`` (restated in NumPy below,
                              so that a checkout without the header can run it).  Every call walks all ``m`` trees of
                              every draw.  It is timed on ``--baseline-cols`` columns (default 5) x the repeats and
                              SCALED by the number of columns to the full call: labelled as scaled, not measured, at the
                              full size.  With ``--baseline-root DIR`` it runs in a process of its own on the package
                              found in ``DIR`` (a built checkout of the parent commit), twice (``host`` / ``host_again``)
                              so that its run-to-run spread is on record.
* ``k_permimp``               against ``k_predict`` on the same rows and draws, each between its own stream events
                              (``PGB_WALK_TIMING``), and the mean length of a use list over ``m``: per column the
                              permuted walk visits that share of the trees ``R + 1`` times where the baseline visits all
                              of them ``R`` times -- the expected gain of the kernel is that ratio.

Writes ``profiles/permimp_timing.json`` (``--out``) with the kernel-resource rows of ``k_permimp`` and prints it as one
JSON line.  Nothing is required of the figures.
(The file is not named ``*_timing.py``: ``tests/test_timing_tools.py`` holds the list of those; this tool's own ``--help``
is checked in ``tests/test_permimp.py``.)

  python tools/timing_permimp.py [--reps 3] [--shapes cfg2] [--baseline-cols 5] [--baseline-root DIR] [--out FILE]
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
REPEATS = 5
SEED = 7
LEGS = ("host", "host_again")
PERMIMP_RNG = 0xFFF0  # PGB_PERMIMP_RNG


def _philox(k0, k1, c0, c1, c2, c3):
    """pgb_philox4x32_10 (include/pgbart_spec.h) on Python integers."""
    M = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M, (p0 >> 32) ^ c3 ^ k1, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c0, c1, c2, c3


def perm_index(seed: int, col: int, rep: int, n: int):
    """``pgb_perm_index(seed, col, rep, n, i)`` for every ``i`` in ``[0, n)`` (include/pgbart_permimp.h), in NumPy."""
    import numpy as np

    half = max(1, ((n - 1).bit_length() + 1) >> 1)
    mask = np.uint32((1 << half) - 1)
    b0 = _philox(seed & 0xFFFFFFFF, seed >> 32, col, rep, 0, PERMIMP_RNG << 16)
    b1 = _philox(seed & 0xFFFFFFFF, seed >> 32, col, rep, 1, PERMIMP_RNG << 16)
    keys = [np.uint32(k) for k in (*b0, b1[0], b1[1])]
    x = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, bool)
    while todo.any():
        v = x[todo]
        L, R = (v >> np.uint64(half)).astype(np.uint32), v.astype(np.uint32) & mask
        for k in keys:
            h = R ^ k
            h ^= h >> np.uint32(16)
            h *= np.uint32(0x85EBCA6B)
            h ^= h >> np.uint32(13)
            h *= np.uint32(0xC2B2AE35)
            h ^= h >> np.uint32(16)
            L, R = R, L ^ (h & mask)
        x[todo] = (L.astype(np.uint64) << np.uint64(half)) | R.astype(np.uint64)
        todo &= x >= n
    return x.astype(np.int64)


def _fit(shape):
    from pymc_bart_amd.utils import _get_posterior_sampler

    f = _timing.fit(shape)
    return f.X, f.Y, _get_posterior_sampler(f.op), f.seconds


def route_before(sampler, X, y, cols, repeats=REPEATS):
    """``mse[d, s, r]`` by one ``bayes_r2`` call per (column, repeat) on a host-permuted copy of ``X``."""
    import numpy as np

    from pymc_bart_amd import bayes_r2

    out = []
    for c in cols:
        for r in range(repeats):
            Xp = X.copy()
            Xp[:, c] = X[perm_index(SEED, int(c), r, X.shape[0]), c]
            out.append(bayes_r2(sampler, Xp, y)["mse"][:, 0])
    return np.stack(out, axis=1).reshape(-1, len(cols), repeats)


def baseline(names, reps, n_cols) -> dict:
    """The route before on the package found on sys.path, timed twice per round, at every shape."""
    import torch  # noqa: F401

    import pymc_bart_amd

    # (the parent commit has no pymc_bart_amd/permutation.py: the mark that the baseline's package is not this tree's)
    out = {"has_permutation_module": os.path.exists(os.path.join(os.path.dirname(pymc_bart_amd.__file__), "permutation.py"))}
    for name in names:
        X, y, sampler, secs = _fit(SHAPES[name])
        cols = list(range(min(n_cols, X.shape[1])))
        out[name] = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, lambda: route_before(sampler, X, y, cols)), reps))
        out[name].update(chain_seconds=round(secs, 1), columns_timed=len(cols))
    return out


def _kernels_alone(sampler, X, reps):
    """``k_permimp`` (all columns, ``REPEATS`` repeats, with ``f``) and ``k_predict`` on the same rows and draws, each
    between its own events; the mean use-list length over ``m``."""
    import numpy as np

    from pymc_bart_amd.permutation import PRED, PermutationJob

    job = PermutationJob(sampler, X, None, None, REPEATS, None, None, None, "identity", None, SEED)
    res = _timing.resident_predictions(job)
    be = res.backend
    lib, mem = be.lib, be.mem
    n, D, K, q = min(job.n, 64 * 256), job.D, job.K, job.q   # (16 k rows: D q R K n doubles of scratch)
    permuted = lib.predict_permuted_entry_point()
    ms = {}
    for name in ("pgb_walk_kernel_ms", "pgb_permimp_kernel_ms"):
        ms[name] = getattr(lib.lib, name)
        ms[name].argtypes = [C.POINTER(C.c_double)]
    xd = mem.from_host(job.X[:n])
    fd, sd = mem.empty((D * K * n,), np.float64), mem.empty((D * q * REPEATS * K * n,), np.float64)
    xcols = mem.from_host(np.ascontiguousarray(job.X[:, job.cols].T))
    carr = job.pool.as_c()
    picks = np.arange(D, dtype=np.int32)
    took = {"k_predict": [], "k_permimp": []}
    with _timing.walk_timing():
        for _ in range(reps + 1):
            v = C.c_double()
            lib.check(lib.lib.pgb_predict(C.byref(carr), job.fidx.ctypes.data, D, job.m, mem.ptr(xd), n, job.p, job.p, None, 0,
                                          mem.ptr(fd), mem.stream_ptr), "pgb_predict")
            ms["pgb_walk_kernel_ms"](C.byref(v))
            took["k_predict"].append(v.value)
            lib.check(permuted(C.byref(carr), job.fidx.ctypes.data, D, job.m, mem.ptr(xd), n, job.p, job.p, mem.ptr(xcols), job.n,
                               0, job.cols.ctypes.data, q, REPEATS, SEED, picks.ctypes.data, D, mem.ptr(fd), PRED, mem.ptr(sd),
                               mem.stream_ptr), "pgb_predict_permuted")
            ms["pgb_permimp_kernel_ms"](C.byref(v))
            took["k_permimp"].append(v.value)
    took = {k: float(np.median(v[1:])) for k, v in took.items()}
    # the use lists, recounted: per (draw, column) the trees of the draw that use the column
    pool = job.pool.decoded() if hasattr(job.pool, "decoded") else job.pool
    uses = np.zeros((pool.n_trees, job.p), bool)
    tree_of = np.searchsorted(np.asarray(pool.node_off), np.arange(pool.total_nodes), side="right") - 1
    split = np.asarray(pool.var) >= 0
    uses[tree_of[split], np.asarray(pool.var)[split]] = True           # (a fit's trees hold no unreachable nodes)
    lin = ~split & (np.asarray(pool.svar) >= 0) & (np.asarray(pool.svar) < job.p)
    uses[tree_of[lin], np.asarray(pool.svar)[lin]] = True
    mean_len = float(uses[job.fidx].sum(axis=1).mean())
    return took, n, mean_len


def main(argv=None) -> int:
    ap = _timing.base_parser("permimp_timing.json", "cfg2", reps=3, baseline=True)
    ap.add_argument("--baseline-cols", type=int, default=5)
    args = ap.parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        _timing.print_baseline(baseline(names, args.reps, args.baseline_cols))
        return 0
    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import permutation_importance

    line = {"metric": "ms_per_call", "reps": args.reps, "repeats": REPEATS, "shapes": _timing.kept_shapes(args.out, names)}
    new = {}
    for name in names:
        shape = SHAPES[name]
        X, y, sampler, secs = _fit(shape)
        got = {}
        t = _timing.time_legs({"permutation_importance": lambda: got.__setitem__("new", permutation_importance(
            sampler, X, y, n_repeats=REPEATS, random_seed=SEED))}, args.reps)["permutation_importance"]
        k_ms, k_rows, mean_len = _kernels_alone(sampler, X, args.reps)
        some = list(range(min(2, X.shape[1])))
        before = route_before(sampler, X, y, some, 1)[:, :, 0]
        close = bool(np.allclose(got["new"]["mse_permuted"][:, some, 0], before, rtol=1e-9, atol=0.0))
        m = shape["m"]
        new[name] = {"shape": dict(shape, chain_seconds=round(secs, 1), columns=int(X.shape[1])), **t,
                     "kernel_rows": k_rows, "k_predict_ms": round(k_ms["k_predict"], 4), "k_permimp_ms": round(k_ms["k_permimp"], 4),
                     "k_permimp_over_k_predict": round(k_ms["k_permimp"] / k_ms["k_predict"], 3),
                     "k_predict_walks_for_the_same_work": int(X.shape[1]) * REPEATS,
                     "mean_use_list_length": round(mean_len, 3), "mean_use_list_length_over_m": round(mean_len / m, 5),
                     "mse_permuted_close_to_the_route_before": close}
        print(f"[timing_permimp] {name}: {json.dumps(new[name])}", file=sys.stderr, flush=True)
        del X, y, sampler, got
    base = None
    if args.baseline_root:
        base = _timing.run_baseline(__file__, args.baseline_root, ["--reps", str(args.reps), "--shapes", ",".join(names),
                                                                   "--baseline-cols", str(args.baseline_cols)])
    for name in names:
        row = new[name]
        if base is not None:
            b = base[name]
            scale = row["shape"]["columns"] / b["columns_timed"]
            bm = {k: v * scale for k, v in b["median_ms"].items()}
            spread = _timing.spread(b, LEGS) * scale
            row["baseline"] = {"what": "one bayes_r2 call per (column, repeat) on a host-permuted copy of X",
                               "measured_on": "a checkout of the parent commit, in a process of its own",
                               "has_permutation_module": base["has_permutation_module"], "scaled": True,
                               "scaled_by": round(scale, 3), "scaled_median_ms": {k: round(v, 1) for k, v in bm.items()}, **b}
            row["baseline_spread_ms_scaled"] = round(spread, 3)
            row["speedup_against_the_scaled_baseline"] = round(min(bm.values()) / row["median_ms"], 2)
            row["below_the_baseline_by_more_than_its_spread"] = bool(row["median_ms"] < min(bm.values()) - spread)
        line["shapes"][name] = row
    line["kernels"] = _timing.kernel_rows("k_permimp")
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
