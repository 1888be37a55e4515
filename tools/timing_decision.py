#!/usr/bin/env python3
"""ms per call of the optimal arm and policy value on the device against the route before it, on one GPU.

On a real Normal chain of ``sample_chain`` (data: ``workloads.cfg2``; the default shape is cfg2-shaped: 100 k x 50,
m = 200, 32 draws), A = 4 arms on column 0, 8 groups of contiguous rows, from host arrays to host results, the median of
``--reps`` calls after one warm-up call:

* ``optimal_arm``   per block of rows one ``pgb_predict``, one ``pgb_predict_arms`` and one ``pgb_arm_decide``; the
                    per-row results and ``(draws, groups, arms)`` doubles reach the host.
* THE BASELINE      the route before it: A copies of ``X`` with the column set to the arm's value, ``sample_posterior`` of
                    each to the host -- ``(draws, n)`` doubles per arm -- and NumPy for the argmax, the means over the
                    draws and the group sums.  With ``--baseline-root DIR`` it runs in a process of its own on the package
                    found in ``DIR`` (a built checkout of the parent commit), twice (``host`` / ``host_again``) so that
                    its run-to-run spread is on record.
* ``k_arms``        against ``k_predict`` on the same rows and draws, each between its own stream events
                    (``PGB_WALK_TIMING``), and the mean length of a union use list over ``m``: the kernel visits that
                    share of the trees A + 1 times where the baseline visits all of them A times.

Writes ``profiles/decision_timing.json`` (``--out``) with the kernel-resource rows of the ``k_arms*`` kernels and prints
it as one JSON line.  Nothing is required of the figures.
(The file is not named ``*_timing.py``: ``tests/test_timing_tools.py`` holds the list of those; this tool's own ``--help``
is checked in ``tests/test_decision.py``.)

  python tools/timing_decision.py [--reps 3] [--shapes cfg2] [--baseline-root DIR] [--out FILE]
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
N_ARMS, N_GROUPS, COL = 4, 8, 0
LEGS = ("host", "host_again")


def _fit(shape):
    from pymc_bart_amd.utils import _get_posterior_sampler

    f = _timing.fit(shape)
    return f.X, _get_posterior_sampler(f.op), f.seconds


def arms_of(X):
    """Four values across the bulk of the column."""
    import numpy as np

    return np.quantile(X[:, COL], [0.2, 0.4, 0.6, 0.8])


def groups_of(n):
    import numpy as np

    return (np.arange(n) * N_GROUPS) // n


def route_before(sampler, X, arms, groups, n_draws):
    """A copies of ``X``, ``sample_posterior`` of each to the host, NumPy for the rest -> the per-row and per-draw
    results of ``optimal_arm`` (up to the order of the sums)."""
    import numpy as np

    preds = []
    for a in arms:
        Xa = X.copy()
        Xa[:, COL] = a
        preds.append(np.asarray(sampler.sample_posterior(Xa, list(range(n_draws)), None)).reshape(-1, X.shape[0]))
    u = np.stack(preds)                                                   # (A, D, n)
    A, D, n = u.shape
    best = np.argmax(u, axis=0)
    umax = np.take_along_axis(u, best[None], axis=0)[0]
    su = u.sum(axis=1)
    bayes = np.argmax(su, axis=0)
    onehot = np.zeros((N_GROUPS, n))
    onehot[groups, np.arange(n)] = 1.0
    W = onehot.sum(axis=1)
    return {"p_best": np.stack([(best == a).mean(axis=0) for a in range(A)], axis=1), "mean_utility": (su / D).T,
            "expected_regret": ((umax[None] - u).sum(axis=1) / D).T, "bayes_arm": bayes,
            "value_optimal": umax @ onehot.T / W, "value_bayes": u[bayes, :, np.arange(n)].T @ onehot.T / W,
            "value_arm": np.stack([u[a] @ onehot.T / W for a in range(A)], axis=-1),
            "share_best": np.stack([(best == a).astype(np.float64) @ onehot.T / W for a in range(A)], axis=-1)}


def baseline(names, reps) -> dict:
    """The route before on the package found on sys.path, timed twice per round, at every shape."""
    import torch  # noqa: F401

    import pymc_bart_amd

    # (the parent commit has no pymc_bart_amd/decision.py: the mark that the baseline's package is not this tree's)
    out = {"has_decision_module": os.path.exists(os.path.join(os.path.dirname(pymc_bart_amd.__file__), "decision.py"))}
    for name in names:
        X, sampler, secs = _fit(SHAPES[name])
        arms, groups = arms_of(X), groups_of(X.shape[0])
        out[name] = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, lambda: route_before(sampler, X, arms, groups, SHAPES[name]["draws"])), reps))
        out[name].update(chain_seconds=round(secs, 1))
    return out


def _kernels_alone(sampler, X, arms, reps):
    """``k_arms`` and ``k_predict`` on the same rows and draws, each between its own events; the decide kernels; the
    mean union-list length."""
    import numpy as np

    from pymc_bart_amd.decision import ArmsJob

    job = ArmsJob(sampler, X, [COL], arms, None, None)
    job.take_history()
    be, (predict_arms, decide, _, query) = job.hip()
    lib, mem = be.lib, be.mem
    n, D, K, A = min(job.n, 64 * 1024), job.D, job.K, job.A
    walk_ms = lib.lib.pgb_walk_kernel_ms
    walk_ms.argtypes = [C.POINTER(C.c_double)]
    xd = mem.from_host(job.X[:n])
    fd, od = mem.empty((D * K * n,), np.float64), mem.empty((A * D * K * n,), np.float64)
    wd, gd = mem.from_host(np.ones(n)), mem.from_host(groups_of(n).astype(np.int32))
    ws = mem.empty((int(query(D, N_GROUPS, A)) // 8,), np.float64)
    nd, md, rd, bd = (mem.empty((A * n,), np.int32), mem.empty((A * n,), np.float64), mem.empty((A * n,), np.float64),
                      mem.empty((n,), np.int32))
    lens = np.zeros(D, np.int32)
    carr = job.pool.as_c()
    took = {"k_predict": [], "k_arms": [], "decide_kernels": []}
    with _timing.walk_timing():
        for _ in range(reps + 1):
            v = C.c_double()
            lib.check(lib.lib.pgb_predict(C.byref(carr), job.fidx.ctypes.data, D, job.m, mem.ptr(xd), n, job.p, job.p, None, 0,
                                          mem.ptr(fd), mem.stream_ptr), "pgb_predict")
            walk_ms(C.byref(v))
            took["k_predict"].append(v.value)
            lib.check(predict_arms(C.byref(carr), job.fidx.ctypes.data, D, job.m, mem.ptr(xd), n, job.p, job.p,
                                   job.cols.ctypes.data, job.s, job.arms.ctypes.data, A, job.picks.ctypes.data, D, mem.ptr(fd),
                                   mem.ptr(od), lens.ctypes.data, mem.stream_ptr), "pgb_predict_arms")
            lib.check(decide(mem.ptr(od), D * K * n, K * n, D, A, n, mem.ptr(wd), mem.ptr(gd), None, None, None, 1.0, 0, N_GROUPS,
                             0, 1, mem.ptr(ws), mem.ptr(nd), mem.ptr(md), mem.ptr(rd), mem.ptr(bd), mem.stream_ptr), "pgb_arm_decide")
            k_arms, k_decide = lib.arms_kernel_ms()
            took["k_arms"].append(k_arms)
            took["decide_kernels"].append(k_decide)
    return {k: float(np.median(v[1:])) for k, v in took.items()}, n, float(lens.mean())


def main(argv=None) -> int:
    ap = _timing.base_parser("decision_timing.json", "cfg2", reps=3, baseline=True)
    args = ap.parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        _timing.print_baseline(baseline(names, args.reps))
        return 0
    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import optimal_arm

    line = {"metric": "ms_per_call", "reps": args.reps, "arms": N_ARMS, "groups": N_GROUPS, "column": COL,
            "shapes": _timing.kept_shapes(args.out, names)}
    new = {}
    for name in names:
        shape = SHAPES[name]
        X, sampler, secs = _fit(shape)
        arms, groups = arms_of(X), groups_of(X.shape[0])
        got = {}
        t = _timing.time_legs({"optimal_arm": lambda: got.__setitem__("new", optimal_arm(sampler, X, [COL], arms, groups=groups))},
                              args.reps)["optimal_arm"]
        k_ms, k_rows, mean_len = _kernels_alone(sampler, X, arms, args.reps)
        before = route_before(sampler, X, arms, groups, shape["draws"])
        close = bool(all(np.allclose(got["new"][key], before[key], rtol=0.0, atol=1e-9)
                         for key in ("mean_utility", "value_optimal", "value_arm")))
        agree = float(np.mean(got["new"]["bayes_arm"] == before["bayes_arm"]))
        m = shape["m"]
        new[name] = {"shape": dict(shape, chain_seconds=round(secs, 1)), **t, "kernel_rows": k_rows,
                     "k_predict_ms": round(k_ms["k_predict"], 4), "k_arms_ms": round(k_ms["k_arms"], 4),
                     "decide_kernels_ms": round(k_ms["decide_kernels"], 4),
                     "k_arms_over_k_predict": round(k_ms["k_arms"] / k_ms["k_predict"], 3),
                     "k_predict_walks_for_the_same_work": N_ARMS,
                     "mean_union_list_length": round(mean_len, 3), "mean_union_list_length_over_m": round(mean_len / m, 5),
                     "close_to_the_route_before": close, "bayes_arm_agreement_with_the_route_before": round(agree, 6)}
        print(f"[timing_decision] {name}: {json.dumps(new[name])}", file=sys.stderr, flush=True)
        del X, sampler, got
    base = None
    if args.baseline_root:
        base = _timing.run_baseline(__file__, args.baseline_root, ["--reps", str(args.reps), "--shapes", ",".join(names)])
    for name in names:
        row = new[name]
        if base is not None:
            b = base[name]
            spread = _timing.spread(b, LEGS)
            row["baseline"] = {"what": "A copies of X, sample_posterior of each to the host, NumPy for the argmax, the means and "
                                       "the group sums",
                               "measured_on": "a checkout of the parent commit, in a process of its own",
                               "has_decision_module": base["has_decision_module"], **b}
            row["baseline_spread_ms"] = round(spread, 3)
            row["speedup_against_the_baseline"] = round(min(b["median_ms"].values()) / row["median_ms"], 2)
            row["below_the_baseline_by_more_than_its_spread"] = bool(row["median_ms"] < min(b["median_ms"].values()) - spread)
        line["shapes"][name] = row
    line["kernels"] = _timing.kernel_rows("k_arms")
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
