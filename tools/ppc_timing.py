#!/usr/bin/env python3
"""ms per call of the posterior predictive summary on the device against what a user did before it, on one GPU.

Per shape, on a real Normal chain of ``sample_chain`` (data: ``workloads.cfg2``; the shapes of
``tools/rowsummary_timing.py``), from host arrays to host results, the median of ``--reps`` calls after one warm-up call:

* ``predictive_summary``  ``pymc_bart_amd.predictive_summary(sampler, X, NormalLikelihood("sigma"), points=...)`` with
                          its defaults (quantiles 3 / 50 / 97 %, 94 % HDI): per block of rows one ``pgb_predict`` into
                          device scratch, one ``pgb_ppc_draw`` in place and one ``pgb_row_summary``; ``(5 + 2) x n``
                          doubles reach the host.
* THE BASELINE            the path the parent commit offers: ``sample_posterior`` of all draws to the host, NumPy
                          ``Generator.normal`` noise with the draw's sigma on top, then ``mean(0)`` and ``np.quantile``
                          (no HDI: the baseline does less).  The code it runs is the parent's unchanged; it is timed
                          twice per round (``host`` / ``host_again``) so that its run-to-run spread is on record.
* ``k_ppc``               ``pgb_ppc_draw`` alone, in place on the resident predictions of the same shape, between two
                          events of the stream.

Shapes: ``plot`` (1000 rows x 10 columns, m = 50, 200 draws) and ``large`` (100 k x 50, m = 200, 1000 draws).  Writes
``profiles/ppc_timing.json`` (``--out``; shapes already in the file and not timed now are kept) with the kernel-resource
rows of ``k_ppc`` and prints it as one JSON line.  The one requirement: at the largest shape timed the device path is
not slower than the baseline (``not_slower_than_the_baseline``; the exit status says so).

  python tools/ppc_timing.py [--reps 5] [--shapes plot,large] [--out FILE]
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {
    "plot": dict(n=1000, p=10, m=50, draws=200),
    "large": dict(n=100_000, p=50, m=200, draws=1000),
}
QUANTILES = (0.03, 0.5, 0.97)
HDI_PROB = 0.94


def _fit(shape):
    from pymc_bart_amd import BARTOp
    from pymc_bart_amd.chains import sample_chain
    from pymc_bart_amd.utils import _get_posterior_sampler
    from pymc_bart_amd.workloads import cfg2

    w = cfg2(n=shape["n"], p=shape["p"], m=shape["m"])
    op = BARTOp(w["X"], w["Y"], m=w["m"])
    t0 = time.perf_counter()
    res = sample_chain(op, 10, shape["draws"], num_particles=10, random_seed=7, keep_draws=False)
    return w["X"], _get_posterior_sampler(op), res["sigma"], time.perf_counter() - t0


def _time(legs: dict, reps: int) -> dict:
    import numpy as np
    import torch

    for f in legs.values():
        f()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": {k: round(float(np.median(v)), 3) for k, v in ms.items()},
            "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
            "max_ms": {k: round(max(v), 3) for k, v in ms.items()}}


def on_the_host(sampler, X, sigma):
    """What a user does without the device path: every draw's predictions to the host, NumPy noise and quantiles."""
    import numpy as np

    pred = np.asarray(sampler.sample_posterior(X, list(range(sampler.n_draws)), None))  # (D, 1, n)
    flat = pred.reshape(pred.shape[0], -1)
    yrep = flat + np.random.default_rng(0).normal(0.0, 1.0, flat.shape) * sigma[:, None]
    return yrep.mean(axis=0), yrep.std(axis=0, ddof=1), np.quantile(yrep, QUANTILES, axis=0)


def _kernel_alone(sampler, X, sigma, reps):
    """``pgb_ppc_draw`` in place on the resident predictions of every draw at every row, by stream events."""
    import numpy as np
    import torch

    from pymc_bart_amd import NormalLikelihood, _abi, predictive

    job = predictive._Job(sampler, X, NormalLikelihood("sigma"), {"sigma": sigma}, None, None, None, 0)
    be = job.backend()
    lib, mem = be.lib, be.mem
    n, D, p = job.n, job.D, job.p
    xd = mem.from_host(job.X)
    md = mem.empty((D * n,), np.float64)
    carr = job.pool.as_c()
    lik = _abi.PpcLik()
    lik.family, lik.n_params, lik.params_host = _abi.FAMILIES["normal"], 1, job.params.ctypes.data
    flags = (C.c_int64 * 2)()
    call = lib.ppc_entry_point()
    ev = []
    for _ in range(reps + 1):
        lib.check(lib.lib.pgb_predict(C.byref(carr), job.fidx.ctypes.data, D, job.m, mem.ptr(xd), n, p, p, None, 0,
                                      mem.ptr(md), mem.stream_ptr), "pgb_predict")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lib.check(call(mem.ptr(md), D, 1, n, n, 0, C.byref(lik), 0, mem.ptr(md), n, None, None, flags, mem.stream_ptr),
                  "pgb_ppc_draw")
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    return float(np.median(ev[1:]))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="plot,large")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ppc_timing.json"))
    args = ap.parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import torch  # noqa: F401

    import occupancy_guard
    from pymc_bart_amd import NormalLikelihood, predictive_summary

    line = {"metric": "ms_per_call", "reps": args.reps, "quantiles": list(QUANTILES), "hdi_prob": HDI_PROB, "shapes": {}}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            line["shapes"] = {k: v for k, v in json.load(fh).get("shapes", {}).items() if k not in names}
    ok = True
    for name in names:
        shape = SHAPES[name]
        X, sampler, sigma, secs = _fit(shape)
        lik, pts = NormalLikelihood("sigma"), {"sigma": sigma}
        t = _time({"predictive_summary": lambda: predictive_summary(sampler, X, lik, points=pts, quantiles=QUANTILES,
                                                                    hdi_prob=HDI_PROB),
                   "host": lambda: on_the_host(sampler, X, sigma), "host_again": lambda: on_the_host(sampler, X, sigma)},
                  args.reps)
        k_ms = _kernel_alone(sampler, X, sigma, args.reps)
        dev = t["median_ms"]["predictive_summary"]
        base = min(t["median_ms"]["host"], t["median_ms"]["host_again"])
        spread = max(abs(t["median_ms"]["host"] - t["median_ms"]["host_again"]),
                     max(t["max_ms"][k] - t["min_ms"][k] for k in ("host", "host_again")))
        row = {"shape": dict(shape, chain_seconds=round(secs, 1)), "median_ms": dev, "min_ms": t["min_ms"]["predictive_summary"],
               "max_ms": t["max_ms"]["predictive_summary"],
               "baseline": {"what": "sample_posterior to the host + Generator.normal + mean / std / np.quantile",
                            "median_ms": {k: t["median_ms"][k] for k in ("host", "host_again")},
                            "min_ms": {k: t["min_ms"][k] for k in ("host", "host_again")},
                            "max_ms": {k: t["max_ms"][k] for k in ("host", "host_again")}},
               "baseline_spread_ms": round(spread, 3), "speedup": round(base / dev, 2),
               "not_slower_than_the_baseline": bool(dev <= base),
               "k_ppc_ms": round(k_ms, 4), "k_ppc_share_of_the_call": round(k_ms / dev, 4),
               "k_ppc_values_per_s": round(X.shape[0] * sampler.n_draws / k_ms * 1e3, 1)}
        print(f"[ppc_timing] {name}: {json.dumps(row)}", file=sys.stderr, flush=True)
        line["shapes"][name] = row
        del X, sampler
    largest = max(names, key=lambda s: SHAPES[s]["n"] * SHAPES[s]["draws"])
    ok = line["shapes"][largest]["not_slower_than_the_baseline"]
    line["kernels"] = [k for k in occupancy_guard.table() if k["kernel"].startswith("k_ppc")]
    with open(args.out, "w") as fh:
        json.dump(line, fh, indent=1)
        fh.write("\n")
    print(json.dumps(line))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
