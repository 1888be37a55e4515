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

import ctypes as C
import json
import sys

import _timing
from _timing import HERE

SHAPES = {
    "plot": dict(n=1000, p=10, m=50, draws=200),
    "large": dict(n=100_000, p=50, m=200, draws=1000),
}
QUANTILES = (0.03, 0.5, 0.97)
HDI_PROB = 0.94
LEGS = ("host", "host_again")


def on_the_host(sampler, X, sigma):
    """What a user does without the device path: every draw's predictions to the host, NumPy noise and quantiles."""
    import numpy as np

    pred = np.asarray(sampler.sample_posterior(X, list(range(sampler.n_draws)), None))  # (D, 1, n)
    flat = pred.reshape(pred.shape[0], -1)
    yrep = flat + np.random.default_rng(0).normal(0.0, 1.0, flat.shape) * sigma[:, None]
    return yrep.mean(axis=0), yrep.std(axis=0, ddof=1), np.quantile(yrep, QUANTILES, axis=0)


def _kernel_alone(sampler, X, sigma, reps):
    """``pgb_ppc_draw`` in place on the resident predictions of every draw at every row, by stream events."""
    from pymc_bart_amd import NormalLikelihood, _abi, predictive

    job = predictive._Job(sampler, X, NormalLikelihood("sigma"), {"sigma": sigma}, None, None, None, 0)
    res = _timing.resident_predictions(job)
    lib, mem, md = res.backend.lib, res.backend.mem, res.pred
    n, D = job.n, job.D
    lik = _abi.PpcLik()
    lik.family, lik.n_params, lik.params_host = _abi.FAMILIES["normal"], 1, job.params.ctypes.data
    flags = (C.c_int64 * 2)()
    call = lib.ppc_entry_point()
    return _timing.events_ms(lambda: lib.check(call(mem.ptr(md), D, 1, n, n, 0, C.byref(lik), 0, mem.ptr(md), n, None, None,
                                                    flags, mem.stream_ptr), "pgb_ppc_draw"), reps, before=res.fill)


def main(argv=None) -> int:
    args = _timing.base_parser("ppc_timing.json", "plot,large").parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, HERE)
    import torch  # noqa: F401

    from pymc_bart_amd import NormalLikelihood, predictive_summary
    from pymc_bart_amd.utils import _get_posterior_sampler

    line = {"metric": "ms_per_call", "reps": args.reps, "quantiles": list(QUANTILES), "hdi_prob": HDI_PROB,
            "shapes": _timing.kept_shapes(args.out, names)}
    for name in names:
        shape = SHAPES[name]
        f = _timing.fit(shape)
        X, sampler, sigma = f.X, _get_posterior_sampler(f.op), f.results[0]["sigma"]
        lik, pts = NormalLikelihood("sigma"), {"sigma": sigma}
        t = _timing.time_legs({"predictive_summary": lambda: predictive_summary(sampler, X, lik, points=pts,
                                                                                quantiles=QUANTILES, hdi_prob=HDI_PROB),
                               **dict.fromkeys(LEGS, lambda: on_the_host(sampler, X, sigma))}, args.reps)
        k_ms = _kernel_alone(sampler, X, sigma, args.reps)
        host = _timing.by_statistic(t, LEGS)
        dev = t["predictive_summary"]["median_ms"]
        base = min(host["median_ms"].values())
        row = {"shape": dict(shape, chain_seconds=round(f.seconds, 1)), **t["predictive_summary"],
               "baseline": {"what": "sample_posterior to the host + Generator.normal + mean / std / np.quantile", **host},
               "baseline_spread_ms": round(_timing.spread(host, LEGS), 3), "speedup": round(base / dev, 2),
               "not_slower_than_the_baseline": bool(dev <= base),
               "k_ppc_ms": round(k_ms, 4), "k_ppc_share_of_the_call": round(k_ms / dev, 4),
               "k_ppc_values_per_s": round(X.shape[0] * sampler.n_draws / k_ms * 1e3, 1)}
        print(f"[ppc_timing] {name}: {json.dumps(row)}", file=sys.stderr, flush=True)
        line["shapes"][name] = row
        del X, sampler, f
    largest = max(names, key=lambda s: SHAPES[s]["n"] * SHAPES[s]["draws"])
    ok = line["shapes"][largest]["not_slower_than_the_baseline"]
    line["kernels"] = _timing.kernel_rows("k_ppc")
    _timing.write(args.out, line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
