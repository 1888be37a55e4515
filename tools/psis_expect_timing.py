#!/usr/bin/env python3
"""ms per call of LOO-PIT on the device against pulling the two matrices it is made of to the host, on one GPU.

On the cfg2-shaped fit of ``tools/psis_timing.py`` (100 k x 50, m = 200, Normal with the chain's sigma per draw,
D = 1000 draws of a real chain), the public calls, each from host arrays to host results, alternating, after every leg
has been warmed:

* ``loo_pit``            ``pymc_bart_amd.loo_pit(...)``: per block the tree walk writes the pointwise matrix to device
                         scratch, ``pgb_predict`` + ``pgb_ppc_draw`` the replicated observations, ``k_psis_expect``
                         smooths and weights them there; a handful of vectors of n reach the host,
* ``loo``                for scale,
* ``matrices_to_host``   (a) THE BASELINE, the parent commit's only route: ``pointwise_log_likelihood(...)`` and
                         ``posterior_predictive(...)``, two ``(D, n)`` matrices through pageable memory, after which the
                         host would still have to smooth.  With ``--baseline-root DIR`` it is timed in a process of its
                         own on the package found in ``DIR`` (a built checkout of the parent commit), twice
                         (``matrices_to_host`` / ``matrices_to_host_again``) so that its run-to-run spread is on record;
                         without, on this tree (whose two calls are the parent's).
* ``kernels``            (b) ``pgb_psis_expect`` (both kinds) against ``pgb_psis_rows`` on the same resident matrices,
                         between two HIP events, alternating.

Writes ``profiles/psis_expect_timing.json`` (``--out``) with the kernel-resource rows and prints it as one JSON line.

  python tools/psis_expect_timing.py [--reps 5] [--draws 1000] [--small] [--baseline-root DIR] [--out FILE]
"""

from __future__ import annotations

import os
import sys
import tempfile

import _timing
from _timing import HERE
from psis_timing import _fit, baseline_argv, parser

LEGS = ("matrices_to_host", "matrices_to_host_again")


def baseline(args) -> dict:
    """The two matrix calls of the package on sys.path, timed twice per round."""
    import torch  # noqa: F401

    import pymc_bart_amd
    from pymc_bart_amd import pointwise_log_likelihood, posterior_predictive

    w, ps, pts, lik, secs = _fit(args.n, args.draws, args.tune, args.particles)

    def matrices():
        pointwise_log_likelihood(ps, w["X"], w["Y"], lik, points=pts)
        posterior_predictive(ps, w["X"], lik, points=pts, random_seed=0)

    out = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, matrices), args.reps))
    pkg = os.path.dirname(os.path.abspath(pymc_bart_amd.__file__))
    out["package"] = os.path.relpath(pkg, HERE)
    out["has_loo_pit"] = hasattr(pymc_bart_amd, "loo_pit")
    out["chain_seconds"] = round(secs, 1)
    return out


def main(argv=None) -> int:
    args = parser("psis_expect_timing.json").parse_args(argv)
    args.n = 100_000 // (10 if args.small else 1)
    os.environ.setdefault("PGB_JIT_CACHE", tempfile.mkdtemp(prefix="pgb_jit_timing_"))
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        _timing.print_baseline(baseline(args))
        return 0
    import warnings

    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import loo_pit, pointwise_log_likelihood, posterior_predictive
    from pymc_bart_amd.loo import loo
    from pymc_bart_amd.sampler import default_backend

    loo_mod = sys.modules["pymc_bart_amd.loo"]
    w, ps, pts, lik, secs = _fit(args.n, args.draws, args.tune, args.particles)
    X, y = w["X"], w["Y"]
    warnings.simplefilter("ignore", UserWarning)
    last = {}

    def leg_pit():
        last["pit"] = loo_pit(ps, X, y, lik, points=pts)

    def leg_loo():
        last["loo"] = loo(ps, X, y, lik, points=pts)

    def leg_matrices():
        last["ll"] = pointwise_log_likelihood(ps, X, y, lik, points=pts)
        last["yrep"] = posterior_predictive(ps, X, lik, points=pts, random_seed=0)

    legs = {"loo_pit": leg_pit, "loo": leg_loo}
    if not args.baseline_root:
        legs.update(dict.fromkeys(LEGS, leg_matrices))
    timed = _timing.by_statistic(_timing.time_legs(legs, args.reps))
    # (b) the kernels alone, on the two matrices of the same fit, resident
    if "ll" not in last:
        leg_matrices()
    ll, yrep = last.pop("ll"), last.pop("yrep")
    be = default_backend()
    mem, lib = be.mem, be.lib
    D, n = ll.shape
    M = loo_mod.tail_length(D)
    md, gd, yd = mem.from_host(ll), mem.from_host(yrep), mem.from_host(np.ascontiguousarray(y, np.float64))
    del ll, yrep
    od = mem.empty((4 * n,), np.float64)
    rows_call, expect_call = lib.psis_entry_point(), lib.psis_expect_entry_point()
    kernels = {
        "k_psis": lambda: lib.check(rows_call(mem.ptr(md), D, n, n, M, mem.ptr(od), mem.stream_ptr), "pgb_psis_rows"),
        "k_psis_expect<1> (PIT)": lambda: lib.check(expect_call(mem.ptr(md), D, n, n, M, mem.ptr(gd), n, mem.ptr(yd), 1,
                                                                mem.ptr(od), mem.stream_ptr), "pgb_psis_expect"),
        "k_psis_expect<0> (value)": lambda: lib.check(expect_call(mem.ptr(md), D, n, n, M, mem.ptr(gd), n, None, 0,
                                                                  mem.ptr(od), mem.stream_ptr), "pgb_psis_expect"),
    }
    kernel_ms = {k: round(v, 3) for k, v in _timing.events_ms(kernels, args.reps).items()}
    kernels["k_psis_expect<1> (PIT)"]()
    same = bool(np.array_equal(mem.to_host(od).reshape(4, n)[2], last["pit"]["loo_pit"]))
    del md, gd, od
    if args.baseline_root:
        base = _timing.run_baseline(__file__, args.baseline_root, baseline_argv(args))
        where = "a checkout of the parent commit, in a process of its own"
    else:
        base = {k: {leg: v[leg] for leg in LEGS} for k, v in timed.items()}
        where = "this tree (its two matrix calls are the parent's)"
    bm = base["median_ms"]
    spread = abs(bm["matrices_to_host"] - bm["matrices_to_host_again"])
    within = max(base["max_ms"][k] - base["min_ms"][k] for k in LEGS)
    med = timed["median_ms"]
    r = last["pit"]
    line = {"metric": "ms_per_call", "reps": args.reps, "small": bool(args.small),
            "shape": {"name": "cfg2-shaped", "n": n, "p": int(X.shape[1]), "m": w["m"], "draws": D, "tail_len": M,
                      "family": "normal", "chain_seconds": round(secs, 1)},
            "median_ms": {k: med[k] for k in ("loo_pit", "loo")},
            "min_ms": {k: timed["min_ms"][k] for k in ("loo_pit", "loo")},
            "baseline": {"measured_on": where, **base},
            "baseline_spread_ms": {"between_the_two_legs": round(spread, 3), "within_a_leg_max_minus_min": round(within, 3)},
            "baseline_minus_loo_pit_ms": round(min(bm["matrices_to_host"], bm["matrices_to_host_again"]) - med["loo_pit"], 3),
            "kernel_ms": kernel_ms,
            "kernel_ratio_to_k_psis": {k: round(v / kernel_ms["k_psis"], 4) for k, v in kernel_ms.items() if k != "k_psis"},
            "expect_kernel_equals_loo_pit_bits": same,
            "loo_pit_result": {"elpd_loo": r["elpd_loo"], "n_high_k": r["n_high_k"], "n_clamped": r["n_clamped"],
                               "mean_loo_pit": float(r["loo_pit"].mean()), "n_capped": r["n_capped"],
                               "n_exhausted": r["n_exhausted"]},
            "kernels": _timing.kernel_rows("k_psis")}
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
