#!/usr/bin/env python3
"""ms per call of PSIS-LOO on the device against pulling the pointwise matrix to the host, on one GPU.

On a cfg2-shaped fit (100 k x 50, m = 200, Normal with the chain's sigma per draw, D = 1000 draws of a real chain), the
public calls, each from host arrays to host results, alternating, after every leg has been warmed:

* ``loo``                      ``pymc_bart_amd.loo(...)``: the tree walk writes each block's matrix to device scratch,
                               ``k_psis`` smooths it there; 5 vectors of n reach the host,
* ``log_predictive_density``   the summary call (lppd / WAIC), for scale,
* ``matrix_to_host``           ``pointwise_log_likelihood(...)``: the ``(D, n)`` matrix through pageable memory -- what a
                               user had to do before running PSIS on the host.  THE BASELINE: with ``--baseline-root DIR``
                               it is timed in a process of its own on the package found in ``DIR`` (a built checkout of
                               the parent commit), twice (``matrix_to_host`` / ``matrix_to_host_again``) so that its
                               run-to-run spread is on record; without, on this tree (whose matrix call is the parent's).
* ``psis_kernel``              ``pgb_psis_rows`` alone on a resident matrix of the same shape, between two HIP events:
                               its share of ``loo``.

Required: ``loo`` <= ``matrix_to_host``.  Writes ``profiles/psis_timing.json`` (``--out``) with the kernel-resource row
of ``k_psis`` and prints it as one JSON line.

  python tools/psis_timing.py [--reps 5] [--draws 1000] [--small] [--baseline-root DIR] [--out FILE]
"""

from __future__ import annotations

import os
import sys
import tempfile

import _timing
from _timing import HERE

LEGS = ("matrix_to_host", "matrix_to_host_again")


def parser(default_out):
    """The arguments of this tool and of ``psis_expect_timing.py``: one cfg2-shaped fit, sized by flags."""
    ap = _timing.base_parser(default_out, baseline=True)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--tune", type=int, default=10)
    ap.add_argument("--particles", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="a tenth of the rows (a quick look, not the record)")
    return ap


def baseline_argv(args):
    return ["--reps", str(args.reps), "--draws", str(args.draws), "--tune", str(args.tune), "--particles",
            str(args.particles)] + (["--small"] if args.small else [])


def _fit(n, D, tune, particles):
    from pymc_bart_amd import NormalLikelihood
    from pymc_bart_amd.trees import PosteriorSampler

    f = _timing.fit(dict(n=n, draws=D), tune=tune, particles=particles)
    res = f.results[0]
    base, batches = res["history"]
    ps = PosteriorSampler.from_history(batches, base, f.op.m, 1)
    return {"X": f.X, "Y": f.Y, "m": f.op.m}, ps, {"sigma": res["sigma"]}, NormalLikelihood("sigma"), f.seconds


def baseline(args) -> dict:
    """The matrix call of the package on sys.path, timed twice per round."""
    import torch  # noqa: F401

    from pymc_bart_amd.pointwise import pointwise_log_likelihood

    w, ps, pts, lik, secs = _fit(args.n, args.draws, args.tune, args.particles)

    def matrix():
        pointwise_log_likelihood(ps, w["X"], w["Y"], lik, points=pts)

    out = _timing.by_statistic(_timing.time_legs(dict.fromkeys(LEGS, matrix), args.reps))
    import pymc_bart_amd

    pkg = os.path.dirname(os.path.abspath(pymc_bart_amd.__file__))
    out["package"] = os.path.relpath(pkg, HERE)
    out["has_loo"] = os.path.exists(os.path.join(pkg, "loo.py"))
    out["chain_seconds"] = round(secs, 1)
    return out


def main(argv=None) -> int:
    args = parser("psis_timing.json").parse_args(argv)
    args.n = 100_000 // (10 if args.small else 1)
    os.environ.setdefault("PGB_JIT_CACHE", tempfile.mkdtemp(prefix="pgb_jit_timing_"))
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        _timing.print_baseline(baseline(args))
        return 0
    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import log_predictive_density, loo
    from pymc_bart_amd.pointwise import pointwise_log_likelihood
    from pymc_bart_amd.sampler import default_backend

    loo_mod = sys.modules["pymc_bart_amd.loo"]
    w, ps, pts, lik, secs = _fit(args.n, args.draws, args.tune, args.particles)
    X, y = w["X"], w["Y"]
    import warnings

    warnings.simplefilter("ignore", UserWarning)
    last = {}

    def leg_loo():
        last["loo"] = loo(ps, X, y, lik, points=pts)

    def leg_lpd():
        last["lpd"] = log_predictive_density(ps, X, y, lik, points=pts)

    def leg_matrix():
        last["ll"] = pointwise_log_likelihood(ps, X, y, lik, points=pts)

    legs = {"loo": leg_loo, "log_predictive_density": leg_lpd}
    if not args.baseline_root:
        legs.update(dict.fromkeys(LEGS, leg_matrix))
    timed = _timing.by_statistic(_timing.time_legs(legs, args.reps))
    # the PSIS kernel alone, on the matrix of the same fit, resident
    ll = last.get("ll")
    if ll is None:
        ll = pointwise_log_likelihood(ps, X, y, lik, points=pts)
    be = default_backend()
    mem, lib = be.mem, be.lib
    D, n = ll.shape
    M = loo_mod.tail_length(D)
    md, od = mem.from_host(ll), mem.empty((2 * n,), np.float64)
    call = lib.psis_entry_point()
    psis_ms = _timing.events_ms(lambda: lib.check(call(mem.ptr(md), D, n, n, M, mem.ptr(od), mem.stream_ptr), "pgb_psis_rows"),
                                args.reps)
    same = bool(np.array_equal(mem.to_host(od).reshape(2, n)[0], last["loo"]["elpd_loo_i"]))
    del md, od, ll
    last.pop("ll", None)
    if args.baseline_root:
        base = _timing.run_baseline(__file__, args.baseline_root, baseline_argv(args))
        where = "a checkout of the parent commit, in a process of its own"
    else:
        base = {k: {leg: v[leg] for leg in LEGS} for k, v in timed.items()}
        where = "this tree (its matrix call is the parent's)"
    bm = base["median_ms"]
    spread = abs(bm["matrix_to_host"] - bm["matrix_to_host_again"])
    within = max(base["max_ms"][k] - base["min_ms"][k] for k in LEGS)
    med = timed["median_ms"]
    r = last["loo"]
    line = {"metric": "ms_per_call", "reps": args.reps, "small": bool(args.small),
            "shape": {"name": "cfg2-shaped", "n": n, "p": int(X.shape[1]), "m": w["m"], "draws": D, "tail_len": M,
                      "family": "normal", "chain_seconds": round(secs, 1)},
            "median_ms": {k: med[k] for k in ("loo", "log_predictive_density")},
            "min_ms": {k: timed["min_ms"][k] for k in ("loo", "log_predictive_density")},
            "baseline": {"measured_on": where, **base},
            "baseline_spread_ms": {"between_the_two_legs": round(spread, 3), "within_a_leg_max_minus_min": round(within, 3)},
            "psis_kernel_ms": round(psis_ms, 3), "psis_kernel_share_of_loo": round(psis_ms / med["loo"], 4),
            "psis_kernel_equals_loo_bits": same,
            "loo_result": {"elpd_loo": r["elpd_loo"], "p_loo": r["p_loo"], "n_high_k": r["n_high_k"],
                           "n_clamped": r["n_clamped"], "max_finite_k": float(np.max(r["pareto_k_i"][np.isfinite(r["pareto_k_i"])]))},
            "required": {"loo_le_matrix_to_host": bool(med["loo"] <= min(bm["matrix_to_host"], bm["matrix_to_host_again"]))},
            "kernels": _timing.kernel_rows(lambda k: k == "k_psis")}
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
