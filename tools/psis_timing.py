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

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fit(n, D, tune, particles):
    from pymc_bart_amd import BARTOp, NormalLikelihood
    from pymc_bart_amd.chains import sample_chain
    from pymc_bart_amd.trees import PosteriorSampler
    from pymc_bart_amd.workloads import cfg2

    w = cfg2(n=n)
    op = BARTOp(w["X"], w["Y"], m=w["m"])
    t0 = time.perf_counter()
    res = sample_chain(op, tune, D, num_particles=particles, random_seed=7, keep_draws=False)
    secs = time.perf_counter() - t0
    base, batches = res["history"]
    ps = PosteriorSampler.from_history(batches, base, w["m"], 1)
    return w, ps, {"sigma": res["sigma"]}, NormalLikelihood("sigma"), secs


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


def baseline(args) -> dict:
    """The matrix call of the package on sys.path, timed twice per round."""
    import torch  # noqa: F401

    from pymc_bart_amd.pointwise import pointwise_log_likelihood

    w, ps, pts, lik, secs = _fit(args.n, args.draws, args.tune, args.particles)

    def matrix():
        pointwise_log_likelihood(ps, w["X"], w["Y"], lik, points=pts)

    out = _time({"matrix_to_host": matrix, "matrix_to_host_again": matrix}, args.reps)
    import pymc_bart_amd

    pkg = os.path.dirname(os.path.abspath(pymc_bart_amd.__file__))
    out["package"] = os.path.relpath(pkg, HERE)
    out["has_loo"] = os.path.exists(os.path.join(pkg, "loo.py"))
    out["chain_seconds"] = round(secs, 1)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--tune", type=int, default=10)
    ap.add_argument("--particles", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="a tenth of the rows (a quick look, not the record)")
    ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit: the baseline's package")
    ap.add_argument("--baseline-leg", action="store_true", help=argparse.SUPPRESS)  # (the child process of --baseline-root)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "psis_timing.json"))
    args = ap.parse_args(argv)
    args.n = 100_000 // (10 if args.small else 1)
    os.environ.setdefault("PGB_JIT_CACHE", tempfile.mkdtemp(prefix="pgb_jit_timing_"))
    sys.path.insert(0, os.path.abspath(args.root))
    if args.baseline_leg:
        print("BASELINE " + json.dumps(baseline(args)))
        return 0
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import numpy as np
    import torch

    import occupancy_guard
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
        legs.update({"matrix_to_host": leg_matrix, "matrix_to_host_again": leg_matrix})
    timed = _time(legs, args.reps)
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
    ev = []
    for _ in range(args.reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lib.check(call(mem.ptr(md), D, n, n, M, mem.ptr(od), mem.stream_ptr), "pgb_psis_rows")
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    psis_ms = float(np.median(ev[1:]))
    same = bool(np.array_equal(mem.to_host(od).reshape(2, n)[0], last["loo"]["elpd_loo_i"]))
    del md, od, ll
    last.pop("ll", None)
    if args.baseline_root:
        cmd = [sys.executable, os.path.abspath(__file__), "--baseline-leg", "--root", os.path.abspath(args.baseline_root),
               "--reps", str(args.reps), "--draws", str(args.draws), "--tune", str(args.tune), "--particles",
               str(args.particles)] + (["--small"] if args.small else [])
        txt = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
        base = json.loads([ln for ln in txt.splitlines() if ln.startswith("BASELINE ")][-1][9:])
        where = "a checkout of the parent commit, in a process of its own"
    else:
        base = {k: {leg: v[leg] for leg in ("matrix_to_host", "matrix_to_host_again")} for k, v in timed.items()}
        where = "this tree (its matrix call is the parent's)"
    bm = base["median_ms"]
    spread = abs(bm["matrix_to_host"] - bm["matrix_to_host_again"])
    within = max(base["max_ms"][k] - base["min_ms"][k] for k in ("matrix_to_host", "matrix_to_host_again"))
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
            "kernels": [k for k in occupancy_guard.table() if k["kernel"] == "k_psis"]}
    with open(args.out, "w") as fh:
        json.dump(line, fh, indent=1)
        fh.write("\n")
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
