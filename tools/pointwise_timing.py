#!/usr/bin/env python3
"""ms per call of the fused pointwise log-likelihood against what the library offered before it, on one GPU.

For each shape, on the trees of a short real chain and resident device buffers, all legs in ONE process, alternating,
each call ended by a device synchronise (host clock), after every leg has been warmed:

* ``predict``         (a)  ``pgb_predict`` alone on the same trees, rows and draws; timed twice per round
                           (``predict`` / ``predict_again``) so that the run-to-run spread is on record,
* ``unfused``         (b)  the device path a user could assemble before: ``pgb_predict`` into a ``(D, K, n)`` buffer, then
                           one elementwise pass over it (``pgb_compiled_probe`` with the density restated as a body),
* ``fused_matrix``         ``pgb_pointwise_loglik`` writing the ``(D, n)`` matrix,
* ``fused_summary``        ``pgb_pointwise_loglik`` writing ``row_stats[3][n]`` only.

Shapes: cfg2-shaped (100 k x 50, m = 200, Normal, D = 100) and cfg4-shaped (1 M x 100, m = 200, probit, D = 32).
``--ab-lib PATH``: a second build of the library (e.g. one with ``-DPGB_PW_LDS_TABLES``) whose fused legs are timed in
the same alternation (``ab_fused_matrix`` / ``ab_fused_summary``): the table-placement A/B.
(That build: the ``hipcc`` line of ``__graft_entry__.build()`` for ``libpgbart_hip.so`` -- its flags and its
``-DPGB_HEADERS_HASH`` -- plus ``-DPGB_PW_LDS_TABLES``, written to ``build/variants/libpgbart_hip_pwlds.so``.)

Writes ``profiles/pointwise_timing.json`` (``--out``) and prints it as one JSON line.

  python tools/pointwise_timing.py [--reps 7] [--shapes cfg2,cfg4] [--small] [--ab-lib PATH] [--out FILE]
"""

from __future__ import annotations

import ctypes as C
import os
import sys
import tempfile

import numpy as np

import _timing
from _timing import HERE as ROOT

sys.path.insert(0, ROOT)

NORMAL_BODY = "double z = (y - mu) / s;  return (-log(s) - 9.1893853320467274e-01) - 0.5 * (z * z);"
PROBIT_BODY = "return log_ndtr(y > 0.5 ? mu : -mu);"


def _probe_sampler(body, names, values):
    """A tiny sampler of the compiled family: the handle pgb_compiled_probe needs."""
    from pymc_bart_amd import CompiledLikelihood
    from pymc_bart_amd.sampler import PyBartSettings, PySampler, default_backend

    rng = np.random.default_rng(0)
    X, Y = rng.uniform(0, 1, (256, 2)), rng.normal(0, 1, 256)
    st = PyBartSettings.from_data(X, Y, m=2, num_particles=4, seed=1, family="compiled")
    s = PySampler(st, X, Y, np.zeros(2, np.int32), np.ones(2), backend=default_backend())
    s.set_compiled_likelihood(CompiledLikelihood(body, params=dict(zip(names, values))))
    s.set_likelihood(list(values))
    return s


def time_shape(name, workload, n, D, family, reps, tune, particles, ab_lib=None) -> dict:
    import torch

    from pymc_bart_amd import BernoulliLikelihood, NormalLikelihood, _abi
    from pymc_bart_amd.sampler import default_backend
    from pymc_bart_amd.trees import PosteriorSampler

    be = default_backend()
    lib, mem = be.lib, be.mem
    lik = NormalLikelihood("sigma") if family == "normal" else BernoulliLikelihood("probit")
    f = _timing.fit(dict(workload=workload, n=n, draws=D, likelihood=None if family == "normal" else lik), tune=tune,
                    particles=particles)
    res, m = f.results[0], f.op.m
    ps = PosteriorSampler.from_history(res["history"][1], res["history"][0], m, 1)
    X, y = np.ascontiguousarray(f.X, np.float64), np.ascontiguousarray(f.Y, np.float64)
    n, p = X.shape
    fidx = np.ascontiguousarray(ps.forest_idx[:D], np.int32)
    carr = ps.pool.as_c()
    sigma = float(np.median(res["sigma"])) if family == "normal" else 1.0
    params = np.full((D, 1), sigma)                       # (one sigma for every draw: what the probe's body can take)
    xd, yd = mem.from_host(X), mem.from_host(y)
    yrep = yd.repeat(D)                                   # the unfused pass reads y next to the (D, n) buffer
    mu = mem.empty((D * n,), np.float64)
    ll_unfused = mem.empty((D * n,), np.float64)
    ll = mem.empty((D * n,), np.float64)
    stats = mem.empty((3 * n,), np.float64)
    probe_s = _probe_sampler(NORMAL_BODY, ["s"], [sigma]) if family == "normal" else _probe_sampler(PROBIT_BODY, [], [])
    probe = probe_s.backend.lib.compiled_probe_entry_point()
    plik = _abi.PointwiseLik()
    plik.family = _abi.FAMILIES[lik.family]
    plik.n_params = 1 if family == "normal" else 0
    plik.params_host = params.ctypes.data if family == "normal" else None
    plik.y_dev = mem.ptr(yd)
    stream = mem.stream_ptr
    nc = C.c_int64(0)

    def predict():
        lib.check(lib.lib.pgb_predict(C.byref(carr), fidx.ctypes.data, D, m, mem.ptr(xd), n, p, p, None, 0, mem.ptr(mu),
                                      stream), "pgb_predict")

    def unfused():
        predict()
        probe_s.backend.lib.check(probe(probe_s._h, mem.ptr(yrep), mem.ptr(mu), None, D * n, mem.ptr(ll_unfused)),
                                  "pgb_compiled_probe")

    def fused(which_lib, matrix):
        call = which_lib.pointwise_entry_point()

        def run():
            which_lib.check(call(C.byref(carr), fidx.ctypes.data, D, m, mem.ptr(xd), n, p, p, C.byref(plik),
                                 mem.ptr(ll) if matrix else None, None if matrix else mem.ptr(stats), C.byref(nc),
                                 stream), "pgb_pointwise_loglik")
        return run

    legs = {"predict": predict, "unfused": unfused, "fused_matrix": fused(lib, True),
            "fused_summary": fused(lib, False), "predict_again": predict}
    if ab_lib is not None:
        legs["ab_fused_matrix"] = fused(ab_lib, True)
        legs["ab_fused_summary"] = fused(ab_lib, False)
    for leg in legs.values():                             # warm every shape (and once more in time_legs)
        leg()
    torch.cuda.synchronize()
    same = bool(torch.equal(ll, ll_unfused))
    t = _timing.time_legs(legs, reps)
    med = {k: v["median_ms"] for k, v in t.items()}
    spread = abs(med["predict"] - med["predict_again"])
    worst = max(t[k]["max_ms"] - t[k]["min_ms"] for k in ("predict", "predict_again"))
    out = {"shape": name, "n": n, "p": p, "m": m, "draws": D, "family": lik.family, "chain_seconds": round(f.seconds, 1),
           "median_ms": med, "min_ms": {k: v["min_ms"] for k, v in t.items()},
           "predict_spread_ms": {"between_the_two_legs": round(spread, 3), "within_a_leg_max_minus_min": round(worst, 3)},
           "fused_matrix_equals_unfused_bits": same, "n_clamped": int(nc.value),
           "fused_summary_over_predict": round(med["fused_summary"] / med["predict"], 3),
           "required": {
               "fused_summary_le_unfused": bool(med["fused_summary"] <= med["unfused"]),
               "fused_matrix_le_unfused": bool(med["fused_matrix"] <= med["unfused"]),
               "summary_margin_beyond_predict_spread": bool(med["unfused"] - med["fused_summary"] > spread),
               "matrix_margin_beyond_predict_spread": bool(med["unfused"] - med["fused_matrix"] > spread)}}
    del probe_s
    return out


def main(argv=None) -> int:
    ap = _timing.base_parser("pointwise_timing.json", "cfg2,cfg4", reps=7)
    ap.add_argument("--tune", type=int, default=10)
    ap.add_argument("--particles", type=int, default=10)
    ap.add_argument("--small", action="store_true", help="a tenth of the rows (a quick look, not the record)")
    ap.add_argument("--ab-lib", default=None, help="a second build of the library for the table-placement A/B")
    args = ap.parse_args(argv)
    os.environ.setdefault("PGB_JIT_CACHE", tempfile.mkdtemp(prefix="pgb_jit_timing_"))
    from pymc_bart_amd import _abi

    import torch  # noqa: F401  (first: the libraries share its HIP runtime)

    ab = _abi.PGBLibrary(args.ab_lib) if args.ab_lib else None
    scale = 10 if args.small else 1
    shapes = []
    for s in args.shapes.split(","):
        if s == "cfg2":
            shapes.append(time_shape("cfg2-shaped", "cfg2", 100_000 // scale, 100, "normal", args.reps, args.tune,
                                     args.particles, ab))
        elif s == "cfg4":
            shapes.append(time_shape("cfg4-shaped", "cfg4", 1_000_000 // scale, 32, "bernoulli_probit", args.reps,
                                     args.tune, args.particles, ab))
    line = {"metric": "ms_per_call", "reps": args.reps, "small": bool(args.small), "ab_lib": args.ab_lib,
            "shapes": shapes, "kernels": _timing.kernel_rows(("k_pointwise", "k_predict"))}
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
