#!/usr/bin/env python3
"""ms per call of the chain diagnostics on the device against what a user did before them, on one GPU.

Per shape, on real chains of ``sample_chain`` (data: ``workloads.cfg2``), from host arrays to host results, the median
of ``--reps`` calls after one warm-up call:

* ``convergence``           ``pymc_bart_amd.convergence(sampler, X)``: per block of rows one ``pgb_predict`` into device
                            scratch and one ``pgb_chain_diag`` on it; ``10 x n`` doubles reach the host.
* THE ROUTE BEFORE IT       ``sample_posterior`` of all draws to the host (timed in full), then R-hat and the ESS column
                            by column with NumPy / SciPy (``tests/_diag_numpy.py``: ranks, ``ndtri``, FFT
                            autocovariances -- what ArviZ does).  With more than ``--host-rows`` rows the NumPy part is
                            timed on that many rows and scaled to all of them; the file says which was done.  Timed
                            ``--host-reps`` times, no warm-up.  It uses nothing of ``pymc_bart_amd.diagnostics``.
* ``k_chain_diag``          ``pgb_chain_diag`` alone on the resident predictions of the same shape, between two events
                            of the stream (the upload of the z table included).
* ``relative_efficiency``   against ``pointwise_log_likelihood`` of all draws to the host (the matrix r_eff would
                            otherwise be computed from; the host's own ESS of it is not timed).

Shapes: ``small`` (2000 rows x 10 columns, m = 50, 4 chains x 250 draws) and ``cfg2`` (100 k x 50, m = 200, 4 chains x
1000 draws).  Writes ``profiles/diag_timing.json`` (``--out``; shapes already in the file and not timed now are kept)
with the kernel-resource row of ``k_chain_diag`` and prints it as one JSON line.  Nothing is required of the figures.

  python tools/diag_timing.py [--reps 3] [--host-reps 1] [--host-rows 2000] [--shapes small,cfg2] [--out FILE]
"""

from __future__ import annotations

import json
import os
import sys

import _timing
from _timing import HERE

SHAPES = {
    "small": dict(n=2000, p=10, m=50, chains=4, draws=250),
    "cfg2": dict(n=100_000, p=50, m=200, chains=4, draws=1000),
}


def _kernel_alone(sampler, X, n_chains, npc, reps):
    """``pgb_chain_diag`` on the resident predictions of every draw at every row, by stream events."""
    import numpy as np

    from pymc_bart_amd import diagnostics, summary

    job = summary.SummaryJob(sampler, X, None, None, None, "identity", None, None)
    res = _timing.resident_predictions(job)
    lib, mem = res.backend.lib, res.backend.mem
    n, K = job.n, job.K
    S = diagnostics.kept_draws(n_chains, npc)
    z = diagnostics.z_table(S)
    od = mem.empty((diagnostics.NOUT * K * n,), np.float64)
    call = lib.chain_diag_entry_point()
    ms = _timing.events_ms(lambda: lib.check(call(mem.ptr(res.pred), n_chains, npc, K * n, K * n, 0, diagnostics.ALL,
                                                  z.ctypes.data, 1.0 / np.log10(S), mem.ptr(od), mem.stream_ptr),
                                             "pgb_chain_diag"), reps)
    return ms, mem.to_host(od).reshape(diagnostics.NOUT, K, n)


def main(argv=None) -> int:
    ap = _timing.base_parser("diag_timing.json", "small,cfg2", reps=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-rows", type=int, default=2000)
    args = ap.parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path[:0] = [HERE, os.path.join(HERE, "tests")]
    import numpy as np
    import torch  # noqa: F401

    import _diag_numpy as restatement
    from pymc_bart_amd import NormalLikelihood, convergence, pointwise_log_likelihood, relative_efficiency
    from pymc_bart_amd.utils import _get_posterior_sampler

    def one(f, reps, warm=True):
        return _timing.time_legs({"leg": f}, reps, warm)["leg"]

    line = {"metric": "ms_per_call", "reps": args.reps, "host_reps": args.host_reps,
            "shapes": _timing.kept_shapes(args.out, names)}
    for name in names:
        shape = SHAPES[name]
        f = _timing.fit(shape, chains=shape["chains"])
        X, y, sampler, secs = f.X, np.asarray(f.Y, np.float64), _get_posterior_sampler(f.op), f.seconds
        pts, lik = {"sigma": np.concatenate([c["sigma"] for c in f.results])}, NormalLikelihood("sigma")
        n, nc, npc = X.shape[0], shape["chains"], shape["draws"]
        last = {}

        def leg_convergence():
            last["res"] = convergence(sampler, X)

        def leg_reff():
            last["reff"] = relative_efficiency(sampler, X, y, lik, points=pts)

        row = {"shape": dict(shape, chain_seconds=round(secs, 1)), "convergence": one(leg_convergence, args.reps)}
        k_ms, stats = _kernel_alone(sampler, X, nc, npc, args.reps)
        res = last["res"]
        row["k_chain_diag_ms"] = round(k_ms, 3)
        row["k_chain_diag_share_of_the_call"] = round(k_ms / row["convergence"]["median_ms"], 4)
        row["k_chain_diag_columns_per_s"] = round(n * sampler.n_outputs / k_ms * 1e3, 1)
        row["k_chain_diag_equals_the_call_bits"] = bool(np.array_equal(stats[2].T, res["ess_bulk"])
                                                        and np.array_equal(stats[6].T, res["mean"]))
        row["result"] = {"max_rhat": float(np.max(res["rhat"])), "min_ess_bulk": float(np.min(res["ess_bulk"])),
                         "min_ess_tail": float(np.min(res["ess_tail"])), "n_high_rhat": res["n_high_rhat"],
                         "n_low_ess": res["n_low_ess"], "n_constant": res["n_constant"]}
        del stats
        # the route before it: every draw's predictions to the host, NumPy on top
        rows = min(n, args.host_rows)
        keep = {}

        def leg_to_host():
            keep["pred"] = np.asarray(sampler.sample_posterior(X, list(range(sampler.n_draws)), None))  # (D, K, n)

        def leg_numpy():
            pred = keep["pred"]
            keep["host"] = restatement.columns(np.ascontiguousarray(pred.reshape(pred.shape[0], -1)[:, :rows]), nc)

        t_host = one(leg_to_host, args.host_reps, warm=False)
        t_np = one(leg_numpy, args.host_reps, warm=False)
        scale = n * sampler.n_outputs / rows
        host_ms = t_host["median_ms"] + t_np["median_ms"] * scale
        row["host_route"] = {"sample_posterior_to_host": t_host, "numpy_diagnostics": t_np, "numpy_rows_timed": rows,
                             "numpy_scaled_by": round(scale, 3),
                             "numpy_part": "timed on all rows" if rows == n else f"timed on {rows} rows and scaled to {n}",
                             "total_ms": round(host_ms, 1)}
        row["host_route_over_convergence"] = round(host_ms / row["convergence"]["median_ms"], 1)
        got = res["ess_bulk"][:rows, 0]
        row["ess_bulk_max_rel_diff_to_the_restatement"] = float(np.max(np.abs(got / keep["host"][2][:rows] - 1.0)))
        keep.clear()
        # r_eff against the matrix it would otherwise be computed from
        row["relative_efficiency"] = one(leg_reff, args.reps)

        def leg_matrix():
            keep["ll"] = pointwise_log_likelihood(sampler, X, y, lik, points=pts)

        row["pointwise_log_likelihood_to_host"] = one(leg_matrix, args.host_reps, warm=False)
        keep.clear()
        reff = last["reff"]
        row["reff"] = {"reff": reff["reff"], "reff_min": reff["reff_min"], "n_clamped": reff["n_clamped"]}
        line["shapes"][name] = row
        print(f"[diag_timing] {name}: {json.dumps(row)}", file=sys.stderr, flush=True)
        _timing.write(args.out, line, echo=False)   # (after every shape: a visit that ends early keeps what it has)
        del X, y, sampler, last, f
    line["kernels"] = _timing.kernel_rows(lambda k: k == "k_chain_diag")
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
