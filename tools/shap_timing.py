#!/usr/bin/env python3
"""ms per call of ``shap_values`` -- ``pgb_predict_shap``, one call per block of rows -- on one GPU, with ``pgb_predict``
on the same rows and draws in the same process as the yardstick.

The public call is timed from host arrays to host results, after warming, median of ``--reps``, at two shapes:

* ``plot``  plot-sized: n = 1000, p = 10, m = 50, 100 stored draws, 20 of them attributed;
* ``cfg2``  cfg2-shaped: 100 k x 50, m = 200, 50 stored draws, 8 of them attributed.

Also recorded, per shape: ``k_shap`` alone between stream events (``_timing.walk_timing()``, ``pgb_shap_kernel_ms``) and
``k_predict`` alone (``pgb_walk_kernel_ms``), their ratio, ``shap_summary`` (the attributions stay on the device), and
the kernels' resource rows.  There is no earlier implementation of the attributions: no speed-up is claimed, the ratio
to ``pgb_predict`` says what an attribution costs next to a prediction.

Writes ``profiles/shap_timing.json`` (``--out``) and prints it as one JSON line.

  python tools/shap_timing.py [--reps 5] [--shapes plot,cfg2] [--out FILE]
"""

from __future__ import annotations

import ctypes as C
import json
import sys

import _timing
from _timing import HERE

SHAPES = {
    "plot": dict(n=1000, p=10, m=50, draws=100, picks=20),
    "cfg2": dict(n=100_000, p=50, m=200, draws=50, picks=8),
}


def _kernels_alone(s, rows, picks, reps):
    """``k_shap`` and ``k_predict`` of the same rows and draws between stream events (medians, ms)."""
    import numpy as np

    lib = s._chain_samplers[0]._get_backend().lib
    shap_ms, walk_ms = lib.lib.pgb_shap_kernel_ms, lib.lib.pgb_walk_kernel_ms
    shap_ms.argtypes = walk_ms.argtypes = [C.POINTER(C.c_double)]
    a, b = [], []
    with _timing.walk_timing():
        for _ in range(reps + 1):
            v = C.c_double(-1.0)
            s.shap(rows, picks)
            shap_ms(C.byref(v))
            a.append(v.value)
            v = C.c_double(-1.0)
            s.sample_posterior(rows, picks, None)
            walk_ms(C.byref(v))
            b.append(v.value)
    ks, kp = float(np.median(a[1:])), float(np.median(b[1:]))
    return {"k_shap_ms": round(ks, 4), "k_predict_ms": round(kp, 4), "k_shap_over_k_predict": round(ks / kp, 1)}


def main(argv=None) -> int:
    args = _timing.base_parser("shap_timing.json", "plot,cfg2").parse_args(argv)
    sys.path.insert(0, HERE)
    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import shap_summary, shap_values
    from pymc_bart_amd.utils import _get_posterior_sampler

    line = {"metric": "ms_per_call", "reps": args.reps, "shapes": {}}
    for name in [s for s in args.shapes.split(",") if s]:
        shape = SHAPES[name]
        f = _timing.fit(shape)
        X, s, secs = f.X, _get_posterior_sampler(f.op), f.seconds
        picks = np.random.default_rng(3).integers(0, s.n_draws, size=shape["picks"]).tolist()
        t = _timing.time_legs({"shap_values": lambda: shap_values(s, X, draws=picks),
                   "shap_summary": lambda: shap_summary(s, X, draws=picks),
                   "sample_posterior": lambda: s.sample_posterior(X, picks, None)}, args.reps)
        row = {"shape": dict(shape, chain_seconds=round(secs, 1)), **t,
               "shap_values_over_sample_posterior": round(t["shap_values"]["median_ms"] / t["sample_posterior"]["median_ms"], 1),
               "kernels_alone": _kernels_alone(s, s._chain_samplers[0].resident_rows(X), picks, args.reps)}
        vals = shap_values(s, X[:256], draws=picks)
        pred = np.asarray(s.sample_posterior(X[:256], picks, None))[:, 0, :]
        row["efficiency_max_abs_gap"] = float(np.max(np.abs(vals["base"][:, None] + vals["values"].sum(-1) - pred)))
        line["shapes"][name] = row
        print(f"[shap_timing] {name}: {json.dumps(row)}", file=sys.stderr, flush=True)
        del X, f, s
    line["kernels"] = _timing.kernel_rows("k_shap<")
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
