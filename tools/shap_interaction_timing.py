#!/usr/bin/env python3
"""ms of ``k_shap_interaction`` between stream events, next to ``k_shap`` on the same rows and draws, and ms per call of
``shap_interaction_values`` / ``shap_interaction_summary`` on one GPU, at the two shapes of ``tools/shap_timing.py``:

* ``plot``  plot-sized: n = 1000, p = 10, m = 50, 100 stored draws, 20 of them attributed;
* ``cfg2``  cfg2-shaped: 100 k x 50, m = 200, 50 stored draws, 8 of them attributed.

Kernels alone (``_timing.walk_timing()``; ``pgb_shap_interactions_kernel_ms``, ``pgb_shap_kernel_ms``): the device buffers of
``device_blocks`` are timed block by block and never copied to the host, the kernel times of the blocks added up; at
most ``--kernel-rows`` rows (default 16384), with every column and with the first 8.  The public calls run from host
arrays to host results, after warming, median of ``--reps``: with every column at ``plot``; at ``cfg2`` with the first 8
columns only -- all 50 make 8 x 2500 x 100 k doubles, 16 GB on the host.  There is no earlier implementation and no
target ratio: the numbers say what the pairwise split costs next to the attributions it refines.

Writes ``profiles/shap_interaction_timing.json`` (``--out``) and prints it as one JSON line.

  python tools/shap_interaction_timing.py [--reps 5] [--shapes plot,cfg2] [--kernel-rows N] [--out FILE]
"""

from __future__ import annotations

import ctypes as C
import json
import sys

import _timing
from _timing import HERE
from shap_timing import SHAPES


def _kernels_alone(s, X, picks, cols, reps):
    """``k_shap_interaction`` over ``cols`` and ``k_shap`` on the rows ``X`` and the draws ``picks``: medians of the
    kernel ms added over the row blocks."""
    import numpy as np

    from pymc_bart_amd import shap, shap_interaction

    part = s._chain_samplers[0]
    be = part._get_backend()
    pool, table = s.pooled_history()
    K, m = int(part.n_outputs), int(part.m)
    Xc, pk = shap.checked(X, False, picks, int(np.asarray(table).shape[0]))
    cc = shap_interaction._checked_cols(cols, Xc.shape[1])
    x_ms, s_ms = be.lib.lib.pgb_shap_interactions_kernel_ms, be.lib.lib.pgb_shap_kernel_ms
    x_ms.argtypes = s_ms.argtypes = [C.POINTER(C.c_double)]

    def total(blocks, read):
        acc = 0.0
        for _ in blocks:
            v = C.c_double(-1.0)
            read(C.byref(v))
            acc += v.value
        return acc

    a, b = [], []
    with _timing.walk_timing():
        for _ in range(reps + 1):
            a.append(total(shap_interaction.device_blocks(be, pool, table, m, K, Xc, cc, pk), x_ms))
            b.append(total(shap.device_blocks(be, pool, table, m, K, Xc, pk), s_ms))
    kx, ks = float(np.median(a[1:])), float(np.median(b[1:]))
    return {"rows": int(Xc.shape[0]), "cols": int(cc.size), "k_shap_interaction_ms": round(kx, 4), "k_shap_ms": round(ks, 4),
            "k_shap_interaction_over_k_shap": round(kx / ks, 1)}


def main(argv=None) -> int:
    ap = _timing.base_parser("shap_interaction_timing.json", "plot,cfg2")
    ap.add_argument("--kernel-rows", type=int, default=16384)
    args = ap.parse_args(argv)
    sys.path.insert(0, HERE)
    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import shap_interaction_summary, shap_interaction_values, shap_values
    from pymc_bart_amd.utils import _get_posterior_sampler

    line = {"metric": "ms_per_call", "reps": args.reps, "shapes": {}}
    for name in [s for s in args.shapes.split(",") if s]:
        shape = SHAPES[name]
        f = _timing.fit(shape)
        X, s, secs = f.X, _get_posterior_sampler(f.op), f.seconds
        picks = np.random.default_rng(3).integers(0, s.n_draws, size=shape["picks"]).tolist()
        cols = None if name == "plot" else list(range(8))
        t = _timing.time_legs({"shap_interaction_values": lambda: shap_interaction_values(s, X, cols=cols, draws=picks),
                   "shap_interaction_summary": lambda: shap_interaction_summary(s, X, cols=cols, draws=picks),
                   "shap_values": lambda: shap_values(s, X, draws=picks)}, args.reps)
        Xk = X[:args.kernel_rows]
        row = {"shape": dict(shape, chain_seconds=round(secs, 1)), "public_cols": shape["p"] if cols is None else len(cols), **t,
               "kernels_alone": [_kernels_alone(s, Xk, picks, None, args.reps), _kernels_alone(s, Xk, picks, list(range(8)), args.reps)]}
        vals = shap_interaction_values(s, X[:256], draws=picks)
        ref = shap_values(s, X[:256], draws=picks)
        row["row_sum_max_abs_gap"] = float(np.max(np.abs(vals["values"].sum(-1) - ref["values"])))
        line["shapes"][name] = row
        print(f"[shap_interaction_timing] {name}: {json.dumps(row)}", file=sys.stderr, flush=True)
        del X, f, s
    line["kernels"] = _timing.kernel_rows("k_shap_interaction<")
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
