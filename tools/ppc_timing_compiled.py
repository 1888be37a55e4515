#!/usr/bin/env python3
"""ms per call of ``pgb_ppc_draw_compiled`` against ``pgb_ppc_draw`` on the same device matrix, on one GPU.

At a cfg2-shaped matrix of predictors (1000 draws x 100 k rows, K = 1; values N(1, 1.5) made on the device, so that the
rates of the count family reach both Poisson samplers), out of place into one result matrix, between two events of the
stream, the median of ``--reps`` calls after one warm-up call, the two calls of a pair alternating:

* ``normal``   the sampler body ``return mu + s * normal();``        against family ``normal``;
* ``negbin``   ``return poisson((exp(mu) * gamma(a)) / a);``        against family ``negbin_log``.

The built-in kernel ``k_ppc`` is the yardstick; there is no threshold -- the kernel is elementwise and should sit near
it.  Each pair is also timed on the first 32 draws x 1024 rows of the matrix (``tiny``): next to no kernel time, so the
difference there is what a call costs around its kernel -- ``pgb_ppc_draw_compiled`` loads and checks its code object
per call.  Writes ``profiles/ppc_compiled_timing.json`` (``--out``) with each pair's times and ratio and with the VGPR /
scratch figures of both bodies' ``k_ppc_compiled`` next to ``k_ppc``'s, and prints it as one JSON line.

  python tools/ppc_timing_compiled.py [--reps 5] [--draws 1000] [--rows 100000] [--out FILE]
"""

from __future__ import annotations

import ctypes as C
import sys

import _timing
from _timing import HERE

TINY = (32, 1024)  # draws x rows of the call that measures the cost around the kernel
PAIRS = {
    "normal": ("return mu + s * normal();", ("s",), "normal", 0.5),
    "negbin": ("return poisson((exp(mu) * gamma(a)) / a);", ("a",), "negbin_log", 2.0),
}


def main(argv=None) -> int:
    ap = _timing.base_parser("ppc_compiled_timing.json")
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--rows", type=int, default=100_000)
    args = ap.parse_args(argv)
    sys.path.insert(0, HERE)
    import numpy as np
    import torch

    from pymc_bart_amd import _abi
    from pymc_bart_amd.compiled import compile_sampler
    from pymc_bart_amd.sampler import default_backend

    be = default_backend()
    lib, mem = be.lib, be.mem
    D, n = args.draws, args.rows
    mu = mem.empty((D * n,), np.float64).normal_(1.0, 1.5)
    out = mem.empty((D * n,), np.float64)
    flags = (C.c_int64 * 2)()
    line = {"metric": "ms_per_call", "reps": args.reps, "shape": {"draws": D, "rows": n, "K": 1}, "pairs": {}}
    for name, (body, names, family, value) in PAIRS.items():
        build = compile_sampler(body, names)
        params = np.full((D, 1), value)
        code = _abi.PpcCode()
        blob = C.create_string_buffer(build.code, len(build.code))
        code.code_object, code.code_bytes = C.cast(blob, C.c_void_p), len(build.code)
        code.n_params, code.params_host = 1, params.ctypes.data
        lik = _abi.PpcLik()
        lik.family, lik.n_params, lik.params_host = _abi.FAMILIES[family], 1, params.ctypes.data
        compiled, builtin = lib.ppc_compiled_entry_point(), lib.ppc_entry_point()

        def pair(d, rows):
            a = lambda s: (mem.ptr(mu), d, 1, rows, rows, 0, C.byref(s), 0, mem.ptr(out), rows, None, None, flags,  # noqa: E731
                           mem.stream_ptr)
            return _timing.events_ms({"compiled": lambda: lib.check(compiled(*a(code)), "pgb_ppc_draw_compiled"),
                                      "builtin": lambda: lib.check(builtin(*a(lik)), "pgb_ppc_draw")}, args.reps)

        ms = pair(D, n)
        tiny = pair(*TINY)  # (next to no kernel time: what a call costs around its kernel)
        torch.cuda.synchronize()
        line["pairs"][name] = {"body": body, "family": family, "param": value,
                               "compiled_ms": round(ms["compiled"], 4), "builtin_ms": round(ms["builtin"], 4),
                               "ratio": round(ms["compiled"] / ms["builtin"], 4),
                               "difference_ms": round(ms["compiled"] - ms["builtin"], 4),
                               "tiny": {"draws": TINY[0], "rows": TINY[1], "compiled_ms": round(tiny["compiled"], 4),
                                        "builtin_ms": round(tiny["builtin"], 4),
                                        "difference_ms": round(tiny["compiled"] - tiny["builtin"], 4)},
                               "k_ppc_compiled": {k: build.resources[k] for k in ("vgpr", "sgpr", "scratch_bytes", "vgpr_spills",
                                                                                 "sgpr_spills")}}
        print(f"[ppc_timing_compiled] {name}: {line['pairs'][name]}", file=sys.stderr, flush=True)
    line["kernels"] = _timing.kernel_rows("k_ppc")
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
