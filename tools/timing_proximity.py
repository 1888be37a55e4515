#!/usr/bin/env python3
"""What the posterior proximity costs on one GPU: the leaf-code walk next to the prediction walk, the count kernel next
to its VALU-issue bound, and the device route next to the host route.

On a real chain of ``sample_chain`` (data: ``workloads.cfg2``; the default shape is cfg2-shaped: 100 k x 50, m = 200,
64 draws) with 256 query rows against all rows, medians of ``--reps`` after one warm-up:

* (a) ``k_leaf_codes`` against ``k_predict`` on the same rows and draws, each between its own stream events
      (``_timing.walk_timing()``, ``pgb_walk_kernel_ms``).  The walks are the same; the code walk stores one byte per
      (row, tree, draw) where the prediction reads the leaf value and stores 8 bytes per (row, draw).
* (b) ``pgb_prox_count`` between two events of the stream (``k_prox_count`` and the entry point's wait for the stream) as
      byte comparisons per second, next to the VALU-issue bound: ``256 CUs x 4 SIMDs x 2.4 GHz / 2`` cycles per
      32-bit wave-instruction, over the vector instructions per (16 queries, word) counted in the disassembly of the
      built library, times the 64 lanes x 16 queries x 4 bytes one pass of the loop compares.
* (c) ``nearest_rows`` (k = 10) from host arrays to host results, and THE HOST ROUTE: ``leaf_ids`` to the host plus the
      NumPy comparison ``(codes_r != codes_q).sum(0)`` per query.  The host route is timed on a corner (``--corner-rows``
      reference rows x ``--corner-queries`` queries, all draws) and SCALED by the number of pairs to the full call: it is
      labelled as scaled, not measured, at the full size.

Writes ``profiles/proximity_timing.json`` (``--out``) and prints it as one JSON line.  Nothing is required of the
figures.
(The file is not named ``*_timing.py``: ``tests/test_timing_tools.py`` holds the list of those; this tool's own ``--help``
and instruction count are checked in ``tests/test_proximity.py``.)

  python tools/timing_proximity.py [--reps 5] [--shapes cfg2] [--out FILE]
"""

from __future__ import annotations

import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import _timing
from _timing import HERE

SHAPES = {
    "plot": dict(n=2000, p=10, m=50, draws=32),
    "cfg2": dict(n=100_000, p=50, m=200, draws=64),
}
QUERIES = 256
# 32-bit VALU issue: 256 CUs x 4 SIMDs x 2.4 GHz, a wave64 32-bit instruction occupies its SIMD-32 for 2 cycles
VALU_B32_PEAK_GINST = 256 * 4 * 2.4 / 2.0  # G wave-instructions / s
QUERY_TILE = 16                            # PROX_QT


def valu_per_word() -> int | None:
    """The vector instructions of one pass of ``k_prox_count``'s loop over the words (16 queries x 1 reference word per
    lane), counted in the disassembly of the built library: from the scalar load of the tile's 16 query words to the
    loop's branch.  ``None`` when the loop is not found in that form."""
    import occupancy_guard

    tmp = tempfile.mkdtemp(prefix="pgb_prox_")
    try:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(occupancy_guard.SO, local)
        llvm = occupancy_guard.LLVM
        subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", local], stdout=subprocess.DEVNULL, cwd=tmp)
        co = [f for f in os.listdir(tmp) if "gfx950" in f]
        if len(co) != 1:
            return None
        asm = subprocess.check_output([os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", os.path.join(tmp, co[0])],
                                      text=True).splitlines()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    heads = [i for i, ln in enumerate(asm) if ln.endswith(">:")]                # one label per function
    mine = [i for i in heads if "k_prox_count" in asm[i]]
    if len(mine) != 1:
        return None
    end = min([i for i in heads if i > mine[0]], default=len(asm))
    ops = [ln.split()[0] for ln in asm[mine[0] + 1:end] if ln.startswith("\t") and ln.split()]
    starts = [i for i, op in enumerate(ops) if op == "s_load_dwordx16"]
    if len(starts) != 1:
        return None
    count = 0
    for op in ops[starts[0]:]:
        if op.startswith("s_cbranch"):
            return count
        count += op.startswith("v_")
    return None


def main(argv=None) -> int:
    ap = _timing.base_parser("proximity_timing.json", "cfg2")
    ap.add_argument("--corner-rows", type=int, default=2000)
    ap.add_argument("--corner-queries", type=int, default=32)
    args = ap.parse_args(argv)
    names = [s for s in args.shapes.split(",") if s]
    sys.path.insert(0, HERE)
    import numpy as np
    import torch  # noqa: F401

    from pymc_bart_amd import leaf_ids, nearest_rows
    from pymc_bart_amd.proximity import ProximityJob, words
    from pymc_bart_amd.utils import _get_posterior_sampler

    per_word = valu_per_word()
    line = {"metric": "ms_per_call", "reps": args.reps, "queries": QUERIES, "shapes": _timing.kept_shapes(args.out, names),
            "valu_b32_peak_G_wave_instructions_per_s": VALU_B32_PEAK_GINST,
            "k_prox_count_valu_per_16_queries_and_word": per_word}
    for name in names:
        shape = SHAPES[name]
        f = _timing.fit(shape)
        X, sampler = f.X, _get_posterior_sampler(f.op)
        n = X.shape[0]
        rng = np.random.default_rng(3)
        Xq = X[rng.choice(n, QUERIES, replace=False)] + rng.normal(0, 0.01, (QUERIES, X.shape[1]))
        job = ProximityJob(sampler, Xq, X)
        D, m, T = job.D, job.m, job.T
        res = _timing.resident_predictions(job)
        be = res.backend
        lib, mem = be.lib, be.mem
        codes_, count, _, _ = lib.proximity_entry_points()
        ms_of = lib.lib.pgb_walk_kernel_ms
        ms_of.argtypes = [C.POINTER(C.c_double)]

        # (a) the two walks, each between its own events
        walk = {"k_predict": [], "k_leaf_codes": []}
        cr = None
        with _timing.walk_timing():
            for _ in range(args.reps + 1):
                v = C.c_double()
                res.fill()
                ms_of(C.byref(v))
                walk["k_predict"].append(v.value)
                cr = None
                cr = job.codes(be, codes_, res.x, n, 0, D)
                ms_of(C.byref(v))
                walk["k_leaf_codes"].append(v.value)
        walk = {k: float(np.median(v[1:])) for k, v in walk.items()}

        # (b) the count alone on the resident codes
        cq = job.codes(be, codes_, mem.from_host(job.Q), QUERIES, 0, D)
        dist = mem.empty((QUERIES * n,), np.int32)
        W = words(T)
        count_ms = _timing.events_ms(lambda: lib.check(count(mem.ptr(cq), QUERIES, QUERIES, mem.ptr(cr), n, n, W, mem.ptr(dist), n, 1,
                                                             mem.stream_ptr), "pgb_prox_count"), args.reps)
        compared = float(QUERIES) * n * T
        rate = compared / (count_ms * 1e-3)
        bound = None if not per_word else VALU_B32_PEAK_GINST * 1e9 / per_word * 64 * QUERY_TILE * 4
        del cq, cr, dist, res

        # (c) the device route end to end, and the host route on a corner
        got = {}
        t_dev = _timing.time_legs({"nearest_rows": lambda: got.__setitem__("dev", nearest_rows(sampler, Xq, X, k=10))}, args.reps)
        cn, cq_n = min(args.corner_rows, n), min(args.corner_queries, QUERIES)

        def host_route():
            ids_r = leaf_ids(sampler, X[:cn]).reshape(T, cn)
            ids_q = leaf_ids(sampler, Xq[:cq_n]).reshape(T, cq_n)
            got["host"] = np.stack([(ids_r != ids_q[:, i:i + 1]).sum(0) for i in range(cq_n)])

        t0 = time.perf_counter()
        host_route()
        corner_ms = (time.perf_counter() - t0) * 1e3
        want = np.sort(got["host"], axis=1)[:, :10]
        check = nearest_rows(sampler, Xq[:cq_n], X[:cn], k=10)
        same = bool(np.array_equal(T - check["matches"].astype(np.int64), want))
        scale = (float(QUERIES) * n) / (float(cq_n) * cn)
        row = {"shape": dict(shape, chain_seconds=round(f.seconds, 1), slots=T),
               "walks_ms": {k: round(v, 4) for k, v in walk.items()},
               "k_leaf_codes_over_k_predict": round(walk["k_leaf_codes"] / walk["k_predict"], 3),
               "pgb_prox_count_ms": round(count_ms, 4), "byte_comparisons": compared,
               "byte_comparisons_per_s": rate, "valu_issue_bound_byte_comparisons_per_s": bound,
               "share_of_valu_issue_bound": None if not bound else round(rate / bound, 4),
               "nearest_rows_k10": t_dev["nearest_rows"],
               "host_route": {"corner": {"rows": cn, "queries": cq_n, "ms": round(corner_ms, 1)},
                              "scaled_to_full_ms": round(corner_ms * scale, 1), "scaled": True,
                              "corner_equals_device": same}}
        print(f"[timing_proximity] {name}: {json.dumps(row)}", file=sys.stderr, flush=True)
        line["shapes"][name] = row
        del X, sampler, f, job, got
    line["kernels"] = _timing.kernel_rows(("k_leaf_codes", "k_prox_"))
    _timing.write(args.out, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
