"""The measuring protocol of the ``tools/*_timing.py``, stated once: the chain every tool times on, the host-clock
legs, the event-timed entry point, the baseline process and the file a tool writes.  The figures of
``profiles/*_timing.json`` rest on it, so a change here (warm-up, interleaving, what counts as spread) reaches them all.

torch and the package are imported when a function first needs them -- after the tool has put its package on
``sys.path`` (``--root`` in a baseline process) --, so that ``--help`` works without a device.  Nothing here falls back
when there is no GPU: it fails.
"""

from __future__ import annotations

import argparse
import contextlib
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASELINE_SECONDS = 1100


def base_parser(default_out, shapes=None, reps=5, baseline=False) -> argparse.ArgumentParser:
    """``--reps``, ``--shapes`` (the default ``shapes``; none for a tool of one shape) and ``--out`` (``default_out``
    under ``profiles/``); ``baseline``: also the three arguments of the baseline process."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=reps)
    if shapes is not None:
        ap.add_argument("--shapes", default=shapes)
    if baseline:
        ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit: the baseline's package")
        ap.add_argument("--baseline-leg", action="store_true", help=argparse.SUPPRESS)  # (the child process of --baseline-root)
        ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", default_out))
    return ap


def fit(shape, chains=1, tune=10, particles=10):
    """The chain(s) a tool times on: a ``BARTOp`` on ``workloads.cfg2`` data of the shape's ``n`` / ``p`` / ``m`` (those
    it names), ``shape["draws"]`` draws after ``tune`` tuning steps, seed 7, the draws not kept.  ``chains > 1``: one
    after the other, their histories attached to the op.  A shape may name another ``workload`` of
    ``pymc_bart_amd.workloads`` and a ``likelihood`` for ``sample_chain``.  -> ``X``, ``Y``, ``op``, ``results`` (one
    per chain), ``seconds`` (of the chains)."""
    from pymc_bart_amd import BARTOp, workloads
    from pymc_bart_amd.chains import attach_history, sample_chain

    w = getattr(workloads, shape.get("workload", "cfg2"))(**{k: shape[k] for k in ("n", "p", "m") if k in shape})
    op = BARTOp(w["X"], w["Y"], m=w["m"])
    t0 = time.perf_counter()
    results = [sample_chain(op, tune, shape["draws"], num_particles=particles, random_seed=7, chain=c, keep_draws=False,
                            likelihood=shape.get("likelihood")) for c in range(chains)]
    seconds = time.perf_counter() - t0
    if chains > 1:
        attach_history(op, results)
    return SimpleNamespace(X=w["X"], Y=w["Y"], op=op, results=results, seconds=seconds)


def time_legs(legs: dict, reps: int, warm: bool = True) -> dict:
    """``{leg: {"median_ms", "min_ms", "max_ms"}}`` of ``reps`` rounds over the legs, interleaved, every call between
    two device synchronises on the host clock; ``warm``: every leg once before."""
    import numpy as np
    import torch

    if warm:
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
    return {k: {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
            for k, v in ms.items()}


def by_statistic(timed: dict, legs=None) -> dict:
    """``time_legs``' result the other way round, ``{"median_ms": {leg: ...}, "min_ms": ..., "max_ms": ...}`` (of
    ``legs``): the layout of a baseline record and of some files."""
    legs = list(timed) if legs is None else legs
    return {stat: {k: timed[k][stat] for k in legs} for stat in ("median_ms", "min_ms", "max_ms")}


def events_ms(call, reps: int, before=None):
    """ms of ``call()`` between two events of the current stream: ``reps + 1`` pairs, the first dropped, the median.
    A dict of calls alternates them and gives a dict of medians; ``before()`` runs ahead of every pair, untimed."""
    import numpy as np
    import torch

    calls = call if isinstance(call, dict) else {None: call}
    ev = {k: [] for k in calls}
    for _ in range(reps + 1):
        for k, f in calls.items():
            if before is not None:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ev[k].append(a.elapsed_time(b))
    med = {k: float(np.median(v[1:])) for k, v in ev.items()}
    return med if isinstance(call, dict) else med[None]


def resident_predictions(job):
    """``pgb_predict`` of every draw of the stored-draw ``job`` at every row of it into device scratch -> ``backend``,
    ``x`` (the rows), ``pred`` (``[D][K][n]`` doubles) and ``fill()``, which runs the prediction into ``pred`` again."""
    import ctypes as C

    import numpy as np

    be = job.hip_backend("a timing tool runs")
    lib, mem = be.lib, be.mem
    n, D, K, p = job.n, job.D, job.K, job.p
    xd = mem.from_host(job.X)
    md = mem.empty((D * K * n,), np.float64)
    carr = job.pool.as_c()

    def fill():
        lib.check(lib.lib.pgb_predict(C.byref(carr), job.fidx.ctypes.data, D, job.m, mem.ptr(xd), n, p, p, None, 0,
                                      mem.ptr(md), mem.stream_ptr), "pgb_predict")

    fill()
    return SimpleNamespace(backend=be, x=xd, pred=md, fill=fill)


@contextlib.contextmanager
def walk_timing():
    """``PGB_WALK_TIMING=1`` inside (the walk kernels then record their own stream events), the variable as it was
    afterwards, also after an exception."""
    before = os.environ.get("PGB_WALK_TIMING")
    os.environ["PGB_WALK_TIMING"] = "1"
    try:
        yield
    finally:
        if before is None:
            del os.environ["PGB_WALK_TIMING"]
        else:
            os.environ["PGB_WALK_TIMING"] = before


def print_baseline(obj) -> None:
    """What a baseline process (``--baseline-leg``) ends with."""
    print("BASELINE " + json.dumps(obj), flush=True)


def run_baseline(script, root, argv):
    """The baseline: ``script --baseline-leg --root ROOT *argv`` in a process of its own, on the package found in
    ``root``; its stderr passes through.  -> what it handed to ``print_baseline`` (its last ``BASELINE`` line)."""
    cmd = [sys.executable, os.path.abspath(script), "--baseline-leg", "--root", os.path.abspath(root), *argv]
    txt = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=BASELINE_SECONDS).stdout
    return json.loads([ln for ln in txt.splitlines() if ln.startswith("BASELINE ")][-1][9:])


def spread(b: dict, legs) -> float:
    """The run-to-run spread of a baseline record ``b`` (``by_statistic``'s layout) timed as two legs of the same call:
    the larger of the difference of their medians and of either leg's max - min."""
    first, again = legs
    return max(abs(b["median_ms"][first] - b["median_ms"][again]), max(b["max_ms"][k] - b["min_ms"][k] for k in legs))


def kept_shapes(out, names) -> dict:
    """The shapes already in the file ``out`` that are not timed now (``names``)."""
    if not os.path.exists(out):
        return {}
    with open(out) as fh:
        return {k: v for k, v in json.load(fh).get("shapes", {}).items() if k not in names}


def kernel_rows(which) -> list:
    """The resource rows of ``occupancy_guard.table()`` whose kernel name starts with ``which`` (a string or a tuple
    of them) or satisfies it (a predicate)."""
    import occupancy_guard

    keep = which if callable(which) else (lambda name: name.startswith(which))
    return [k for k in occupancy_guard.table() if keep(k["kernel"])]


def write(out, line, echo: bool = True) -> None:
    """``line`` into the file ``out`` and (``echo``), as one JSON line, to stdout."""
    with open(out, "w") as fh:
        json.dump(line, fh, indent=1)
        fh.write("\n")
    if echo:
        print(json.dumps(line))
