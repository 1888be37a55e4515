"""Test helpers of the partial dependence tests (``test_pdp.py``, ``test_pdp_gpu.py``).

* :func:`yardstick` -- ``pdp_sweep`` restated: per column one ``sampler.sample_posterior`` call with every other
  column excluded.
* :func:`breakpoints`, :func:`representatives`, :func:`lookup`, :func:`profile_sweep` -- the profile route of
  ``include/pgbart_pdp.h`` restated in NumPy: a forest's split values on a column, the value each slot is evaluated
  at, the slot of a value, and the sweep put together from per-slot predictions.
* :func:`hand_pool` -- a small dyadic pool whose split values on column 0 are the edge cases.
* :func:`probes` -- values of ``x`` that must fall into each slot: its ends, the doubles next to them, its middle.
"""

from __future__ import annotations

import numpy as np

import math

import _predict_exact as ex
from _predict_exact import Leaf, Split
from pymc_bart_amd import _abi


def yardstick(sampler, X, cols, picks) -> np.ndarray:
    """``(n_cols, n_picks, K, n_rows)`` through ``sampler.sample_posterior`` with exclusions."""
    X = np.ascontiguousarray(X, np.float64)
    p = X.shape[1]
    picks = np.asarray(picks)
    return np.stack([np.asarray(sampler.sample_posterior(X, [int(v) for v in picks[c]], [v for v in range(p) if v != j]))
                     for c, j in enumerate(cols)])


def breakpoints(pool, forest, j: int):
    """``(eligible, b)``: the split values the trees ``forest`` (indices into ``pool``) hold on column ``j``, sorted
    and de-duplicated by ``==`` (NaN split values left out); not eligible when a split on ``j`` follows another rule
    than the continuous one or a leaf regresses on ``j``."""
    vals = []
    for t in np.asarray(forest).tolist():
        for g in range(int(pool.node_off[t]), int(pool.node_off[t + 1])):
            if pool.var[g] < 0:
                if pool.svar[g] == j:
                    return False, None
            elif pool.var[g] == j:
                if pool.rule[g] != _abi.RULE_CONTINUOUS:
                    return False, None
                if pool.split[g] == pool.split[g]:
                    vals.append(float(pool.split[g]))
    b = []
    for v in sorted(vals):
        if not b or v != b[-1]:
            b.append(v)
    return True, np.asarray(b, np.float64)


def representatives(b: np.ndarray) -> np.ndarray:
    """The value each of the ``B + 2`` slots is evaluated at: the breakpoints, ``+inf`` ("above all"), NaN."""
    return np.concatenate([b, [np.inf, np.nan]])


def lookup(b: np.ndarray, x: np.ndarray) -> np.ndarray:
    """The slot of every ``x``: the first breakpoint ``>= x``; none: ``B``; NaN: ``B + 1``."""
    x = np.asarray(x, np.float64)
    slot = np.array([next((k for k, v in enumerate(b.tolist()) if v >= xi), b.size) for xi in x.tolist()], np.int64)
    slot[np.isnan(x)] = b.size + 1
    return slot


def probes(b: np.ndarray) -> list:
    """Per slot the values of ``x`` that belong to it (the NaN slot: NaN alone)."""
    out = []
    for k in range(b.size):
        lo = -np.inf if k == 0 else b[k - 1]
        xs = [float(b[k])]
        if np.nextafter(b[k], -np.inf) > lo:
            xs.append(float(np.nextafter(b[k], -np.inf)))
        if np.nextafter(lo, np.inf) < b[k]:
            xs.append(float(np.nextafter(lo, np.inf)))
        if np.isfinite(lo) and np.isfinite(b[k]) and lo < lo / 2 + b[k] / 2 <= b[k]:
            xs.append(float(lo / 2 + b[k] / 2))
        if k == 0:
            xs.append(-np.inf)
            if np.isfinite(b[0]):
                xs.append(float(b[0] - 1.0))
        if b[k] == 0.0:
            xs += [0.0, -0.0]
        out.append(xs)
    if b.size == 0:
        out.append([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf])
    elif np.isfinite(b[-1]):
        out.append([float(np.nextafter(b[-1], np.inf)), float(b[-1] + 1.0), np.inf])
    else:
        out.append([])  # a breakpoint +inf: nothing lies above it
    out.append([np.nan])
    return out


def profile_sweep(sampler, X, cols, picks) -> np.ndarray:
    """``pdp_sweep`` by the profile route, restated: per (column, pick) the forest is predicted at the slots'
    representatives only (``sample_posterior`` with exclusions) and every row takes its slot's prediction.  Every
    column must be eligible."""
    X = np.asarray(X, np.float64)
    n, p = X.shape
    picks = np.asarray(picks)
    K = sampler.n_outputs
    out = np.empty((len(cols), picks.shape[1], K, n))
    for c, j in enumerate(cols):
        others = [v for v in range(p) if v != j]
        for s, d in enumerate(picks[c].tolist()):
            ok, b = breakpoints(sampler.pool, sampler.forest_idx[d], j)
            assert ok, (j, d)
            rep = np.full((b.size + 2, p), 12345.0)   # (the other columns are excluded: never read)
            rep[:, j] = representatives(b)
            table = np.asarray(sampler.sample_posterior(rep, [int(d)], others))[0]   # (K, slots)
            out[c, s] = table[:, lookup(b, X[:, j])]
    return out


def hand_pool():
    """Seven dyadic trees over three columns: column 0 carries the split values 0.0 (twice), -0.0, 0.5 (in three
    trees), -1.25 and +inf; column 1 a single split; column 2 none.  Leaves regress on column 1 or 2, never on 0."""
    rng = np.random.default_rng(19)

    def leaf(svar=-1):
        lf = Leaf(ex.dyadic(rng, 10, 8.0, 2))
        if svar >= 0:
            lf.svar, lf.slope, lf.xbar = svar, ex.dyadic(rng, 4, 2.0, 2), float(ex.dyadic(rng, 4, 2.0))
        return lf

    def split(var, v, left, right):
        nd = Split(var, v, left, right)
        nd.left.count, nd.right.count = ex.pair_counts(rng)
        return nd

    roots = [
        split(0, 0.5, leaf(), split(0, math.inf, leaf(1), leaf())),
        split(0, 0.0, split(0, -1.25, leaf(), leaf(2)), split(0, 0.5, leaf(), leaf())),
        split(1, 0.25, split(0, -0.0, leaf(), leaf()), split(0, 0.5, leaf(1), leaf())),
        split(0, 0.0, leaf(), leaf()),
        leaf(2),
        split(1, 0.25, leaf(), leaf(1)),
        ex.chain_tree(rng, 2, 5, [0], lambda r, j: float(ex.dyadic(r, 3, 2.0)), "left"),
    ]
    return ex.build_pool(roots, 2)
