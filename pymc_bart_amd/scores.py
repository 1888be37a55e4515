"""Reading a fit: scoring rules of the posterior predictive on the device (``pgb_row_score``,
``include/pgbart_score.h``).

``log_predictive_density`` and ``loo`` score a fit by its log density, ``bayes_r2`` by the squared error of the mean
function; how good the predictive DISTRIBUTION is at held-out rows, in the units of the response, is what the proper
scoring rules say: the continuous ranked probability score (for counts: the ranked probability score), the quantile
(pinball) loss, the interval score with the coverage of central intervals, and the Dawid-Sebastiani score.  All are
functions of one row's ``D`` replicated observations and its observed ``y``: per block of rows one ``pgb_predict`` call
writes the predictors of all draws into device scratch, one ``pgb_ppc_draw`` (``pgb_ppc_draw_compiled``) call turns them
into ``y_rep`` in place and one ``pgb_row_score`` call sorts every column over its draws and reads the pieces of the
scores out of it -- ``(6 + 2 L) x rows`` doubles reach the host, ``L`` the levels of the call, and nothing of size
``draws x rows``.

* :func:`predictive_scores` scores a fit at the rows of ``X`` against ``y``.
* :func:`score_matrix` takes a ``(D, n)`` matrix ``y_rep`` the caller already has on the host.

HIP backend only.  Between 2 and :data:`MAX_DRAWS` draws, at most :data:`MAX_LEVELS` levels per call (the quantiles and
the ends of the intervals that are not among them).
"""

from __future__ import annotations

import math

import numpy as np

from ._stored import check_y, hip_only, matrix_blocks
from .predictive import Replicator, _Job

MAX_DRAWS = 16384    # PGB_ROWSUM_MAX_DRAWS (include/pgbart_rowsummary.h)
MAX_LEVELS = 16      # PGB_ROWSUM_MAX_Q
N_FIXED = 6          # PGB_SCORE_NFIXED: mean, var, abs_err, pair_sum, n_below, n_equal
DEFAULT_QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)
DEFAULT_INTERVALS = (0.5, 0.9)


class Levels:
    """The levels of one call: the user's quantiles ``q`` followed by the ends ``(1 - c) / 2`` and ``(1 + c) / 2`` of
    every central interval of mass ``c`` (``masses``) that are not in the list already (by their bits: 0.25 is in
    ``(0.05, 0.25, ...)``, ``(1 - 0.9) / 2`` is not 0.05).  ``all``: the list the kernel takes; ``ends`` ``(I, 2)``: where
    in it the two ends of every interval are."""

    def __init__(self, quantiles, intervals):
        q = np.asarray([] if quantiles is None else quantiles, dtype=np.float64)
        if q.ndim != 1:
            raise ValueError(f"quantiles must be a vector of levels, got shape {q.shape}")
        if q.size and not np.all((q >= 0.0) & (q <= 1.0)):  # (a NaN fails both comparisons)
            raise ValueError("quantiles must be in [0, 1]")
        c = np.asarray([] if intervals is None else intervals, dtype=np.float64)
        if c.ndim != 1:
            raise ValueError(f"intervals must be a vector of masses, got shape {c.shape}")
        if c.size and not np.all((c > 0.0) & (c < 1.0)):
            raise ValueError("the mass of a central interval must be in (0, 1)")
        levels = [float(v) for v in q]
        ends = np.empty((c.size, 2), np.int64)
        for i, mass in enumerate(c):
            for side, level in enumerate(((1.0 - float(mass)) / 2.0, (1.0 + float(mass)) / 2.0)):
                if level not in levels:
                    levels.append(level)
                ends[i, side] = levels.index(level)
        if len(levels) > MAX_LEVELS:
            raise ValueError(f"at most {MAX_LEVELS} levels per call (the quantiles and the interval ends that are not among "
                             f"them), got {len(levels)}")
        self.q, self.masses, self.ends = np.ascontiguousarray(q), np.ascontiguousarray(c), ends
        self.all = np.ascontiguousarray(levels, dtype=np.float64)

    @property
    def n_out(self) -> int:
        return N_FIXED + 2 * int(self.all.size)


def check_n_draws(D: int) -> int:
    D = int(D)
    if D < 2:
        raise ValueError(f"a score over the draws needs at least 2 draws, got {D}")
    if D > MAX_DRAWS:
        raise ValueError(f"a score on the device takes at most {MAX_DRAWS} draws, got {D} (thin them: draws=)")
    return D


def score_backend(be):
    """``be`` (``None``: the default backend) if its library has ``pgb_row_score`` -- ``NotImplementedError`` naming it
    otherwise (the CPU oracle) -- and is the HIP one."""
    if be is None:
        from .sampler import default_backend

        be = default_backend()
    be.lib.score_entry_point()
    return hip_only(be, "predictive scores run")


def score_block(lib, mem, md, D: int, n_cols: int, ld: int, yd, levels: np.ndarray) -> np.ndarray:
    """``(6 + 2 L, n_cols)`` of the device matrix ``md`` ``[D][ld]`` against the device vector ``yd`` ``[n_cols]``."""
    rows = N_FIXED + 2 * int(levels.size)
    sd = mem.empty((rows * n_cols,), np.float64)
    rc = lib.score_entry_point()(mem.ptr(md), D, n_cols, ld, mem.ptr(yd), levels.ctypes.data if levels.size else None,
                                 int(levels.size), mem.ptr(sd), mem.stream_ptr)
    lib.check(rc, "pgb_row_score")
    return mem.to_host(sd).reshape(rows, n_cols)


def interval_scores(lo, hi, y, mass: float):
    """``(hi - lo) + (2 / alpha) (lo - y)+ + (2 / alpha) (y - hi)+`` with ``alpha = 1 - mass``, and ``lo <= y <= hi``."""
    alpha = 1.0 - float(mass)
    score = (hi - lo) + (2.0 / alpha) * np.maximum(lo - y, 0.0) + (2.0 / alpha) * np.maximum(y - hi, 0.0)
    return score, (lo <= y) & (y <= hi)


def result(stats: np.ndarray, y: np.ndarray, D: int, lev: Levels) -> dict:
    """``stats`` ``(6 + 2 L, n)`` (``pgb_row_score``'s rows) and ``y`` ``(n,)`` -> the public dict."""
    n, L, Q = int(y.size), int(lev.all.size), int(lev.q.size)
    mean, var, abs_err, pair_sum = (stats[r].copy() for r in range(4))
    below, equal = stats[4].astype(np.int64), stats[5].astype(np.int64)
    quant, pinball = stats[N_FIXED:N_FIXED + L], stats[N_FIXED + L:N_FIXED + 2 * L]
    crps = abs_err - pair_sum / (float(D) * float(D))
    sq = (mean - y) ** 2
    zero = var == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        dss = np.where(zero, np.inf, sq / var + np.log(var))
    iscore, covered = np.empty((lev.masses.size, n)), np.empty((lev.masses.size, n), bool)
    for i, mass in enumerate(lev.masses):
        iscore[i], covered[i] = interval_scores(quant[lev.ends[i, 0]], quant[lev.ends[i, 1]], y, mass)
    return {"crps": crps, "crps_fair": abs_err - pair_sum / (float(D) * float(D - 1)), "squared_error": sq, "dss": dss,
            "n_zero_var": int(zero.sum()), "pit": (below + 0.5 * equal) / D, "n_below": below, "n_equal": equal,
            "mean": mean, "sd": np.sqrt(var), "quantiles": quant[:Q].copy(), "pinball": pinball[:Q].copy(),
            "interval_score": iscore, "covered": covered,
            "mean_crps": float(crps.mean()), "se_crps": float(crps.std() / math.sqrt(n)) if n > 1 else 0.0,
            "mean_pinball": pinball[:Q].mean(axis=1), "mean_interval_score": iscore.mean(axis=1),
            "coverage": covered.mean(axis=1), "rmse": float(math.sqrt(sq.mean())),
            "q": lev.q.copy(), "intervals": lev.masses.copy(), "n_draws": int(D)}


def predictive_scores(sampler, X, y, likelihood, points=None, offset=None, draws=None, excluded=None, random_seed=0,
                      quantiles=DEFAULT_QUANTILES, intervals=DEFAULT_INTERVALS) -> dict:
    """Proper scoring rules of the posterior predictive at the rows of ``X`` against the observed ``y``, computed on the
    device from the replicated observations :func:`~pymc_bart_amd.posterior_predictive` would return for the same
    arguments (``sampler``, ``likelihood``, ``points``, ``offset``, ``draws``, ``excluded``, ``random_seed``: as there),
    without that matrix.  ``quantiles``: levels in [0, 1]; ``intervals``: masses ``c`` in (0, 1) of central intervals
    ``[q((1 - c) / 2), q((1 + c) / 2)]``; together at most 16 levels.  Between 2 and 16384 draws.  The categorical
    family is refused (class labels have no order); a two-output mean/scale fit has one ``y_rep`` per row and is taken.

    Per row, arrays ``(n_rows,)``: ``crps = E|Y - y| - E|Y - Y'| / 2`` over the draws (``crps_fair``: the pairs
    ``Y != Y'`` only, ``D (D - 1)`` of them), ``squared_error = (mean - y)^2``, ``dss = (mean - y)^2 / var + log var``
    (``inf`` where the draws of a row are all equal; ``n_zero_var`` counts those rows), ``pit``, ``n_below``,
    ``n_equal`` (:func:`~pymc_bart_amd.predictive_pit`'s), ``mean``, ``sd``; ``quantiles`` and ``pinball`` ``(Q,
    n_rows)`` for the levels of ``quantiles``; ``interval_score`` ``(I, n_rows)`` -- the width plus ``2 / (1 - c)`` times
    the distance by which ``y`` lies outside -- and ``covered`` ``(I, n_rows)``.  Over the rows: ``mean_crps``,
    ``se_crps`` (the standard deviation of ``crps`` over ``sqrt(n_rows)``), ``mean_pinball`` ``(Q,)``,
    ``mean_interval_score`` and ``coverage`` ``(I,)``, ``rmse``.  And ``q``, ``intervals``, ``n_draws``, ``n_capped``,
    ``n_exhausted``.  Rows are processed in blocks of at most ``PGB_PW_BLOCK_BYTES`` of device scratch; results depend
    on neither the blocking nor the order of the draws."""
    if getattr(likelihood, "family", None) == "categorical":
        raise ValueError("the categorical family is not scored by rank: class labels have no order (score it by its log "
                         "density: log_predictive_density)")
    job = _Job(sampler, X, likelihood, points, offset, draws, excluded, random_seed, y=y, pit=True)
    D = check_n_draws(job.D)
    lev = Levels(quantiles, intervals)
    be = score_backend(job.backend() if job.backend is not None else None)
    lib, mem = be.lib, be.mem
    replicate = Replicator(lib, job, job.seed)
    n, K, p = job.n, job.K, job.p
    per_row = 8 * (p + K * (D + 1) + (D if K > 1 else 0) + lev.n_out + 1 + (1 if job.aux is not None else 0))
    stats = np.empty((lev.n_out, n))
    for blk in job.blocks(be, per_row, predict=True):
        r0, r1, nb, md = blk.r0, blk.r1, blk.nb, blk.md
        rd = md if K == 1 else mem.empty((D * nb,), np.float64)  # (K = 1: in place)
        replicate(be, md, nb, r0, blk.od, rd)
        yd = mem.from_host(job.y[r0:r1])
        stats[:, r0:r1] = score_block(lib, mem, rd, D, nb, nb, yd, lev.all)
    res = result(stats, job.y, D, lev)
    res.update(replicate.info)
    return res


def score_matrix(y_rep, y, quantiles=DEFAULT_QUANTILES, intervals=DEFAULT_INTERVALS, backend=None) -> dict:
    """:func:`predictive_scores`' dict (without ``n_capped`` and ``n_exhausted``) for a matrix ``y_rep`` ``(D, n)`` of
    replicated observations held on the host and the observed ``y`` ``(n,)`` (uploaded in blocks of columns of at most
    ``PGB_PW_BLOCK_BYTES``)."""
    a = np.asarray(y_rep, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError(f"y_rep must be a matrix (draws, rows), got shape {a.shape}")
    D, n = check_n_draws(a.shape[0]), int(a.shape[1])
    y = check_y(y, n)
    lev = Levels(quantiles, intervals)
    if not np.all(np.isfinite(a)):
        raise ValueError("y_rep must be finite")
    be = score_backend(backend)
    stats = np.empty((lev.n_out, n))
    for r0, r1, md, yd in matrix_blocks(be, 8 * (D + 1 + lev.n_out), a, y):
        stats[:, r0:r1] = score_block(be.lib, be.mem, md, D, r1 - r0, r1 - r0, yd, lev.all)
    return result(stats, y, D, lev)
