"""Reading a fit: per-row summaries of the posterior predictions on the device (``pgb_row_summary``,
``include/pgbart_rowsummary.h``).

What every notebook ends in -- ``pred.mean(0)``, ``np.quantile(pred, q, 0)``, ``az.hdi(pred)`` -- without the
``(draws, K, rows)`` array leaving the device: per block of rows one ``pgb_predict`` call writes the predictions of
all draws into device scratch and one ``pgb_row_summary`` call sorts every column over its draws and reads the mean,
the variance, the quantiles and the highest-density interval out of it.

* :func:`posterior_summary` summarises the predictions of a fit at the rows of ``X``.
* :func:`summarize_matrix` takes a ``(D, n)`` matrix the caller already has on the host.

HIP backend only.  Between 2 and :data:`MAX_DRAWS` draws, at most :data:`MAX_QUANTILES` quantiles per call.
"""

from __future__ import annotations

import math

import numpy as np

from ._stored import Job, drop_k_axis, hip_only, matrix_blocks

MAX_DRAWS = 16384    # PGB_ROWSUM_MAX_DRAWS (include/pgbart_rowsummary.h)
MAX_QUANTILES = 16   # PGB_ROWSUM_MAX_Q
TRANSFORMS = {"identity": 0, "exp": 1, "logistic": 2, "probit": 3}  # PGB_ROWSUM_*
DEFAULT_QUANTILES = (0.03, 0.5, 0.97)
DEFAULT_HDI_PROB = 0.94


def hdi_length(D: int, prob) -> int:
    """``max(floor(prob D), 1)``: the sorted draws ``i`` and ``i + hdi_length`` bound the candidate intervals
    (``importance.hdi``); 0 for ``prob=None`` (no interval)."""
    if prob is None:
        return 0
    prob = float(prob)
    if not (0.0 < prob <= 1.0):
        raise ValueError(f"hdi_prob must be in (0, 1] or None, got {prob!r}")
    return max(int(math.floor(prob * int(D))), 1)


def spec(D: int, quantiles, hdi_prob, transform):
    """-> (q array, hdi_k, transform code) of one call, checked."""
    if transform not in TRANSFORMS:
        raise ValueError(f"unknown transform {transform!r}: use one of {', '.join(TRANSFORMS)}")
    q = np.asarray([] if quantiles is None else quantiles, dtype=np.float64)
    if q.ndim != 1:
        raise ValueError(f"quantiles must be a vector of levels, got shape {q.shape}")
    if q.size > MAX_QUANTILES:
        raise ValueError(f"at most {MAX_QUANTILES} quantiles per call, got {q.size}")
    if q.size and not np.all((q >= 0.0) & (q <= 1.0)):  # (a NaN fails both comparisons)
        raise ValueError("quantiles must be in [0, 1]")
    D = int(D)
    if D < 2:
        raise ValueError(f"a summary over the draws needs at least 2 draws, got {D}")
    if D > MAX_DRAWS:
        raise ValueError(f"a summary on the device takes at most {MAX_DRAWS} draws, got {D} (thin them: draws=)")
    return np.ascontiguousarray(q), hdi_length(D, hdi_prob), TRANSFORMS[transform]


def summary_block(lib, mem, md, D: int, n_cols: int, ld: int, od, code: int, q: np.ndarray, hdi_k: int) -> np.ndarray:
    """``(2 + Q + 2, n_cols)`` of the device matrix ``md`` ``[D][ld]`` (``od``: the columns' offsets on the device)."""
    rows = 2 + q.size + 2
    sd = mem.empty((rows * n_cols,), np.float64)
    rc = lib.rowsummary_entry_point()(mem.ptr(md), D, n_cols, ld, None if od is None else mem.ptr(od), code,
                                      q.ctypes.data if q.size else None, int(q.size), int(hdi_k), mem.ptr(sd), mem.stream_ptr)
    lib.check(rc, "pgb_row_summary")
    return mem.to_host(sd).reshape(rows, n_cols)


def result(stats: np.ndarray, n: int, K: int, q: np.ndarray, hdi_prob, hdi_k: int, D: int) -> dict:
    """``stats`` ``(2 + Q + 2, K, n)`` -> the public dict (arrays ``(..., n, K)``)."""
    by = np.ascontiguousarray(np.moveaxis(stats.reshape(-1, K, n), 1, 2))  # (rows, n, K)
    Q = q.size
    var = by[1].copy()
    return {"mean": by[0].copy(), "sd": np.sqrt(var), "var": var, "quantiles": by[2:2 + Q].copy(),
            "hdi": by[2 + Q:4 + Q].copy() if hdi_k else None, "q": q.copy(),
            "hdi_prob": None if hdi_prob is None else float(hdi_prob), "n_draws": int(D)}


class SummaryJob(Job):
    """One :func:`posterior_summary` call: the job base plus the summary spec."""

    def __init__(self, sampler, X, draws, quantiles, hdi_prob, transform, offset, excluded):
        super().__init__(sampler)
        self.take_X(X)
        self.take_offset(offset)
        self.take_excluded(excluded)
        self.take_draws(draws)
        self.hdi_prob = hdi_prob
        self.q, self.hdi_k, self.code = spec(self.D, quantiles, hdi_prob, transform)
        self.take_history()

    def run(self, keep_matrix: bool = False, on_block=None, out_rows: int = 0):
        """-> (the public dict, the predictions ``(D, K, n)`` or None).  ``keep_matrix``: also copy every block's
        predictions to the host (partial dependence returns them next to their summary).  ``on_block(be, blk)``:
        another second kernel on every block's predictions ``blk.md`` ``[D][K * blk.nb]`` in place of
        ``pgb_row_summary`` (:mod:`pymc_bart_amd.diagnostics`); it returns ``(out_rows, K * blk.nb)`` and the first
        result is then the array ``(out_rows, K, n)`` itself."""
        be = self.hip_backend("posterior summaries run")
        n, D, K, p, Q = self.n, self.D, self.K, self.p, self.q.size
        rows = 2 + Q + 2 if on_block is None else int(out_rows)
        stats = np.empty((rows, K, n))
        pred = np.empty((D, K, n)) if keep_matrix else None
        for blk in self.blocks(be, 8 * (p + K * (D + 1 + rows)), predict=True):
            r0, r1, nb = blk.r0, blk.r1, blk.nb
            if on_block is None:
                got = summary_block(be.lib, be.mem, blk.md, D, K * nb, K * nb, blk.od, self.code, self.q, self.hdi_k)
            else:
                got = on_block(be, blk)
            stats[:, :, r0:r1] = got.reshape(-1, K, nb)
            if keep_matrix:
                pred[:, :, r0:r1] = be.mem.to_host(blk.md).reshape(D, K, nb)
        if on_block is not None:
            return stats, pred
        return result(stats, n, K, self.q, self.hdi_prob, self.hdi_k, D), pred


def posterior_summary(sampler, X, draws=None, quantiles=DEFAULT_QUANTILES, hdi_prob=DEFAULT_HDI_PROB,
                      transform: str = "identity", offset=None, excluded=None) -> dict:
    """Per-row summaries over the posterior draws of the BART function at the rows of ``X``, computed on the device.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns (several chains are
    summarised as one pool).  ``draws``: indexes of the stored draws (default: all; between 2 and 16384).
    ``quantiles``: up to 16 levels in [0, 1] (NumPy's default linear interpolation).  ``hdi_prob``: the mass of the
    highest-density interval (``importance.hdi``; ``None``: no interval).  ``transform``: ``"identity"``, ``"exp"``,
    ``"logistic"`` or ``"probit"`` (the normal CDF), applied to every prediction -- after ``offset`` ``(K, n_rows)``
    has been added -- before anything is summarised.  ``excluded``: covariates marginalised out by the trees' own
    counts, as in ``sample_posterior``.

    Returns ``mean``, ``sd``, ``var`` (ddof 1), each ``(n_rows, K)``; ``quantiles`` ``(Q, n_rows, K)``; ``hdi``
    ``(2, n_rows, K)`` (``None`` without ``hdi_prob``); and ``q``, ``hdi_prob``, ``n_draws``.  Rows are processed in
    blocks of at most ``PGB_PW_BLOCK_BYTES`` of device scratch; results do not depend on the blocking, nor on the
    order of the draws."""
    return SummaryJob(sampler, X, draws, quantiles, hdi_prob, transform, offset, excluded).run()[0]


def summarize_matrix(a, quantiles=DEFAULT_QUANTILES, hdi_prob=DEFAULT_HDI_PROB, transform: str = "identity",
                     backend=None) -> dict:
    """:func:`posterior_summary`'s numbers for a matrix ``a`` ``(D, n)`` of draws held on the host (uploaded in blocks
    of columns of at most ``PGB_PW_BLOCK_BYTES``): arrays ``(n,)``, ``quantiles`` ``(Q, n)``, ``hdi`` ``(2, n)``."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError(f"a must be a matrix (draws, columns), got shape {a.shape}")
    D, n = int(a.shape[0]), int(a.shape[1])
    q, hdi_k, code = spec(D, quantiles, hdi_prob, transform)
    if not np.all(np.isfinite(a)):
        raise ValueError("a must be finite")
    be = hip_only(backend, "posterior summaries run")
    stats = np.empty((2 + q.size + 2, n))
    for r0, r1, md in matrix_blocks(be, 8 * (D + 4 + q.size), a):
        stats[:, r0:r1] = summary_block(be.lib, be.mem, md, D, r1 - r0, r1 - r0, None, code, q, hdi_k)
    return drop_k_axis(result(stats, n, 1, q, hdi_prob, hdi_k, D))
