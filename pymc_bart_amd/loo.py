"""Scoring a fit, continued: PSIS-LOO of posterior draws on the device (``pgb_psis_rows``, include/pgbart_pointwise.h).

Leave-one-out cross-validation by Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry; what
ArviZ's ``loo`` computes from the pointwise matrix): per row ``elpd_loo_i`` and the Pareto shape ``pareto_k_i`` that
says whether the row's estimate can be trusted.  The numeric contract is ``include/pgbart_psis.h``.

* :func:`loo` scores a fit: every block of rows has its pointwise matrix written to device scratch by the tree walk
  of :mod:`pymc_bart_amd.pointwise` and smoothed there -- nothing of size ``draws x rows`` reaches the host.
* :func:`psis_loo_matrix` takes a ``(D, n)`` matrix the caller already has on the host.

HIP backend only.  At most :data:`MAX_DRAWS` draws, and a tail of at most :data:`MAX_TAIL` (reached only by a small
``reff`` with thousands of draws); ``reff`` is the caller's (1.0: independent draws).
"""

from __future__ import annotations

import math
import warnings

import numpy as np

from . import _abi
from .pointwise import _Job, _block_bytes

MAX_DRAWS = 16384  # PGB_PSIS_MAX_DRAWS (include/pgbart_psis.h)
MAX_TAIL = 448     # PGB_PSIS_MAX_TAIL
CLAMP = 2047.0     # pgb_clamp_loglik


def tail_length(D: int, reff: float = 1.0) -> int:
    """``ceil(min(D / 5, 3 sqrt(D / reff)))``: the number of largest importance ratios that are smoothed."""
    reff = float(reff)
    if not (0.0 < reff <= 1.0):
        raise ValueError(f"reff must be in (0, 1], got {reff!r}")
    D = int(D)
    if D < 2:
        raise ValueError(f"PSIS needs at least 2 draws, got {D}")
    if D > MAX_DRAWS:
        raise ValueError(f"PSIS on the device takes at most {MAX_DRAWS} draws, got {D} (thin them: draws=)")
    M = int(math.ceil(min(D / 5.0, 3.0 * math.sqrt(D / reff))))
    if M > MAX_TAIL:
        raise ValueError(f"reff = {reff:g} with {D} draws gives a tail of {M} values, the device takes {MAX_TAIL}")
    return M


def khat_threshold(D: int) -> float:
    return min(1.0 - 1.0 / math.log10(D), 0.7)


def _hip(backend):
    from .sampler import default_backend

    be = backend if backend is not None else default_backend()
    if be.lib.backend_name != "hip-gfx950":
        raise _abi.PGBError(f"PSIS-LOO runs on the HIP backend only, not on {be.lib.backend_name}")
    return be


def _psis_block(lib, mem, md, D: int, nb: int, ld: int, M: int) -> np.ndarray:
    """``(2, nb)`` = (elpd_loo_i, k_i) of the device matrix ``md`` ``[D][ld]``."""
    od = mem.empty((2 * nb,), np.float64)
    rc = lib.psis_entry_point()(mem.ptr(md), D, nb, ld, M, mem.ptr(od), mem.stream_ptr)
    lib.check(rc, "pgb_psis_rows")
    return mem.to_host(od).reshape(2, nb)


def _result(elpd_i, k_i, D: int, M: int, n_clamped: int, lppd_i=None) -> dict:
    n = elpd_i.size
    thr = khat_threshold(D)
    n_high = int(np.sum(k_i > thr))
    res = {"elpd_loo_i": elpd_i, "pareto_k_i": k_i, "elpd_loo": float(elpd_i.sum()),
           "se_elpd_loo": float(np.sqrt(n * elpd_i.var())) if n > 1 else 0.0, "khat_threshold": thr, "n_high_k": n_high,
           "tail_len": M, "n_draws": D, "n_clamped": int(n_clamped)}
    if lppd_i is not None:
        res["lppd_i"] = lppd_i
        res["p_loo_i"] = lppd_i - elpd_i
        res["p_loo"] = float(res["p_loo_i"].sum())
    if n_high > 0:
        warnings.warn(f"{n_high} of {n} rows have a Pareto k above {thr:.3f}: their elpd_loo_i cannot be trusted "
                      "(pareto_k_i says which)", UserWarning, stacklevel=3)
    return res


def psis_loo_matrix(ll, reff: float = 1.0, backend=None) -> dict:
    """PSIS-LOO of a pointwise log-likelihood matrix ``ll`` ``(D, n)`` held on the host (what
    :func:`~pymc_bart_amd.pointwise_log_likelihood` returns).  The matrix is uploaded in blocks of rows of at most
    ``PGB_PW_BLOCK_BYTES``.  Values are held within [-2047, 2047] like the library's own (``n_clamped`` counts those
    that met the bound).  Returns :func:`loo`'s dict without the ``lppd`` terms."""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[1] < 1:
        raise ValueError(f"ll must be a matrix (draws, rows), got shape {ll.shape}")
    D, n = int(ll.shape[0]), int(ll.shape[1])
    M = tail_length(D, reff)
    if not np.all(np.isfinite(ll)):
        raise ValueError("ll must be finite")
    n_clamped = int(np.sum((ll <= -CLAMP) | (ll >= CLAMP)))
    if n_clamped:
        ll = np.clip(ll, -CLAMP, CLAMP)
    be = _hip(backend)
    lib, mem = be.lib, be.mem
    block = max(64, min(n, _block_bytes() // (8 * (D + 2)) // 64 * 64))
    out = np.empty((2, n))
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        md = mem.from_host(np.ascontiguousarray(ll[:, r0:r1]))
        out[:, r0:r1] = _psis_block(lib, mem, md, D, r1 - r0, r1 - r0, M)
    return _result(out[0].copy(), out[1].copy(), D, M, n_clamped)


def loo(sampler, X, y, likelihood, points=None, offset=None, draws=None, reff: float = 1.0) -> dict:
    """PSIS-LOO of a fit, on the device.  The arguments are :func:`~pymc_bart_amd.log_predictive_density`'s, and
    ``reff`` the relative efficiency of the draws (1.0 unless the caller has computed it from the chains).

    Returns ``elpd_loo_i``, ``pareto_k_i``, ``lppd_i`` (the bits of ``log_predictive_density``), ``p_loo_i = lppd_i -
    elpd_loo_i``, their sums ``elpd_loo`` and ``p_loo``, ``se_elpd_loo = sqrt(n var(elpd_loo_i))``,
    ``khat_threshold = min(1 - 1 / log10(D), 0.7)``, ``n_high_k`` (the rows above it: a ``UserWarning`` names them),
    ``tail_len``, ``n_draws`` and ``n_clamped``.  ``pareto_k_i`` is ``inf`` where the tail was too short or too
    degenerate for a fit (then the row's weights are not smoothed)."""
    job = _Job(sampler, X, y, likelihood, points, offset, draws)
    M = tail_length(job.D, reff)
    out = np.empty((2, job.n))

    def smooth(lib, mem, md, nb, r0):
        out[:, r0:r0 + nb] = _psis_block(lib, mem, md, job.D, nb, nb, M)

    _, stats, clamped = job.run(matrix=True, summary=True, on_block=smooth)
    return _result(out[0].copy(), out[1].copy(), job.D, M, clamped, lppd_i=stats[0].copy())
