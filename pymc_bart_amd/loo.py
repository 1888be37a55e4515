"""Scoring a fit, continued: PSIS-LOO of posterior draws on the device (``pgb_psis_rows``, include/pgbart_pointwise.h).

Leave-one-out cross-validation by Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry; what
ArviZ's ``loo`` computes from the pointwise matrix): per row ``elpd_loo_i`` and the Pareto shape ``pareto_k_i`` that
says whether the row's estimate can be trusted.  The numeric contract is ``include/pgbart_psis.h``.

* :func:`loo` scores a fit: every block of rows has its pointwise matrix written to device scratch by the tree walk
  of :mod:`pymc_bart_amd.pointwise` and smoothed there -- nothing of size ``draws x rows`` reaches the host.
* :func:`psis_loo_matrix` takes a ``(D, n)`` matrix the caller already has on the host.
* :func:`loo_pit` and :func:`loo_predictive` are the leave-one-out checks that need the smoothed weights themselves:
  the LOO-PIT of the observed ``y`` and the LOO predictive mean / sd (residuals), each the self-normalised sum
  ``sum_d w_d g_d / sum_d w_d`` of a functional of the draws' predictions.  ``pgb_psis_expect`` folds the functional
  into the kernel that owns the weights, so the weights matrix never exists and ``n`` numbers per output reach the
  host.  :func:`psis_expectation_matrix` does the same for two ``(D, n)`` matrices held on the host.

HIP backend only.  At most :data:`MAX_DRAWS` draws, and a tail of at most :data:`MAX_TAIL` (reached only by a small
``reff`` with thousands of draws); ``reff`` is the caller's (1.0: independent draws;
:func:`~pymc_bart_amd.relative_efficiency` computes it from the chains).
"""

from __future__ import annotations

import math
import warnings

import numpy as np

from ._stored import check_seed, hip_only, matrix_blocks
from .pointwise import ScoringJob

MAX_DRAWS = 16384  # PGB_PSIS_MAX_DRAWS (include/pgbart_psis.h)
MAX_TAIL = 448     # PGB_PSIS_MAX_TAIL
CLAMP = 2047.0     # pgb_clamp_loglik
G_MAX = 1e150      # PGB_PSIS_G_MAX: the values of g are held within +-G_MAX
KINDS = {"value": 0, "pit": 1}  # PGB_PSIS_G_VALUE, PGB_PSIS_G_PIT


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
    be = hip_only(backend, "PSIS-LOO runs")
    out = np.empty((2, n))
    for r0, r1, md in matrix_blocks(be, 8 * (D + 2), ll):
        out[:, r0:r1] = _psis_block(be.lib, be.mem, md, D, r1 - r0, r1 - r0, M)
    return _result(out[0].copy(), out[1].copy(), D, M, n_clamped)


def loo(sampler, X, y, likelihood, points=None, offset=None, draws=None, reff: float = 1.0) -> dict:
    """PSIS-LOO of a fit, on the device.  The arguments are :func:`~pymc_bart_amd.log_predictive_density`'s, and
    ``reff`` the relative efficiency of the draws (1.0 unless the caller has computed it from the chains).

    Returns ``elpd_loo_i``, ``pareto_k_i``, ``lppd_i`` (the bits of ``log_predictive_density``), ``p_loo_i = lppd_i -
    elpd_loo_i``, their sums ``elpd_loo`` and ``p_loo``, ``se_elpd_loo = sqrt(n var(elpd_loo_i))``,
    ``khat_threshold = min(1 - 1 / log10(D), 0.7)``, ``n_high_k`` (the rows above it: a ``UserWarning`` names them),
    ``tail_len``, ``n_draws`` and ``n_clamped``.  ``pareto_k_i`` is ``inf`` where the tail was too short or too
    degenerate for a fit (then the row's weights are not smoothed)."""
    job = ScoringJob(sampler, X, y, likelihood, points, offset, draws)
    M = tail_length(job.D, reff)
    out = np.empty((2, job.n))

    def smooth(be, blk):
        out[:, blk.r0:blk.r1] = _psis_block(be.lib, be.mem, blk.md, job.D, blk.nb, blk.nb, M)

    _, stats, clamped = job.run(matrix=True, summary=True, on_block=smooth)
    return _result(out[0].copy(), out[1].copy(), job.D, M, clamped, lppd_i=stats[0].copy())


# ---------------------------------------------------------------------- PSIS-weighted expectations (pgb_psis_expect)
def _expect_block(lib, mem, md, D: int, nb: int, ld: int, M: int, g_ptr: int, ldg: int, yd, kind: int) -> np.ndarray:
    """``(2 + n_e, nb)`` = (elpd_loo_i, k_i, E_0[, E_1]) of the device matrices ``md`` ``[D][ld]`` and ``g_ptr``
    ``[D][ldg]`` (a device address: an output of a ``[D][K][nb]`` buffer is ``ptr + 8 k nb`` with ``ldg = K nb``)."""
    rows = 2 + (2 if kind == KINDS["value"] else 1)
    od = mem.empty((rows * nb,), np.float64)
    rc = lib.psis_expect_entry_point()(mem.ptr(md), D, nb, ld, M, g_ptr, ldg, None if yd is None else mem.ptr(yd), kind,
                                       mem.ptr(od), mem.stream_ptr)
    lib.check(rc, "pgb_psis_expect")
    return mem.to_host(od).reshape(rows, nb)


def _sd(e1: np.ndarray, e2: np.ndarray) -> np.ndarray:
    return np.sqrt(np.maximum(e2 - e1 * e1, 0.0))


def psis_expectation_matrix(ll, g, y=None, kind: str = "value", reff: float = 1.0, backend=None) -> dict:
    """PSIS-weighted expectations of ``g`` ``(D, n)`` under the leave-one-out weights of the pointwise log-likelihood
    matrix ``ll`` ``(D, n)``, both held on the host (what :func:`~pymc_bart_amd.pointwise_log_likelihood` and
    :func:`~pymc_bart_amd.posterior_predictive` / ``sample_posterior`` return).  ``kind="value"``: ``loo_mean =
    E[g]`` and ``loo_sd = sqrt(max(E[g^2] - E[g]^2, 0))`` per row; ``kind="pit"``: ``loo_pit = E[(g < y) + (g == y) /
    2]`` of the observed ``y`` ``(n,)`` (the mid-p form).  Blocking, clamp count and the k warning are
    :func:`psis_loo_matrix`'s, whose dict is returned next to the new keys.  ``g`` is held within +-1e150."""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[1] < 1:
        raise ValueError(f"ll must be a matrix (draws, rows), got shape {ll.shape}")
    g = np.asarray(g, dtype=np.float64)
    if g.shape != ll.shape:
        raise ValueError(f"g must have ll's shape {ll.shape}, got {g.shape}")
    if kind not in KINDS:
        raise ValueError(f"kind must be 'value' or 'pit', got {kind!r}")
    D, n = int(ll.shape[0]), int(ll.shape[1])
    M = tail_length(D, reff)
    if not np.all(np.isfinite(ll)):
        raise ValueError("ll must be finite")
    if np.any(np.isnan(g)):
        raise ValueError("g must not hold NaN")
    yy = None
    if kind == "pit":
        if y is None:
            raise ValueError("kind='pit' needs the observed y, one value per row")
        yy = np.asarray(y, dtype=np.float64)
        if yy.shape != (n,):
            raise ValueError(f"y must hold one value per row: shape ({n},), got {yy.shape}")
        if not np.all(np.isfinite(yy)):
            raise ValueError("y must be finite")
    n_clamped = int(np.sum((ll <= -CLAMP) | (ll >= CLAMP)))
    if n_clamped:
        ll = np.clip(ll, -CLAMP, CLAMP)
    be = hip_only(backend, "PSIS-LOO runs")
    out = np.empty((2 + (2 if kind == "value" else 1), n))
    for r0, r1, md, gd, yd in matrix_blocks(be, 8 * (2 * D + 5), ll, g, yy):
        out[:, r0:r1] = _expect_block(be.lib, be.mem, md, D, r1 - r0, r1 - r0, M, be.mem.ptr(gd), r1 - r0, yd, KINDS[kind])
    res = _result(out[0].copy(), out[1].copy(), D, M, n_clamped)
    if kind == "pit":
        res["loo_pit"] = out[2].copy()
    else:
        res["loo_mean"] = out[2].copy()
        res["loo_sd"] = _sd(out[2], out[3])
    return res


def _expect_job(sampler, X, y, likelihood, points, offset, draws, reff, random_seed, mode: str):
    """The validated job of :func:`loo_pit` / :func:`loo_predictive` -- everything checked on the host before a
    backend is touched -> (job, tail length, seed)."""
    from .predictive import check_domain, check_family

    family = check_family(likelihood) if mode != "mu" else None   # (no sampler: refused by name)
    job = ScoringJob(sampler, X, y, likelihood, points, offset, draws)
    M = tail_length(job.D, reff)
    seed = check_seed(random_seed)
    if family is not None and family != "compiled":  # (a sampler body owns its domain)
        check_domain(family, job.params)
    return job, M, seed


def _run_expect(job, M: int, seed: int, mode: str):
    """Per block of rows, with the block's pointwise matrix in device scratch: ``pgb_predict`` -> (``pgb_ppc_draw``, in
    place for K = 1 | ``pgb_add_offset``) -> ``pgb_psis_expect``.  ``mode``: "pit" (y_rep against y), "y" (y_rep),
    "mu" (the linear predictor, one call per output).  -> (psis (2, n), E (calls, n_e, n), row stats, n_clamped, info)."""
    D, K, n = job.D, job.K, job.n
    n_e = 1 if mode == "pit" else 2
    kind = KINDS["pit" if mode == "pit" else "value"]
    psis = np.empty((2, n))
    E = np.empty((K if mode == "mu" else 1, n_e, n))
    info = {"n_capped": 0, "n_exhausted": 0}
    from .predictive import Replicator

    replicate = []  # (made with the first block: it needs the backend's library)

    def expect(be, blk):
        lib, mem, md, od, nb, r0, r1 = be.lib, be.mem, blk.md, blk.od, blk.nb, blk.r0, blk.r1
        gd = job.predict(be, blk.xd, nb)  # [D][K][nb]
        if mode == "mu":
            if od is not None:
                lib.check(lib.add_offset_entry_point()(mem.ptr(gd), D, K, nb, mem.ptr(od), mem.stream_ptr), "pgb_add_offset")
            for k in range(K):
                o = _expect_block(lib, mem, md, D, nb, nb, M, mem.ptr(gd) + 8 * k * nb, K * nb, None, kind)
                E[k, :, r0:r1] = o[2:]
        else:
            if not replicate:
                replicate.append(Replicator(lib, job, seed))
            rd = gd if K == 1 else mem.empty((D * nb,), np.float64)  # (K = 1: in place)
            replicate[0](be, gd, nb, r0, od, rd)
            info.update(replicate[0].info)
            o = _expect_block(lib, mem, md, D, nb, nb, M, mem.ptr(rd), nb, blk.yd if mode == "pit" else None, kind)
            E[0, :, r0:r1] = o[2:]
        psis[:, r0:r1] = o[:2]

    scratch = 2 + n_e + K * D + (D if K > 1 and mode != "mu" else 0) + (1 if mode != "mu" and job.aux is not None else 0)
    _, stats, clamped = job.run(matrix=True, summary=True, on_block=expect, scratch=scratch)
    return psis, E, stats, clamped, info


def loo_pit(sampler, X, y, likelihood, points=None, offset=None, draws=None, reff: float = 1.0, random_seed=0) -> dict:
    """The leave-one-out probability integral transform of the observed ``y`` (what ArviZ's ``loo_pit`` computes from
    the weights matrix), on the device: ``loo_pit[i] = sum_d w_di ((y_rep[d, i] < y[i]) + (y_rep[d, i] == y[i]) / 2) /
    sum_d w_di`` with ``w_.i`` the Pareto-smoothed importance weights of row ``i`` and ``y_rep`` the replicated
    observations :func:`~pymc_bart_amd.posterior_predictive` gives for the same ``random_seed`` (a value per seed,
    position of the draw and global row: the result does not depend on ``PGB_PW_BLOCK_BYTES``).  Uniform for a
    calibrated model; the mid-p form keeps that for the discrete families.

    The arguments are :func:`loo`'s; a compiled likelihood without a sampler body, and the callback family, have no
    sampler and are refused.  Returns
    :func:`loo`'s dict plus ``loo_pit``, ``n_capped`` and ``n_exhausted`` (``include/pgbart_ppc.h``).  Nothing of size
    ``draws x rows`` reaches the host."""
    job, M, seed = _expect_job(sampler, X, y, likelihood, points, offset, draws, reff, random_seed, "pit")
    psis, E, stats, clamped, info = _run_expect(job, M, seed, "pit")
    res = _result(psis[0].copy(), psis[1].copy(), job.D, M, clamped, lppd_i=stats[0].copy())
    res["loo_pit"] = E[0, 0].copy()
    res.update(info)
    return res


def loo_predictive(sampler, X, y, likelihood, points=None, offset=None, draws=None, reff: float = 1.0, random_seed=0,
                   kind: str = "mu") -> dict:
    """The leave-one-out predictive mean and sd of every row (``loo_expectation`` of ArviZ), on the device:
    ``loo_mean = E[g]`` and ``loo_sd = sqrt(max(E[g^2] - E[g]^2, 0))`` under the row's Pareto-smoothed weights.

    ``kind="mu"``: ``g`` is the linear predictor ``mu_d(X[i]) + offset`` -- arrays ``(n,)``, or ``(K, n)`` for trees
    with K > 1 outputs (one call per output); any family :func:`loo` takes.  ``kind="y"``: ``g`` is the replicated
    observation ``y_rep[d, i]`` of :func:`~pymc_bart_amd.posterior_predictive` under ``random_seed`` (families with a
    sampler only); for K = 1 also ``loo_residual = y - loo_mean``; ``n_capped`` / ``n_exhausted`` are reported.
    Returns :func:`loo`'s dict next to these keys.  Nothing of size ``draws x rows`` reaches the host."""
    if kind not in ("mu", "y"):
        raise ValueError(f"kind must be 'mu' or 'y', got {kind!r}")
    job, M, seed = _expect_job(sampler, X, y, likelihood, points, offset, draws, reff, random_seed, kind)
    psis, E, stats, clamped, info = _run_expect(job, M, seed, kind)
    res = _result(psis[0].copy(), psis[1].copy(), job.D, M, clamped, lppd_i=stats[0].copy())
    mean, sd = E[:, 0].copy(), _sd(E[:, 0], E[:, 1])
    if mean.shape[0] == 1:
        mean, sd = mean[0], sd[0]
    res["loo_mean"], res["loo_sd"] = mean, sd
    if kind == "y":
        if job.K == 1:
            res["loo_residual"] = job.y - mean
        res.update(info)
    return res
