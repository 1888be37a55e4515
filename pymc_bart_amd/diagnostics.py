"""Checking a fit: per-row R-hat and effective sample sizes of the chains, and the relative efficiency ``r_eff`` that
PSIS-LOO takes, on the device (``pgb_chain_diag``, ``include/pgbart_diag.h``).

The question that comes before every other way of reading a fit -- have the chains mixed at this row? -- answered
without the ``(draws, K, rows)`` array leaving the device: rank-normalised split R-hat, bulk, tail and mean ESS
(Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; what ArviZ's ``rhat`` / ``ess`` compute column by column).

* :func:`convergence` diagnoses the BART function of a fit at the rows of ``X``: per block of rows one ``pgb_predict``
  into device scratch and one ``pgb_chain_diag`` on it.
* :func:`relative_efficiency` gives ``r_eff`` of every row's likelihood ``exp(ll)`` -- what ``loo(..., reff=)``,
  ``loo_pit`` and ``loo_predictive`` take -- from the pointwise matrix in device scratch, exactly as ``loo`` obtains it.
* :func:`diagnose_matrix` takes a ``(D, n)`` chain-major matrix the caller already has on the host.

HIP backend only.  At least 4 draws per chain, at most :data:`MAX_CHAINS` chains; after the split (the middle draw of
an odd chain is dropped) at most :data:`MAX_DRAWS` draws, :data:`MAX_DRAWS_MEAN` for :func:`relative_efficiency`.
"""

from __future__ import annotations

import functools
import math
from statistics import NormalDist

import numpy as np

from ._stored import chains, hip_only, matrix_blocks
from .pointwise import ScoringJob
from .summary import SummaryJob

MAX_DRAWS = 8192        # PGB_DIAG_MAX_DRAWS (include/pgbart_diag.h)
MAX_DRAWS_MEAN = 16384  # PGB_DIAG_MAX_DRAWS_MEAN
MAX_CHAINS = 64         # PGB_DIAG_MAX_CHAINS
NOUT = 10               # PGB_DIAG_NOUT
TRANSFORMS = {"identity": 0, "exp_shift": 1}  # PGB_DIAG_*
ALL, MEAN_ONLY = 0, 1   # PGB_DIAG_ALL, PGB_DIAG_MEAN_ONLY
RHAT_THRESHOLD = 1.01   # Vehtari et al. 2021
ESS_PER_CHAIN = 100.0   # ... ESS below 100 per chain is too low


@functools.lru_cache(maxsize=8)
def _z_table(S: int) -> np.ndarray:
    inv = NormalDist().inv_cdf
    z = np.array([inv((0.5 * i + 1.0 - 0.375) / (S + 0.25)) for i in range(2 * S - 1)], dtype=np.float64)
    z.setflags(write=False)
    return z


def z_table(S: int) -> np.ndarray:
    """The ``2 S - 1`` z-scores ``ndtri((r - 3/8) / (S + 1/4))`` of the average ranks ``r = 1, 1.5, .., S``."""
    return _z_table(int(S))


def kept_draws(n_chains: int, n_per_chain: int, stats: int = ALL) -> int:
    """``S = 2 n_chains (n_per_chain // 2)``, the draws kept by the split; checked against the device's limits."""
    n_chains, n_per_chain = int(n_chains), int(n_per_chain)
    if not 1 <= n_chains <= MAX_CHAINS:
        raise ValueError(f"n_chains must be in [1, {MAX_CHAINS}], got {n_chains}")
    if n_per_chain < 4:
        raise ValueError(f"chain diagnostics need at least 4 draws per chain, got {n_per_chain}")
    S = 2 * n_chains * (n_per_chain // 2)
    cap = MAX_DRAWS_MEAN if stats == MEAN_ONLY else MAX_DRAWS
    if S > cap:
        raise ValueError(f"chain diagnostics on the device take at most {cap} draws after the split, got {S} "
                         f"({n_chains} chains x {n_per_chain}; thin them: draws_per_chain=)")
    return S


def _diag_block(lib, mem, md, n_chains: int, n_per_chain: int, n_cols: int, ld: int, code: int, stats: int) -> np.ndarray:
    """``(NOUT, n_cols)`` of the device matrix ``md`` ``[n_chains n_per_chain][ld]``."""
    S = 2 * n_chains * (n_per_chain // 2)
    z = None if stats == MEAN_ONLY else z_table(S)
    od = mem.empty((NOUT * n_cols,), np.float64)
    rc = lib.chain_diag_entry_point()(mem.ptr(md), n_chains, n_per_chain, n_cols, ld, code, stats,
                                      None if z is None else z.ctypes.data, 1.0 / math.log10(S), mem.ptr(od), mem.stream_ptr)
    lib.check(rc, "pgb_chain_diag")
    return mem.to_host(od).reshape(NOUT, n_cols)


def _public(stats: np.ndarray, n_chains: int, n_per_chain: int) -> dict:
    """``stats`` ``(NOUT, ...)`` -> the public dict (arrays of the trailing shape)."""
    var, ess_mean = stats[7].copy(), stats[5].copy()
    with np.errstate(invalid="ignore"):
        rhat = np.sqrt(np.maximum(stats[0], stats[1]))
    return {"rhat": rhat, "ess_bulk": stats[2].copy(), "ess_tail": np.minimum(stats[3], stats[4]), "ess_mean": ess_mean,
            "mcse_mean": np.sqrt(var / ess_mean), "mean": stats[6].copy(), "sd": np.sqrt(var),
            "n_constant": int(np.sum(stats[8] != 0.0)), "n_chains": int(n_chains), "n_per_chain": int(n_per_chain)}


def diagnose_matrix(a, n_chains: int, transform: str = "identity", backend=None) -> dict:
    """Convergence diagnostics of every column of ``a`` ``(D, n)``, a matrix of draws held on the host, chain-major:
    row ``c * (D // n_chains) + i`` is draw ``i`` of chain ``c``.  ``transform="exp_shift"`` diagnoses ``exp(a -
    max(a))`` per column (the likelihood of a log-likelihood column).  Columns are uploaded in blocks of at most
    ``PGB_PW_BLOCK_BYTES``.

    Returns, each ``(n,)``: ``rhat`` (the larger of the rank-normalised split R-hat of the values and of their
    absolute deviations from the median), ``ess_bulk``, ``ess_tail`` (the smaller of the ESS of the 5 % and the 95 %
    quantile), ``ess_mean``, ``mcse_mean = sd / sqrt(ess_mean)``, ``mean``, ``sd``; and ``n_constant`` (columns without
    variation: R-hat 1, ESS = the number of draws), ``n_chains``, ``n_per_chain``."""
    if transform not in TRANSFORMS:
        raise ValueError(f"unknown transform {transform!r}: use one of {', '.join(TRANSFORMS)}")
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError(f"a must be a matrix (draws, columns), got shape {a.shape}")
    D, n = int(a.shape[0]), int(a.shape[1])
    n_chains = int(n_chains)
    if n_chains < 1 or D % n_chains:
        raise ValueError(f"the {D} draws do not divide into n_chains = {n_chains} chains of equal length")
    npc = D // n_chains
    kept_draws(n_chains, npc)
    if not np.all(np.isfinite(a)):
        raise ValueError("a must be finite")
    be = hip_only(backend, "chain diagnostics run")
    stats = np.empty((NOUT, n))
    for r0, r1, md in matrix_blocks(be, 8 * (D + NOUT), a):
        stats[:, r0:r1] = _diag_block(be.lib, be.mem, md, n_chains, npc, r1 - r0, r1 - r0, TRANSFORMS[transform], ALL)
    return _public(stats, n_chains, npc)


def _chain_draws(sampler, draws_per_chain, stats: int):
    """-> (indexes of the stored draws, chain-major; n_chains; n_per_chain) of the sampler's own chains."""
    lengths = [int(part.forest_idx.shape[0]) for part in chains(sampler)]
    if draws_per_chain is None:
        if len(set(lengths)) != 1:
            raise ValueError(f"the chains hold {lengths} draws: chains of unequal length need draws_per_chain= "
                             "(the last draws of every chain; nothing is truncated silently)")
        N = lengths[0]
    else:
        N = int(draws_per_chain)
        if N > min(lengths):
            raise ValueError(f"draws_per_chain = {N}, but the chains hold {lengths} draws")
    kept_draws(len(lengths), N, stats)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    idx = np.concatenate([starts[c] + lengths[c] - N + np.arange(N, dtype=np.int64) for c in range(len(lengths))])
    return idx, len(lengths), N


def convergence(sampler, X, draws_per_chain=None, transform: str = "identity", offset=None, excluded=None) -> dict:
    """Per-row convergence diagnostics of the BART function of a fit at the rows of ``X``, computed on the device.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns; the chains are its
    own (each part's stored draws).  ``draws_per_chain=N`` takes the last ``N`` draws of every chain; chains of unequal
    length without it are a ``ValueError``.  ``transform``: ``"identity"`` only for now.  ``offset`` ``(K, n_rows)``
    shifts every column by a constant: it changes ``mean`` and nothing else.  ``excluded``: as in ``sample_posterior``.

    Returns :func:`diagnose_matrix`'s keys with arrays ``(n_rows, K)``, and ``n_high_rhat`` (rows with R-hat above
    1.01) and ``n_low_ess`` (rows whose bulk or tail ESS is below ``100 x n_chains``), the published thresholds.
    Rows are processed in blocks of at most ``PGB_PW_BLOCK_BYTES`` of device scratch; the result does not depend on
    the blocking, nor on the order of the chains."""
    if transform != "identity":
        raise ValueError(f"convergence takes transform='identity' only for now, not {transform!r}")
    idx, n_chains, npc = _chain_draws(sampler, draws_per_chain, ALL)
    job = SummaryJob(sampler, X, idx, None, None, "identity", offset, excluded)

    def diag(be, blk):
        n_cols = job.K * blk.nb
        return _diag_block(be.lib, be.mem, blk.md, n_chains, npc, n_cols, n_cols, TRANSFORMS["identity"], ALL)

    stats, _ = job.run(on_block=diag, out_rows=NOUT)                            # (NOUT, K, n)
    res = _public(np.ascontiguousarray(np.moveaxis(stats, 1, 2)), n_chains, npc)  # arrays (n, K)
    if job.offset is not None:
        res["mean"] = res["mean"] + job.offset.T
    res["n_high_rhat"] = int(np.sum(res["rhat"] > RHAT_THRESHOLD))
    res["n_low_ess"] = int(np.sum(np.minimum(res["ess_bulk"], res["ess_tail"]) < ESS_PER_CHAIN * n_chains))
    return res


def relative_efficiency(sampler, X, y, likelihood, points=None, offset=None, draws_per_chain=None) -> dict:
    """The relative efficiency of the draws for every row's likelihood, on the device: ``reff_i = min(ess_mean_i / S,
    1)`` with ``ess_mean_i`` the effective sample size of ``exp(ll[., i])`` over the sampler's own chains (ArviZ's
    ``ess(..., method="mean", relative=True)`` of the likelihood, what its ``loo`` computes ``reff`` from).

    The arguments are :func:`~pymc_bart_amd.loo`'s; ``points`` holds one point per draw USED (all of them, or with
    ``draws_per_chain=N`` the last ``N`` of every chain, chain after chain).  Per block of rows the pointwise
    log-likelihood is written to device scratch as ``loo`` does it and diagnosed there; nothing of size ``draws x
    rows`` reaches the host.

    Returns ``reff_i`` ``(n_rows,)``, ``reff`` (their mean: the scalar ``loo(..., reff=res["reff"])`` takes),
    ``reff_min``, ``ess_mean_i``, ``n_draws`` (after the split), ``n_chains``, ``n_per_chain`` and ``n_clamped``."""
    idx, n_chains, npc = _chain_draws(sampler, draws_per_chain, MEAN_ONLY)
    job = ScoringJob(sampler, X, y, likelihood, points, offset, idx)
    S = 2 * n_chains * (npc // 2)
    ess = np.empty(job.n)

    def diag(be, blk):
        ess[blk.r0:blk.r1] = _diag_block(be.lib, be.mem, blk.md, n_chains, npc, blk.nb, blk.nb, TRANSFORMS["exp_shift"],
                                         MEAN_ONLY)[5]

    _, _, clamped = job.run(matrix=True, summary=False, on_block=diag, scratch=NOUT)
    reff_i = np.minimum(ess / S, 1.0)
    return {"reff_i": reff_i, "reff": float(reff_i.mean()), "reff_min": float(reff_i.min()), "ess_mean_i": ess,
            "n_draws": S, "n_chains": n_chains, "n_per_chain": npc, "n_clamped": int(clamped)}
