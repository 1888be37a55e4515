"""Reading a fit: posterior predictive draws on the device (``pgb_ppc_draw``, ``include/pgbart_ppc.h``).

``posterior_summary`` gives the band of the mean function; what a model predicts one will OBSERVE needs the family's
noise on top of every draw's linear predictor.  Per block of rows one ``pgb_predict`` call writes the predictors of all
draws into device scratch and one ``pgb_ppc_draw`` call turns them into replicated observations ``y_rep`` -- a
counter-based value per (seed, position of the draw, global row), so that a result depends on neither the blocking nor
the launch geometry.

* :func:`posterior_predictive` returns ``y_rep`` ``(D, n)`` -- the stand-in for ``pm.sample_posterior_predictive``.
* :func:`predictive_summary` returns its per-row mean, quantiles and HDI through ``pgb_row_summary``; nothing of size
  ``draws x rows`` reaches the host.
* :func:`predictive_pit` returns the PIT values of observed ``y`` (mid-p: ``(below + equal / 2) / D``); no matrix is
  written at all.

The ten built-in families have a sampler; the compiled and callback families have a log density only and are refused.
Rejection samplers are bounded: pairs that exhausted their attempts (``n_exhausted``) or met a cap (``n_capped``: a
Poisson rate above 2^30, a non-finite value) are counted, never silent.  HIP backend only.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .pointwise import FAMILY_OUTPUTS, FAMILY_PARAMS, MAX_OFFSET, _block_bytes, _chains, _param_matrix
from .summary import DEFAULT_HDI_PROB, DEFAULT_QUANTILES, _result, _spec, _summary_block


def _check_family(likelihood) -> str:
    family = getattr(likelihood, "family", None)
    if family in ("callback", "compiled"):
        raise ValueError(f"the {family} family has a log density only, no sampler: posterior predictive draws take the "
                         f"built-in families ({', '.join(FAMILY_PARAMS)})")
    if family not in FAMILY_PARAMS:
        raise ValueError(f"unknown likelihood family {family!r}")
    return family


def _check_domain(family: str, params: np.ndarray) -> None:
    """pgb_logpdf_prepare's domain: every param positive (and finite: ``_param_matrix``), 0 < q < 1."""
    bad = ~np.all(params > 0.0, axis=1)
    if family == "asymmetric_laplace":
        bad |= ~(params[:, 1] < 1.0)
    if np.any(bad):
        d = int(np.flatnonzero(bad)[0])
        raise ValueError(f"the params of draw {d} are outside the {family} family's domain (positive and finite; "
                         f"0 < q < 1): {params[d].tolist()}")


class _Job:
    """Everything of one call, validated on the host before a backend is touched."""

    def __init__(self, sampler, X, likelihood, points, offset, draws, excluded, random_seed, y=None, pit=False):
        parts = _chains(sampler)
        self.K = K = int(parts[0].n_outputs)
        self.m = int(parts[0].m)
        self.family = _check_family(likelihood)
        self.n_par = FAMILY_PARAMS[self.family]
        lk = int(getattr(likelihood, "n_outputs", 1))
        if lk != K:
            raise ValueError(f"the likelihood has n_outputs = {lk}, the sampler's trees n_outputs = {K}")
        want = FAMILY_OUTPUTS.get(self.family, 1)
        if (want > 0 and K != want) or (want == 0 and K < 2):
            raise ValueError(f"the {self.family} family does not take n_outputs = {K}")
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError(f"X must be a matrix (n_rows, p), got shape {X.shape}")
        self.X = np.ascontiguousarray(X)
        n, p = self.n, self.p = int(X.shape[0]), int(X.shape[1])
        self.y = None
        if pit:
            y = np.asarray(y, dtype=np.float64)
            if y.shape != (n,):
                raise ValueError(f"y must hold one value per row of X: shape ({n},), got {y.shape}")
            if not np.all(np.isfinite(y)):
                raise ValueError("y must be finite")
            self.y = np.ascontiguousarray(y)
        self.offset = None
        if offset is not None:
            off = np.asarray(offset, dtype=np.float64)
            if off.shape == (n,) and K == 1:
                off = off[None, :]
            if off.shape != (K, n):
                raise ValueError(f"offset must have shape (n_outputs, n_rows) = ({K}, {n}), got {off.shape}")
            if not np.all(np.isfinite(off)) or np.max(np.abs(off)) > MAX_OFFSET:
                raise ValueError(f"offset must be finite and within +-{MAX_OFFSET:g}")
            self.offset = np.ascontiguousarray(off)
        excl = np.asarray([] if excluded is None else excluded, dtype=np.int64).ravel()
        if excl.size and (excl.min() < 0 or excl.max() >= p):
            raise ValueError(f"excluded must index the {p} columns of X")
        self.excluded = np.ascontiguousarray(excl, dtype=np.int32)
        total = int(sum(part.forest_idx.shape[0] for part in parts))
        if draws is None:
            idx = np.arange(total, dtype=np.int64)
        else:
            idx = np.asarray(draws, dtype=np.int64).ravel()
            if idx.size and (idx.min() < 0 or idx.max() >= total):
                raise ValueError(f"draws must index the {total} stored draws")
        if idx.size < 1:
            raise ValueError("no draws to replicate")
        self.D = D = int(idx.size)
        self.params = _param_matrix(likelihood, points, D)
        _check_domain(self.family, self.params)
        seed = int(random_seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"random_seed must be an integer in [0, 2^64), got {random_seed!r}")
        self.seed = seed
        from .trees import pooled_history

        cached = getattr(sampler, "pooled_history", None)  # (the multi-chain sampler keeps it)
        self.pool, table = cached() if cached is not None else pooled_history(parts)
        self.fidx = np.ascontiguousarray(np.asarray(table)[idx], dtype=np.int32)
        self.backend = parts[0]._get_backend if hasattr(parts[0], "_get_backend") else None

    def run(self, mode: str, q=None, hdi_k: int = 0):
        """``mode``: "matrix" -> y_rep (D, n); "summary" -> pgb_row_summary's rows (2 + Q + 2, n); "pit" -> the counts
        (2, n).  Each with (n_capped, n_exhausted)."""
        from .sampler import default_backend

        be = self.backend() if self.backend is not None else default_backend()
        lib, mem = be.lib, be.mem
        if lib.backend_name != "hip-gfx950":
            raise _abi.PGBError(f"posterior predictive draws run on the HIP backend only, not on {lib.backend_name}")
        call = lib.ppc_entry_point()
        n, D, K, p = self.n, self.D, self.K, self.p
        Q = 0 if q is None else q.size
        per_row = 8 * (p + K * (D + 1) + (D if K > 1 and mode != "pit" else 0) + (2 + Q + 2 if mode == "summary" else 0) + 2)
        block = max(64, min(n, _block_bytes() // per_row // 64 * 64))
        out = {"matrix": np.empty((D, n)), "summary": np.empty((2 + Q + 2, n)), "pit": np.empty((2, n), np.int64)}[mode]
        lik = _abi.PpcLik()
        lik.family = _abi.FAMILIES[self.family]
        lik.n_params = self.n_par
        lik.params_host = self.params.ctypes.data if self.n_par else None
        carr = self.pool.as_c()
        excl = self.excluded
        flags = (C.c_int64 * 2)()
        capped = exhausted = 0
        for r0 in range(0, n, block):
            r1 = min(n, r0 + block)
            nb = r1 - r0
            xd = mem.from_host(self.X[r0:r1])
            od = None if self.offset is None else mem.from_host(np.ascontiguousarray(self.offset[:, r0:r1]))
            lik.offset_dev = None if od is None else mem.ptr(od)
            md = mem.empty((D * K * nb,), np.float64)  # [D][K][nb]
            rc = lib.lib.pgb_predict(C.byref(carr), self.fidx.ctypes.data, D, self.m, mem.ptr(xd), nb, p, p,
                                     excl.ctypes.data if excl.size else None, int(excl.size), mem.ptr(md), mem.stream_ptr)
            lib.check(rc, "pgb_predict")
            yd = pd = rd = None
            if mode == "pit":
                yd = mem.from_host(self.y[r0:r1])
                pd = mem.from_host(np.zeros(2 * nb, np.int32))
            else:
                rd = md if K == 1 else mem.empty((D * nb,), np.float64)  # (K = 1: in place)
            rc = call(mem.ptr(md), D, K, nb, nb, r0, C.byref(lik), self.seed, None if rd is None else mem.ptr(rd), nb,
                      None if yd is None else mem.ptr(yd), None if pd is None else mem.ptr(pd), flags, mem.stream_ptr)
            lib.check(rc, "pgb_ppc_draw")
            capped += int(flags[0])
            exhausted += int(flags[1])
            if mode == "matrix":
                out[:, r0:r1] = mem.to_host(rd).reshape(D, nb)
            elif mode == "summary":
                out[:, r0:r1] = _summary_block(lib, mem, rd, D, nb, nb, None, 0, q, hdi_k)
            else:
                out[:, r0:r1] = mem.to_host(pd).reshape(2, nb)
        return out, {"n_capped": capped, "n_exhausted": exhausted}


def posterior_predictive(sampler, X, likelihood, points=None, offset=None, draws=None, excluded=None, random_seed=0,
                         return_info: bool = False):
    """Replicated observations ``y_rep[d, i] ~ p(y | mu_d(X[i]) + offset[., i], params[d])`` for every stored draw
    ``d`` (or those ``draws`` indexes) and every row of ``X``: an array ``(D, n_rows)`` (the class for the categorical
    family, 0 / 1 for the Bernoulli families).

    ``sampler``, ``likelihood``, ``points``, ``offset``: as :func:`~pymc_bart_amd.pointwise_log_likelihood` takes them
    (the compiled and callback families have no sampler and are refused).  ``excluded``: covariates marginalised out
    by the trees' own counts, as in ``sample_posterior``.  ``random_seed``: a value is a function of the seed, the
    POSITION of the draw in ``draws`` and the row index alone -- the same call gives the same array, whatever
    ``PGB_PW_BLOCK_BYTES`` says.  ``return_info``: also return ``{"n_capped", "n_exhausted"}``, the (draw, row) pairs
    whose value met a cap or whose rejection sampler ran out of attempts (``include/pgbart_ppc.h``)."""
    job = _Job(sampler, X, likelihood, points, offset, draws, excluded, random_seed)
    out, info = job.run("matrix")
    return (out, info) if return_info else out


def predictive_summary(sampler, X, likelihood, points=None, offset=None, draws=None, excluded=None, random_seed=0,
                       quantiles=DEFAULT_QUANTILES, hdi_prob=DEFAULT_HDI_PROB) -> dict:
    """:func:`~pymc_bart_amd.summarize_matrix`'s dict (arrays ``(n_rows,)``, ``quantiles`` ``(Q, n_rows)``, ``hdi``
    ``(2, n_rows)``) of :func:`posterior_predictive`'s matrix, computed on the device without it -- the predictive
    band of the observations, not the band of the mean function -- plus ``n_capped`` and ``n_exhausted``.  Between 2
    and 16384 draws."""
    job = _Job(sampler, X, likelihood, points, offset, draws, excluded, random_seed)
    q, hdi_k, _ = _spec(job.D, quantiles, hdi_prob, "identity")
    stats, info = job.run("summary", q, hdi_k)
    res = _result(stats, job.n, 1, q, hdi_prob, hdi_k, job.D)
    for key in ("mean", "sd", "var", "quantiles", "hdi"):
        if res[key] is not None:
            res[key] = res[key][..., 0]
    res.update(info)
    return res


def predictive_pit(sampler, X, y, likelihood, points=None, offset=None, draws=None, excluded=None, random_seed=0) -> dict:
    """The probability integral transform of the observed ``y`` under the posterior predictive, by counting:
    ``pit[i] = (n_below[i] + n_equal[i] / 2) / D`` with ``n_below`` / ``n_equal`` the draws whose replicated
    observation of row ``i`` is below / equal to ``y[i]`` (the mid-p form: uniform for a calibrated model, discrete
    families included; its mean is the Bayesian p-value of ``y``).  Also ``n_draws``, ``n_capped``, ``n_exhausted``.
    Nothing of size ``draws x rows`` is written anywhere."""
    job = _Job(sampler, X, likelihood, points, offset, draws, excluded, random_seed, y=y, pit=True)
    counts, info = job.run("pit")
    below, equal = counts[0].copy(), counts[1].copy()
    res = {"pit": (below + 0.5 * equal) / job.D, "n_below": below, "n_equal": equal, "n_draws": job.D}
    res.update(info)
    return res
