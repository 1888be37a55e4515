"""Scoring a fit: the pointwise log-likelihood of posterior draws, lppd and WAIC (``include/pgbart_pointwise.h``).

Under PyMC these numbers come from the model's own ``logp``.  Here the likelihood lives inside the library -- ten
closed families written relative to a saturated model (right for particle weights, wrong for comparing two models)
or a C body compiled at run time -- so the library evaluates it itself: the FULL, normalised log density
(``include/pgbart_logpdf.h``) of ``y[i]`` under draw ``d``, inside the tree walk that predicts ``mu_d(X[i])``.

* :func:`pointwise_log_likelihood` returns the ``(D, n_rows)`` matrix (what ArviZ's ``loo`` / ``waic`` take).
* :func:`log_predictive_density` returns the row-wise reduction over draws -- ``lppd_i`` (log mean exp),
  ``p_waic_i`` (the variance over draws) -- and their sums.  On the device this is summary mode: nothing of size
  ``draws x rows`` is written anywhere.

Values are clamped to [-2047, 2047] (NaN -> -2047), what the sampler itself can represent; every clamped (draw, row)
pair is counted (``n_clamped``).  HIP backend only; the callback family has no device density.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi

#: params per draw of the built-in families (``pgb_logpdf_nparams``) and the outputs they take (0: any K >= 2)
FAMILY_PARAMS = {"normal": 1, "bernoulli_probit": 0, "bernoulli_logit": 0, "categorical": 0, "normal_meanscale": 0,
                 "poisson_log": 0, "negbin_log": 1, "asymmetric_laplace": 2, "student_t": 2, "gamma_log": 1}
FAMILY_OUTPUTS = {"categorical": 0, "normal_meanscale": 2}
MAX_OFFSET = 1.0e6  # PGB_MAX_OFFSET
CHUNK = 32          # PGB_PW_CHUNK (include/pgbart_logpdf.h)


def _block_bytes() -> int:
    """Device bytes one block of rows may take (its matrix, or its rows of X): ``PGB_PW_BLOCK_BYTES``, default 1 GiB."""
    return max(1 << 16, int(os.environ.get("PGB_PW_BLOCK_BYTES", 1 << 30)))


def _chains(sampler) -> list:
    parts = getattr(sampler, "_chain_samplers", None)
    parts = list(parts) if parts is not None else [sampler]
    for part in parts:
        if not all(hasattr(part, a) for a in ("pool", "forest_idx", "m")):
            raise TypeError("sampler must be what _get_posterior_sampler(op) or PosteriorSampler.from_history returns")
    return parts


def _n_params(likelihood) -> int:
    family = getattr(likelihood, "family", None)
    if family == "callback":
        raise ValueError("the callback family is evaluated by a host function: it has no device density to score "
                         "(write the likelihood as a CompiledLikelihood body)")
    if family == "compiled":
        return len(likelihood.param_names)
    if family not in FAMILY_PARAMS:
        raise ValueError(f"unknown likelihood family {family!r}")
    return FAMILY_PARAMS[family]


def _param_matrix(likelihood, points, D: int) -> np.ndarray:
    """``[D][n_params]`` through the likelihood's own ``params(point)``."""
    n_par = _n_params(likelihood)
    if points is None or (isinstance(points, dict) and all(np.ndim(v) == 0 for v in points.values())):
        rows = [likelihood.params(points)] * D  # fixed numbers / scalars: the same for every draw
    elif isinstance(points, dict):
        cols = {}
        for k, v in points.items():
            a = np.asarray(v)
            if a.ndim == 0:
                cols[k] = None
            elif a.ndim == 1 and a.shape[0] == D:
                cols[k] = a
            else:
                raise ValueError(f"points[{k!r}] must be a scalar or hold one value per draw ({D}), got shape {a.shape}")
        rows = [likelihood.params({k: (points[k] if a is None else a[d]) for k, a in cols.items()}) for d in range(D)]
    else:
        pts = list(points)
        if len(pts) != D:
            raise ValueError(f"points must hold one point per draw ({D}), got {len(pts)}")
        rows = [likelihood.params(pt) for pt in pts]
    out = np.zeros((D, max(n_par, 1)), np.float64)
    for d, r in enumerate(rows):
        r = np.asarray(r, np.float64).ravel()
        if r.size != n_par:
            raise ValueError(f"the {likelihood.family} likelihood takes {n_par} params per draw, its params() gave {r.size}")
        out[d, :n_par] = r
    if not np.all(np.isfinite(out)):
        raise ValueError("likelihood params must be finite")
    return np.ascontiguousarray(out[:, :n_par])


class _Job:
    """Everything of one call, validated on the host before a backend is touched."""

    def __init__(self, sampler, X, y, likelihood, points, offset, draws):
        parts = _chains(sampler)
        self.K = K = int(parts[0].n_outputs)
        self.m = int(parts[0].m)
        self.family = getattr(likelihood, "family", None)
        self.n_par = _n_params(likelihood)  # (refuses the callback family)
        lk = int(getattr(likelihood, "n_outputs", 1))
        if lk != K:
            raise ValueError(f"the likelihood has n_outputs = {lk}, the sampler's trees n_outputs = {K}")
        want = FAMILY_OUTPUTS.get(self.family, 1) if self.family != "compiled" else K
        if (want > 0 and K != want) or (want == 0 and K < 2):
            raise ValueError(f"the {self.family} family does not take n_outputs = {K}")
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError(f"X must be a matrix (n_rows, p), got shape {X.shape}")
        self.X = np.ascontiguousarray(X)
        n = self.n = int(X.shape[0])
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
        self.aux = None
        if self.family == "compiled" and likelihood.aux is not None:
            if likelihood.aux.size != n:
                raise ValueError(f"the compiled likelihood's aux must hold one value per row ({n}), got {likelihood.aux.size}")
            self.aux = np.ascontiguousarray(likelihood.aux, np.float64)
        # several chains: one pool, one call
        starts = np.concatenate([[0], np.cumsum([part.forest_idx.shape[0] for part in parts])]).astype(np.int64)
        total = int(starts[-1])
        if draws is None:
            idx = np.arange(total, dtype=np.int64)
        else:
            idx = np.asarray(draws, dtype=np.int64).ravel()
            if idx.size and (idx.min() < 0 or idx.max() >= total):
                raise ValueError(f"draws must index the {total} stored draws")
        if idx.size < 1:
            raise ValueError("no draws to score")
        self.D = D = int(idx.size)
        self.params = _param_matrix(likelihood, points, D)
        from .trees import pooled_history

        cached = getattr(sampler, "pooled_history", None)  # (the multi-chain sampler keeps it)
        self.pool, table = cached() if cached is not None else pooled_history(parts)
        self.fidx = np.ascontiguousarray(np.asarray(table)[idx], dtype=np.int32)
        self.likelihood = likelihood
        self.backend = parts[0]._get_backend if hasattr(parts[0], "_get_backend") else None
        self.block = None  # (run: the current block's device copies of X, y and the offset, for on_block)

    def run(self, matrix: bool, summary: bool, on_block=None, scratch: int = 2):
        """-> (matrix (D, n) or None, row_stats (3, n) or None, n_clamped).  ``on_block(lib, mem, md, nb, r0)``: called
        with every block's matrix still on the device (``md``: ``[D][nb]``, rows ``r0 .. r0 + nb``) in place of its
        copy to the host -- nothing of size draws x rows then leaves the device (:mod:`pymc_bart_amd.loo`).  During
        the call ``self.block`` holds the block's device copies ``(X, y, offset or None)``; ``scratch``: the doubles
        per row the hook allocates on the device, counted into the block size."""
        from .sampler import default_backend

        be = self.backend() if self.backend is not None else default_backend()
        lib, mem = be.lib, be.mem
        if lib.backend_name != "hip-gfx950":
            raise _abi.PGBError(f"pointwise log-likelihoods run on the HIP backend only, not on {lib.backend_name}")
        call = lib.pointwise_entry_point()
        n, D, K, p = self.n, self.D, self.K, int(self.X.shape[1])
        lik = _abi.PointwiseLik()
        lik.family = _abi.FAMILIES[self.family]
        lik.n_params = self.n_par
        lik.params_host = self.params.ctypes.data if self.n_par else None
        code = None
        if self.family == "compiled":
            build = self.likelihood.compiled(pointwise=True)
            code = C.create_string_buffer(build.code, len(build.code))
            lik.code_object, lik.code_bytes = C.cast(code, C.c_void_p), len(build.code)
        per_row = 8 * (p + 2 + K + (D if matrix else 0) + (4 * (-(-D // CHUNK)) + 3 if summary else 0)
                       + (int(scratch) if on_block is not None else 0))
        block = max(64, min(n, _block_bytes() // per_row // 64 * 64))
        out = np.empty((D, n)) if matrix and on_block is None else None
        stats = np.empty((3, n)) if summary else None
        carr = self.pool.as_c()
        clamped = 0
        for r0 in range(0, n, block):
            r1 = min(n, r0 + block)
            nb = r1 - r0
            xd = mem.from_host(self.X[r0:r1])
            yd = mem.from_host(self.y[r0:r1])
            od = None if self.offset is None else mem.from_host(np.ascontiguousarray(self.offset[:, r0:r1]))
            ad = None if self.aux is None else mem.from_host(self.aux[r0:r1])
            lik.y_dev = mem.ptr(yd)
            lik.offset_dev = None if od is None else mem.ptr(od)
            lik.aux_dev = None if ad is None else mem.ptr(ad)
            md = mem.empty((D * nb,), np.float64) if matrix else None
            sd = mem.empty((3 * nb,), np.float64) if summary else None
            nc = C.c_int64(0)
            rc = call(C.byref(carr), self.fidx.ctypes.data, D, self.m, mem.ptr(xd), nb, p, p, C.byref(lik),
                      None if md is None else mem.ptr(md), None if sd is None else mem.ptr(sd), C.byref(nc),
                      mem.stream_ptr)
            lib.check(rc, "pgb_pointwise_loglik")
            clamped += int(nc.value)
            if on_block is not None:
                self.block = (xd, yd, od)
                on_block(lib, mem, md, nb, r0)
                self.block = None
            elif matrix:
                out[:, r0:r1] = mem.to_host(md).reshape(D, nb)
            if summary:
                stats[:, r0:r1] = mem.to_host(sd).reshape(3, nb)
        del code
        return out, stats, clamped


def pointwise_log_likelihood(sampler, X, y, likelihood, points=None, offset=None, draws=None,
                             return_clamped: bool = False):
    """``log p(y[i] | draw d)`` for every stored draw ``d`` (or those ``draws`` indexes) and every row of ``X``:
    an array ``(D, n_rows)``.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns (several chains are
    scored as one pool, in chain order).  ``likelihood``: any likelihood object of :mod:`pymc_bart_amd.pgbart` except
    the callback family, or a :class:`~pymc_bart_amd.CompiledLikelihood` (its ``aux`` column then belongs to the rows
    of ``X``).  ``points``: the likelihood's parameters per draw -- a list of D dicts, a dict of length-D arrays, or
    scalars -- read through the likelihood's own ``params(point)``; ``{"sigma": res["sigma"]}`` from ``sample_chain``
    works as is.  ``offset``: ``(K, n_rows)`` added to the predictors.  Rows are processed in blocks when the matrix
    would not fit the device (``PGB_PW_BLOCK_BYTES``).  ``return_clamped``: also return the number of clamped pairs."""
    job = _Job(sampler, X, y, likelihood, points, offset, draws)
    out, _, clamped = job.run(matrix=True, summary=False)
    return (out, clamped) if return_clamped else out


def log_predictive_density(sampler, X, y, likelihood, points=None, offset=None, draws=None) -> dict:
    """The row-wise reduction of :func:`pointwise_log_likelihood` over the draws, computed on the device without the
    matrix: ``lppd_i = log mean_d exp(ll[d, i])``, ``p_waic_i = var_d ll[d, i]`` (ddof 1), ``mean_i``; and on the
    host their sums ``lppd``, ``elpd_waic = sum(lppd_i - p_waic_i)``, ``se_elpd_waic = sqrt(n var(lppd_i - p_waic_i))``,
    with ``n_draws`` and ``n_clamped``."""
    job = _Job(sampler, X, y, likelihood, points, offset, draws)
    _, stats, clamped = job.run(matrix=False, summary=True)
    lppd_i, mean_i, p_waic_i = stats[0].copy(), stats[1].copy(), stats[2].copy()
    elpd_i = lppd_i - p_waic_i
    n = lppd_i.size
    return {"lppd_i": lppd_i, "p_waic_i": p_waic_i, "mean_i": mean_i, "lppd": float(lppd_i.sum()),
            "elpd_waic": float(elpd_i.sum()), "se_elpd_waic": float(np.sqrt(n * elpd_i.var())) if n > 1 else 0.0,
            "n_draws": job.D, "n_clamped": clamped}
