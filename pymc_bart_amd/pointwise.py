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

import numpy as np

from . import _abi
from ._stored import MAX_OFFSET, Job, check_y, fill_lik  # noqa: F401  (MAX_OFFSET: a constant of this module too)
from ._stored import chains as _chains  # noqa: F401  (the name tests/test_ppc_gpu.py has always imported from here)

#: params per draw of the built-in families (``pgb_logpdf_nparams``) and the outputs they take (0: any K >= 2)
FAMILY_PARAMS = {"normal": 1, "bernoulli_probit": 0, "bernoulli_logit": 0, "categorical": 0, "normal_meanscale": 0,
                 "poisson_log": 0, "negbin_log": 1, "asymmetric_laplace": 2, "student_t": 2, "gamma_log": 1}
FAMILY_OUTPUTS = {"categorical": 0, "normal_meanscale": 2}
CHUNK = 32          # PGB_PW_CHUNK (include/pgbart_logpdf.h)


def check_outputs(likelihood, family, K: int, want: int) -> None:
    """The likelihood's outputs against the trees' ``K`` and against what the family takes (``want``; 0: any K >= 2)."""
    lk = int(getattr(likelihood, "n_outputs", 1))
    if lk != K:
        raise ValueError(f"the likelihood has n_outputs = {lk}, the sampler's trees n_outputs = {K}")
    if (want > 0 and K != want) or (want == 0 and K < 2):
        raise ValueError(f"the {family} family does not take n_outputs = {K}")


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


def param_matrix(likelihood, points, D: int) -> np.ndarray:
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


def check_aux(likelihood, n: int):
    """The aux column of a compiled likelihood against the ``n`` rows of ``X`` (``None`` without one)."""
    aux = getattr(likelihood, "aux", None)
    if aux is None:
        return None
    if aux.size != n:
        raise ValueError(f"the compiled likelihood's aux must hold one value per row ({n}), got {aux.size}")
    return np.ascontiguousarray(aux, np.float64)


def take_code(lik, build):
    """Hand a build's code object to the call's ``lik`` record (``code_object``, ``code_bytes``) -> the ctypes buffer
    that holds the bytes: the caller keeps it for as long as ``lik`` is used."""
    code = C.create_string_buffer(build.code, len(build.code))
    lik.code_object, lik.code_bytes = C.cast(code, C.c_void_p), len(build.code)
    return code


class ScoringJob(Job):
    """One scoring call: the job base plus the family, ``y``, the compiled body's ``aux`` and the params per draw."""

    def __init__(self, sampler, X, y, likelihood, points, offset, draws):
        super().__init__(sampler)
        K = self.K
        self.family = getattr(likelihood, "family", None)
        self.n_par = _n_params(likelihood)  # (refuses the callback family)
        check_outputs(likelihood, self.family, K, FAMILY_OUTPUTS.get(self.family, 1) if self.family != "compiled" else K)
        self.take_X(X)
        self.y = check_y(y, self.n)
        self.take_offset(offset)
        self.aux = check_aux(likelihood, self.n) if self.family == "compiled" else None
        self.take_draws(draws, "no draws to score")
        self.params = param_matrix(likelihood, points, self.D)
        self.take_history()
        self.likelihood = likelihood

    def run(self, matrix: bool, summary: bool, on_block=None, scratch: int = 2):
        """-> (matrix (D, n) or None, row_stats (3, n) or None, n_clamped).  ``on_block(be, blk)``: called with every
        block's matrix still on the device (``blk.md``: ``[D][nb]``, rows ``blk.r0 .. blk.r1``, next to the block's
        device copies of X, y and the offset) in place of its copy to the host -- nothing of size draws x rows then
        leaves the device (:mod:`pymc_bart_amd.loo`).  ``scratch``: the doubles per row the hook allocates on the
        device, counted into the block size."""
        be = self.hip_backend("pointwise log-likelihoods run")
        lib, mem = be.lib, be.mem
        call = lib.pointwise_entry_point()
        n, D, K, p = self.n, self.D, self.K, self.p
        lik = fill_lik(_abi.PointwiseLik(), self)
        code = take_code(lik, self.likelihood.compiled(pointwise=True)) if self.family == "compiled" else None
        per_row = 8 * (p + 2 + K + (D if matrix else 0) + (4 * (-(-D // CHUNK)) + 3 if summary else 0)
                       + (int(scratch) if on_block is not None else 0))
        out = np.empty((D, n)) if matrix and on_block is None else None
        stats = np.empty((3, n)) if summary else None
        carr = self.pool.as_c()
        clamped = 0
        for blk in self.blocks(be, per_row, y=True):
            r0, r1, nb = blk.r0, blk.r1, blk.nb
            ad = None if self.aux is None else mem.from_host(self.aux[r0:r1])
            lik.y_dev = mem.ptr(blk.yd)
            lik.offset_dev = None if blk.od is None else mem.ptr(blk.od)
            lik.aux_dev = None if ad is None else mem.ptr(ad)
            md = blk.md = mem.empty((D * nb,), np.float64) if matrix else None
            sd = mem.empty((3 * nb,), np.float64) if summary else None
            nc = C.c_int64(0)
            rc = call(C.byref(carr), self.fidx.ctypes.data, D, self.m, mem.ptr(blk.xd), nb, p, p, C.byref(lik),
                      None if md is None else mem.ptr(md), None if sd is None else mem.ptr(sd), C.byref(nc),
                      mem.stream_ptr)
            lib.check(rc, "pgb_pointwise_loglik")
            clamped += int(nc.value)
            if on_block is not None:
                on_block(be, blk)
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
    job = ScoringJob(sampler, X, y, likelihood, points, offset, draws)
    out, _, clamped = job.run(matrix=True, summary=False)
    return (out, clamped) if return_clamped else out


def log_predictive_density(sampler, X, y, likelihood, points=None, offset=None, draws=None) -> dict:
    """The row-wise reduction of :func:`pointwise_log_likelihood` over the draws, computed on the device without the
    matrix: ``lppd_i = log mean_d exp(ll[d, i])``, ``p_waic_i = var_d ll[d, i]`` (ddof 1), ``mean_i``; and on the
    host their sums ``lppd``, ``elpd_waic = sum(lppd_i - p_waic_i)``, ``se_elpd_waic = sqrt(n var(lppd_i - p_waic_i))``,
    with ``n_draws`` and ``n_clamped``."""
    job = ScoringJob(sampler, X, y, likelihood, points, offset, draws)
    _, stats, clamped = job.run(matrix=False, summary=True)
    lppd_i, mean_i, p_waic_i = stats[0].copy(), stats[1].copy(), stats[2].copy()
    elpd_i = lppd_i - p_waic_i
    n = lppd_i.size
    return {"lppd_i": lppd_i, "p_waic_i": p_waic_i, "mean_i": mean_i, "lppd": float(lppd_i.sum()),
            "elpd_waic": float(elpd_i.sum()), "se_elpd_waic": float(np.sqrt(n * elpd_i.var())) if n > 1 else 0.0,
            "n_draws": job.D, "n_clamped": clamped}
