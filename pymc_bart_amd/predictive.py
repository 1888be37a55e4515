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

The ten built-in families have a sampler, and so has a :class:`~pymc_bart_amd.CompiledLikelihood` with a sampler body
(``sampler=``: ``pgb_ppc_draw_compiled`` runs it, ``k_ppc_compiled``); a compiled likelihood without a sampler body, and
the callback family, have a log density only and are refused.
Rejection samplers are bounded: pairs that exhausted their attempts (``n_exhausted``) or met a cap (``n_capped``: a
Poisson rate above 2^30, a non-finite value) are counted, never silent.  HIP backend only.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._stored import Job, check_seed, check_y, drop_k_axis, fill_lik
from .pointwise import FAMILY_OUTPUTS, FAMILY_PARAMS, check_aux, check_outputs, param_matrix, take_code
from .summary import DEFAULT_HDI_PROB, DEFAULT_QUANTILES, result, spec, summary_block


def check_family(likelihood) -> str:
    family = getattr(likelihood, "family", None)
    if family == "compiled" and getattr(likelihood, "sampler", None) is not None:
        return family
    if family in ("callback", "compiled"):
        raise ValueError(f"the {family} family has a log density only, no sampler: posterior predictive draws take the "
                         f"built-in families ({', '.join(FAMILY_PARAMS)})")
    if family not in FAMILY_PARAMS:
        raise ValueError(f"unknown likelihood family {family!r}")
    return family


def check_domain(family: str, params: np.ndarray) -> None:
    """pgb_logpdf_prepare's domain: every param positive (and finite: ``param_matrix``), 0 < q < 1."""
    bad = ~np.all(params > 0.0, axis=1)
    if family == "asymmetric_laplace":
        bad |= ~(params[:, 1] < 1.0)
    if np.any(bad):
        d = int(np.flatnonzero(bad)[0])
        raise ValueError(f"the params of draw {d} are outside the {family} family's domain (positive and finite; "
                         f"0 < q < 1): {params[d].tolist()}")


class Replicator:
    """The replicating call of one job -- ``pgb_ppc_draw`` of a built-in family or ``pgb_ppc_draw_compiled`` of a
    compiled likelihood's sampler body -- for a block of rows, and the flag counts summed over the blocks.  ``job``
    gives ``family``, ``n_par``, ``params``, ``D``, ``K`` and, for the compiled family, ``likelihood`` and ``aux``."""

    def __init__(self, lib, job, seed: int):
        self.job, self.seed = job, seed
        self.compiled = job.family == "compiled"
        if self.compiled:
            build = job.likelihood.compiled_sampler()
            self.lik = lik = _abi.PpcCode()
            self._code = take_code(lik, build)
            lik.n_params = job.n_par
            lik.params_host = job.params.ctypes.data if job.n_par else None
            self.call, self.name = lib.ppc_compiled_entry_point(), "pgb_ppc_draw_compiled"
        else:
            self.lik = fill_lik(_abi.PpcLik(), job)
            self.call, self.name = lib.ppc_entry_point(), "pgb_ppc_draw"
        self.flags = (C.c_int64 * 2)()
        self.capped = self.exhausted = 0

    def __call__(self, be, gd, nb: int, r0: int, od=None, rd=None, yd=None, pd=None):
        """``gd`` ``[D][K][nb]`` (the predictors of rows ``r0 ..``) -> ``rd`` ``[D][nb]`` (or ``None``) and the PIT
        counts ``pd`` against ``yd`` (or ``None``)."""
        lib, mem, job = be.lib, be.mem, self.job
        self.lik.offset_dev = None if od is None else mem.ptr(od)
        ad = None
        if self.compiled:
            ad = None if job.aux is None else mem.from_host(job.aux[r0:r0 + nb])
            self.lik.aux_dev = None if ad is None else mem.ptr(ad)
        rc = self.call(mem.ptr(gd), job.D, job.K, nb, nb, r0, C.byref(self.lik), self.seed,
                       None if rd is None else mem.ptr(rd), nb, None if yd is None else mem.ptr(yd),
                       None if pd is None else mem.ptr(pd), self.flags, mem.stream_ptr)
        lib.check(rc, self.name)
        del ad
        self.capped += int(self.flags[0])
        self.exhausted += int(self.flags[1])

    @property
    def info(self) -> dict:
        return {"n_capped": self.capped, "n_exhausted": self.exhausted}


class _Job(Job):
    """One replicating call: the job base plus the family, its params in their domain (a sampler body's: finite), the
    body's ``aux``, the seed and ``y`` for the PIT."""

    def __init__(self, sampler, X, likelihood, points, offset, draws, excluded, random_seed, y=None, pit=False):
        super().__init__(sampler)
        self.family = check_family(likelihood)
        self.likelihood = likelihood
        compiled = self.family == "compiled"
        self.n_par = len(likelihood.param_names) if compiled else FAMILY_PARAMS[self.family]
        check_outputs(likelihood, self.family, self.K, self.K if compiled else FAMILY_OUTPUTS.get(self.family, 1))
        self.take_X(X)
        self.y = check_y(y, self.n) if pit else None
        self.take_offset(offset)
        self.aux = check_aux(likelihood, self.n) if compiled else None
        self.take_excluded(excluded)
        self.take_draws(draws, "no draws to replicate")
        self.params = param_matrix(likelihood, points, self.D)
        if not compiled:  # (a sampler body owns its domain)
            check_domain(self.family, self.params)
        self.seed = check_seed(random_seed)
        self.take_history()

    def run(self, mode: str, q=None, hdi_k: int = 0):
        """``mode``: "matrix" -> y_rep (D, n); "summary" -> pgb_row_summary's rows (2 + Q + 2, n); "pit" -> the counts
        (2, n).  Each with (n_capped, n_exhausted)."""
        be = self.hip_backend("posterior predictive draws run")
        lib, mem = be.lib, be.mem
        replicate = Replicator(lib, self, self.seed)
        n, D, K, p = self.n, self.D, self.K, self.p
        Q = 0 if q is None else q.size
        per_row = 8 * (p + K * (D + 1) + (D if K > 1 and mode != "pit" else 0) + (2 + Q + 2 if mode == "summary" else 0) + 2
                       + (1 if self.aux is not None else 0))
        out = {"matrix": np.empty((D, n)), "summary": np.empty((2 + Q + 2, n)), "pit": np.empty((2, n), np.int64)}[mode]
        for blk in self.blocks(be, per_row, predict=True):
            r0, r1, nb, md = blk.r0, blk.r1, blk.nb, blk.md
            yd = pd = rd = None
            if mode == "pit":
                yd = mem.from_host(self.y[r0:r1])
                pd = mem.from_host(np.zeros(2 * nb, np.int32))
            else:
                rd = md if K == 1 else mem.empty((D * nb,), np.float64)  # (K = 1: in place)
            replicate(be, md, nb, r0, blk.od, rd, yd, pd)
            if mode == "matrix":
                out[:, r0:r1] = mem.to_host(rd).reshape(D, nb)
            elif mode == "summary":
                out[:, r0:r1] = summary_block(lib, mem, rd, D, nb, nb, None, 0, q, hdi_k)
            else:
                out[:, r0:r1] = mem.to_host(pd).reshape(2, nb)
        return out, replicate.info


def posterior_predictive(sampler, X, likelihood, points=None, offset=None, draws=None, excluded=None, random_seed=0,
                         return_info: bool = False):
    """Replicated observations ``y_rep[d, i] ~ p(y | mu_d(X[i]) + offset[., i], params[d])`` for every stored draw
    ``d`` (or those ``draws`` indexes) and every row of ``X``: an array ``(D, n_rows)`` (the class for the categorical
    family, 0 / 1 for the Bernoulli families).

    ``sampler``, ``likelihood``, ``points``, ``offset``: as :func:`~pymc_bart_amd.pointwise_log_likelihood` takes them
    (a compiled likelihood without a sampler body, and the callback family, have no sampler and are refused; a
    compiled likelihood's ``aux`` column belongs to the rows of ``X``).  ``excluded``: covariates marginalised out
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
    q, hdi_k, _ = spec(job.D, quantiles, hdi_prob, "identity")
    stats, info = job.run("summary", q, hdi_k)
    res = drop_k_axis(result(stats, job.n, 1, q, hdi_prob, hdi_k, job.D))
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
