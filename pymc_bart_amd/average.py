"""Reading a fit the other way: per-draw averages over rows on the device (``pgb_row_reduce``,
``include/pgbart_rowreduce.h``).

Every other consumer of the stored draws reduces over the draws, per row.  Average and conditional average treatment
effects, poststratified and marginal means, and the per-draw goodness of fit reduce over the ROWS, per draw -- so each
comes with a posterior.  Per block of rows one ``pgb_predict`` call (two for a contrast) writes the predictions of all
draws into device scratch and one ``pgb_row_reduce`` call adds the block to the partial sums of every (draw, output,
group), which stay on the device; ``pgb_row_reduce_finish`` turns them into the results.  Nothing of size draws x rows
leaves the device.

* :func:`average_prediction` -- weighted group means of ``T(f(x_i) + offset)`` per draw.
* :func:`average_contrast` -- the same of ``T(f(x_a,i)) - T(f(x_b,i))`` (toggle the treatment column: the ATE, and by
  subgroup the CATE), optionally with the per-row summaries of the contrast.
* :func:`bayes_r2` -- Bayesian R-squared (Gelman et al. 2019, the residual form), MSE, RMSE and bias per draw.

HIP backend only.  The sums have a fixed order (64 partials by row index mod 64, carried from block to block), so the
results depend neither on the blocking nor on the launch geometry.  Rows whose groups are contiguous are the fast case:
a lane of the kernel exchanges its partial sums with the workspace whenever its group changes, so groups interleaved
row by row are as correct and slower (sort the rows by group first where that matters).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._stored import PW_BLOCK, Job, block_bytes, check_offset, check_X, check_y
from .summary import DEFAULT_HDI_PROB, DEFAULT_QUANTILES, TRANSFORMS, result, spec, summary_block

MAX_GROUPS = 4096  # PGB_ROWRED_MAX_GROUPS (include/pgbart_rowreduce.h)
LANES = 64         # PGB_ROWRED_LANES


def workspace_bytes(D: int, K: int, G: int, has_y: bool) -> int:
    """The bytes of the partial sums of one call (``pgb_row_reduce_workspace_bytes``): 64 partials of 2 (with ``y`` 4)
    sums per (draw, output, group), 64 of the weight per group, two counters."""
    return 8 * (D * K * G * (4 if has_y else 2) * LANES + G * LANES + 2)


def check_weights(weights, n: int) -> np.ndarray:
    if weights is None:
        return np.ones(n)
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != (n,):
        raise ValueError(f"weights must hold one value per row of X: shape ({n},), got {w.shape}")
    if not np.all(np.isfinite(w)) or np.any(w < 0.0):
        raise ValueError("weights must be finite and >= 0")
    return np.ascontiguousarray(w)


def check_groups(groups, n: int, weights: np.ndarray) -> tuple:
    """-> (labels ``(G,)``, the group index of every row as int32, rows per group); ``None``: one group, label 0."""
    if groups is None:
        labels, gid = np.zeros(1, np.int64), np.zeros(n, np.int64)
    else:
        groups = np.asarray(groups)
        if groups.shape != (n,):
            raise ValueError(f"groups must hold one label per row of X: shape ({n},), got {groups.shape}")
        if groups.dtype.kind in "fc" and np.any(np.isnan(groups)):
            raise ValueError("groups must not hold NaN labels")
        try:
            labels, gid = np.unique(groups, return_inverse=True)
        except TypeError:
            raise ValueError(f"groups must hold labels that can be ordered, got dtype {groups.dtype} with mixed kinds") from None
    if labels.size > MAX_GROUPS:
        raise ValueError(f"at most {MAX_GROUPS} groups per call, got {labels.size}")
    total = np.bincount(gid, weights=weights, minlength=labels.size)
    if np.any(total == 0.0):
        raise ValueError(f"group {labels[int(np.argmin(total != 0.0))].item()!r} has total weight 0")
    return labels, np.ascontiguousarray(gid, dtype=np.int32), np.bincount(gid, minlength=labels.size)


class AverageJob(Job):
    """One call of this module: the job base plus the second arm, the weights, the groups, ``y`` and the centres.  The
    arguments are taken in this order: ``X`` (``X_a``), ``X_b``, the transform, the offsets, ``excluded``, the draws,
    the weights, the groups, ``y``, the summary spec of ``rows``, the size of the partial sums, the history."""

    def __init__(self, sampler, X, X_b=None, weights=None, groups=None, draws=None, transform="identity", offset=None,
                 offset_b=None, excluded=None, y=None, rows=False, quantiles=None, hdi_prob=None):
        super().__init__(sampler)
        self.take_X(X)
        self.Xb = self.offset_b = self.y = self.centre = None
        if X_b is not None:
            self.Xb = check_X(X_b)
            if self.Xb.shape != self.X.shape:
                raise ValueError(f"X_b must have the shape of X_a {self.X.shape}, got {self.Xb.shape}")
        if transform not in TRANSFORMS:
            raise ValueError(f"unknown transform {transform!r}: use one of {', '.join(TRANSFORMS)}")
        self.code = TRANSFORMS[transform]
        self.take_offset(offset)
        self.offset_b = check_offset(offset_b, self.K, self.n)
        self.take_excluded(excluded)
        self.take_draws(draws, none="an average over the rows needs at least 1 draw")
        self.weights = check_weights(weights, self.n)
        self.labels, self.gid, self.n_rows = check_groups(groups, self.n, self.weights)
        self.G = int(self.labels.size)
        if y is not None:
            if self.K > 1:
                raise ValueError(f"y takes a fit with one output, this one has {self.K}")
            self.y = check_y(y, self.n)
            # the centre of a group is its weighted mean of y: the fitted values lie around it, so S2 sums small squares
            total = np.bincount(self.gid, weights=self.weights, minlength=self.G)
            self.centre = np.ascontiguousarray((np.bincount(self.gid, weights=self.weights * self.y, minlength=self.G) / total)[None, :])
        self.rows = bool(rows)
        if self.rows:
            self.hdi_prob = hdi_prob
            self.q, self.hdi_k, _ = spec(self.D, quantiles, hdi_prob, transform)
        self.ws_bytes = workspace_bytes(self.D, self.K, self.G, self.y is not None)
        if self.ws_bytes > block_bytes(*PW_BLOCK):
            raise ValueError(f"the partial sums of {self.D} draws x {self.K} outputs x {self.G} groups take {self.ws_bytes} bytes, "
                             f"more than a block may take ({block_bytes(*PW_BLOCK)}, {PW_BLOCK[0]}): use fewer draws or groups")
        self.take_history()

    def bytes_per_row(self) -> int:
        """Device bytes one row of a block costs: its covariates and its D K predictions -- twice for a contrast -- the
        weight, the group, ``y``, the offsets, and the per-row summary of ``rows``.  The partial sums, held across all
        blocks, are not per row: :meth:`run` takes them off what a block may take (``Job.blocks(reserved=)``)."""
        arms = 2 if self.Xb is not None else 1
        per = arms * 8 * (self.p + self.K * self.D) + 8 + 4
        per += 8 * (self.y is not None) + 8 * self.K * ((self.offset is not None) + (self.offset_b is not None))
        if self.rows:
            per += 8 * self.K * (2 + self.q.size + 2)
        return per

    def run(self) -> dict:
        be = self.hip_backend("averages over the rows run")
        lib, mem = be.lib, be.mem
        reduce_, finish, query = lib.rowreduce_entry_points()
        D, K, G, n, has_y = self.D, self.K, self.G, self.n, self.y is not None
        if int(query(D, K, G, int(has_y))) != self.ws_bytes:
            raise _abi.PGBError(f"pgb_row_reduce_workspace_bytes({D}, {K}, {G}, {int(has_y)}) is not {self.ws_bytes}")
        ptr = lambda buf: None if buf is None else mem.ptr(buf)  # noqa: E731
        ws = mem.empty((self.ws_bytes // 8,), np.float64)
        cd = None if self.centre is None else mem.from_host(self.centre)
        stats = np.empty((2 + self.q.size + 2, K, n)) if self.rows else None
        for blk in self.blocks(be, self.bytes_per_row(), y=has_y, predict=True, reserved=self.ws_bytes):
            r0, r1, nb = blk.r0, blk.r1, blk.nb
            wd, gd = mem.from_host(self.weights[r0:r1]), mem.from_host(self.gid[r0:r1])
            mb = obd = None
            if self.Xb is not None:
                mb = self.predict(be, mem.from_host(self.Xb[r0:r1]), nb)
                if self.offset_b is not None:
                    obd = mem.from_host(np.ascontiguousarray(self.offset_b[:, r0:r1]))
            rc = reduce_(mem.ptr(blk.md), ptr(mb), D, K, nb, nb, mem.ptr(wd), mem.ptr(gd), ptr(blk.yd), ptr(blk.od), ptr(obd),
                         ptr(cd), G, self.code, r0, int(r0 == 0), mem.ptr(ws), mem.ptr(blk.md) if self.rows else None,
                         mem.stream_ptr)
            lib.check(rc, "pgb_row_reduce")
            if self.rows:  # (the kernel has written v over the predictions of the first arm: no offset, no transform left)
                got = summary_block(lib, mem, blk.md, D, K * nb, K * nb, None, TRANSFORMS["identity"], self.q, self.hdi_k)
                stats[:, :, r0:r1] = got.reshape(-1, K, nb)
        n_out = 6 if has_y else 2
        od, wod = mem.empty((n_out * D * K * G,), np.float64), mem.empty((G,), np.float64)
        counts = (C.c_int64 * 2)()
        rc = finish(mem.ptr(ws), D, K, G, int(has_y), ptr(cd), mem.ptr(od), mem.ptr(wod), counts, mem.stream_ptr)
        lib.check(rc, "pgb_row_reduce_finish")
        out = np.ascontiguousarray(np.moveaxis(mem.to_host(od).reshape(n_out, D, K, G), 2, 3))  # (n_out, D, G, K)
        res = {"group_labels": self.labels.copy(), "weight": mem.to_host(wod), "n_rows": self.n_rows.copy(), "n_draws": D,
               "n_nonfinite": int(counts[0])}
        if has_y:
            names = ("mean", "var_fit", "bias", "mse", "var_res", "r2")
            res.update({name: out[j, :, :, 0].copy() for j, name in enumerate(names) if name != "mean"})
            res["rmse"] = np.sqrt(res["mse"])
        else:
            res["mean"] = out[0].copy()
        if self.rows:
            res["rows"] = result(stats, n, K, self.q, self.hdi_prob, self.hdi_k, D)
        return res


def average_prediction(sampler, X, weights=None, groups=None, draws=None, transform: str = "identity", offset=None,
                       excluded=None) -> dict:
    """Per-draw weighted means over the rows of ``X`` of the BART function, by group, computed on the device:
    ``mean[d, g, k] = sum_i w_i T(f_d,k(x_i) + offset_k,i) / sum_i w_i`` over the rows ``i`` of group ``g``.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns (several chains are
    one pool).  ``weights``: ``(n_rows,)``, finite and >= 0 (default: ones) -- poststratification cells, survey
    weights.  ``groups``: ``(n_rows,)`` labels of one sortable kind, no NaN (default: one group, label 0); every group needs a
    positive total weight; at most 4096 groups, and the partial sums -- 1 KiB per (draw, output, group) -- must fit
    ``PGB_PW_BLOCK_BYTES``.  ``draws``: indexes of the stored draws (default: all).  ``transform``, ``offset``
    ``(K, n_rows)``, ``excluded``: as in ``posterior_summary``.

    Returns ``mean`` ``(D, G, K)``; ``group_labels`` ``(G,)`` (``np.unique`` of ``groups``); ``weight`` ``(G,)``, the
    total weight of every group; ``n_rows`` ``(G,)``; ``n_draws``; and ``n_nonfinite``, how many of the D K n_rows
    transformed values were an infinity or a NaN (they are added all the same).  Rows are processed in blocks; a
    block and the partial sums together take at most ``PGB_PW_BLOCK_BYTES`` of device scratch (a block has at least 64
    rows); no bit of the result depends on the blocking.  Contiguous groups
    are the fast case (module docstring)."""
    return AverageJob(sampler, X, None, weights, groups, draws, transform, offset, None, excluded).run()


def average_contrast(sampler, X_a, X_b, weights=None, groups=None, draws=None, transform: str = "identity", offset_a=None,
                     offset_b=None, excluded=None, rows: bool = False, quantiles=DEFAULT_QUANTILES,
                     hdi_prob=DEFAULT_HDI_PROB) -> dict:
    """:func:`average_prediction` of the contrast ``T(f(X_a) + offset_a) - T(f(X_b) + offset_b)`` of two designs of the
    same shape -- ``X_a`` and ``X_b`` differ in the treatment column: the average treatment effect per draw, and with
    ``groups`` the conditional one by subgroup.  Both arms use the same draws and the same ``excluded``; each block of
    rows takes two ``pgb_predict`` calls and holds two prediction matrices.

    ``rows=True`` also returns ``rows``, the dict of ``posterior_summary`` (``mean``, ``sd``, ``var``, ``quantiles``,
    ``hdi``, ... per row, over the draws) of the per-row contrast: the kernel writes the contrast over the first arm's
    predictions and one ``pgb_row_summary`` per block reads it; ``quantiles`` and ``hdi_prob`` are its spec, and its
    limits on the number of draws (2 to 16384) then apply.

    Returns the keys of :func:`average_prediction` (``mean`` is exactly 0.0 where the two designs agree)."""
    if X_b is None:
        raise ValueError("X_b must have the shape of X_a, got None")
    return AverageJob(sampler, X_a, X_b, weights, groups, draws, transform, offset_a, offset_b, excluded, None, rows,
                      quantiles, hdi_prob).run()


def bayes_r2(sampler, X, y, weights=None, groups=None, draws=None, transform: str = "identity", offset=None) -> dict:
    """Per-draw goodness of fit of a one-output fit against observations ``y`` ``(n_rows,)``, by group, on the device.

    With ``v_i = T(f_d(x_i) + offset_i)`` and the weighted mean ``E`` over the rows of a group: ``bias = E[y - v]``,
    ``mse = E[(y - v)^2]`` (the Brier score for a Bernoulli ``y`` under the logistic or probit transform), ``rmse``,
    ``var_fit = E[v^2] - E[v]^2``, ``var_res = mse - bias^2`` and ``r2 = var_fit / (var_fit + var_res)``, the residual
    form of the Bayesian R-squared of Gelman, Goodrich, Gabry and Vehtari (2019).  Each is ``(D, G)``; ``r2`` lies in
    [0, 1] and is NaN for a draw whose fit is constant and equals ``y`` (0 / 0).

    The second moment of the fit is taken about a centre, the group's weighted mean of ``y`` computed on the host: the
    fitted values lie around it, which keeps ``var_fit`` away from the cancellation of two large numbers.

    Also returns ``group_labels``, ``weight``, ``n_rows``, ``n_draws`` and ``n_nonfinite`` as
    :func:`average_prediction` does.  A fit with more than one output is refused."""
    if y is None:
        raise ValueError("y must hold one value per row of X, got None")
    return AverageJob(sampler, X, None, weights, groups, draws, transform, offset, None, None, y).run()
