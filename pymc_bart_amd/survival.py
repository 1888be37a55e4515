"""Discrete-time survival analysis with stored posterior draws, on the device (``pgb_surv_curves``;
``include/pgbart_surv.h``): survival curves, the restricted mean survival time and the time a survival level is reached,
per row with a posterior band and per draw as averages over groups of rows (Sparapani, Logan, McCulloch and Laud 2016).

A Bernoulli (probit or logit) forest is fitted on PERSON-PERIOD rows -- one row per subject and grid time at risk, time
being a covariate (:func:`person_period`).  The curve of a subject is ``S(t_j | x) = prod_{l <= j} (1 - p_l)`` with
``p_l`` the link of ``f(t_l, x)``.  A grid of times on one column is a set of arms on that column
(:mod:`pymc_bart_amd.decision`): per draw only the trees that use the time column are walked, once at the row and once
per time.  The product couples the J predictions inside every (draw, row); ``pgb_surv_curves`` forms it in place, carried
across chunks of the grid, and both reductions that follow -- over the draws per row (``pgb_row_summary``) and over the
rows per draw (``pgb_row_reduce``) -- finish on the device.  Nothing of size draws x rows x times reaches the host.

* :func:`person_period` -- the training layout (pure NumPy).
* :func:`survival_matrix` -- ``S`` of every draw, row and time, for small calls.
* :func:`survival_curves` -- the summaries.

HIP backend only.  Every operation has a fixed order, so no bit of a result depends on the blocking of the rows, on the
chunking of the grid or on the launch geometry.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi
from ._stored import PW_BLOCK, block_bytes
from .average import workspace_bytes as reduce_workspace_bytes
from .decision import MAX_ARMS, ArmsJob, with_draw_stats
from .summary import DEFAULT_HDI_PROB, DEFAULT_QUANTILES, TRANSFORMS, spec, summary_block

MAX_TIMES = 4096   # the grid of one call
MAX_LEVELS = 4     # PGB_SURV_MAX_LEVELS
LINKS = ("probit", "logistic")
IDENTITY = TRANSFORMS["identity"]


def time_chunk() -> int:
    """Grid times per ``pgb_predict_arms`` / ``pgb_surv_curves`` call: the environment's ``PGB_SURV_TIME_CHUNK``,
    default 64 (``PGB_ARMS_MAX``, which it cannot exceed), at least 1."""
    return max(1, min(MAX_ARMS, int(os.environ.get("PGB_SURV_TIME_CHUNK", MAX_ARMS))))


def person_period(time, event, X=None, *, times=None) -> dict:
    """The person-period layout a discrete-time survival forest is fitted on.

    ``time`` ``(n,)``: the observed time of every subject (its event or its censoring); ``event`` ``(n,)``: true where
    the event was observed.  ``X`` ``(n, p)``: covariates (default: none).  ``times``: the grid, finite and strictly
    increasing (default: the sorted distinct values of ``time``); an observed time that is not on the grid is refused.

    Subject ``i`` contributes one row per grid time ``t_j <= time_i``; ``y`` is 1 only in the row ``t_j == time_i`` of a
    subject whose event was observed.  Returns ``X`` ``(N, 1 + p)`` with the time in the first column, ``y`` ``(N,)``,
    ``subject`` ``(N,)`` (the index of the row's subject) and ``times``; the rows of a subject are adjacent and in
    ascending time."""
    time = np.asarray(time, dtype=np.float64)
    if time.ndim != 1 or time.size < 1:
        raise ValueError(f"time must be a non-empty vector, got shape {time.shape}")
    if not np.all(np.isfinite(time)):
        raise ValueError("time must be finite")
    n = time.size
    event = np.asarray(event)
    if event.shape != (n,):
        raise ValueError(f"event must hold one value per subject: shape ({n},), got {event.shape}")
    if event.dtype.kind not in "biuf" or not np.all((event == 0) | (event == 1)):
        raise ValueError("event must hold booleans (or 0 / 1)")
    event = event.astype(bool)
    if X is None:
        X = np.empty((n, 0))
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    if X.ndim != 2 or X.shape[0] != n:
        raise ValueError(f"X must hold one row per subject: shape ({n}, p), got {X.shape}")
    grid = np.unique(time) if times is None else check_grid(times)
    at = np.searchsorted(grid, time)            # time_i == grid[at_i]
    off_grid = (at >= grid.size) | (grid[np.minimum(at, grid.size - 1)] != time)
    if np.any(off_grid):
        bad = int(np.argmax(off_grid))
        raise ValueError(f"time[{bad}] = {float(time[bad])!r} is not on the grid of times")
    rows = at + 1                               # the grid times at risk
    subject = np.repeat(np.arange(n), rows)
    first = np.cumsum(rows) - rows
    j = np.arange(subject.size) - first[subject]
    y = ((j == at[subject]) & event[subject]).astype(np.float64)
    return {"X": np.column_stack([grid[j], X[subject]]), "y": y, "subject": subject, "times": grid}


def check_grid(times) -> np.ndarray:
    """The grid of times: a finite, strictly increasing vector."""
    try:
        grid = np.asarray(times, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("times must be a vector of numbers") from None
    if grid.ndim != 1 or grid.size < 1:
        raise ValueError(f"times must be a non-empty vector, got shape {grid.shape}")
    if not np.all(np.isfinite(grid)) or np.any(np.diff(grid) <= 0.0):
        raise ValueError("times must be finite and strictly increasing")
    return np.ascontiguousarray(grid)


class SurvJob(ArmsJob):
    """One call of this module: an :class:`ArmsJob` whose arms are the grid times on the one column ``time_col``, handed
    to ``pgb_predict_arms`` a chunk at a time.  The arguments are taken in this order: ``X``, ``time_col``, the grid,
    the origin, ``output``, the link, the offset, the draws and -- :func:`survival_curves` only -- the summary spec,
    the levels, the weights, the groups, the size of the partial sums; then the history.  The backend is asked for
    last."""

    def __init__(self, sampler, X, times, time_col, output, link, offset, origin, draws, backend):
        super(ArmsJob, self).__init__(sampler)
        self.given_backend = backend
        self.take_X(X)
        if isinstance(time_col, (bool, np.bool_)) or not isinstance(time_col, (int, np.integer)) or not 0 <= int(time_col) < self.p:
            raise ValueError(f"time_col must be an integer in [0, {self.p}), got {time_col!r}")
        self.cols, self.s = np.array([int(time_col)], np.int32), 1
        self.times = check_grid(times)
        self.J = int(self.times.size)
        if self.J > MAX_TIMES:
            raise ValueError(f"at most {MAX_TIMES} times per call, got {self.J}")
        origin = float(origin)
        if not np.isfinite(origin) or not origin < self.times[0]:
            raise ValueError(f"origin must be finite and < times[0] = {float(self.times[0])!r}, got {origin!r}")
        self.dt = np.ascontiguousarray(np.diff(np.concatenate([[origin], self.times])))
        with np.errstate(over="ignore"):
            self.beyond = float(self.times[-1] + self.dt[-1])
        if not np.all(np.isfinite(self.dt)) or not np.isfinite(self.beyond) or not self.beyond > self.times[-1]:
            raise ValueError("the widths of the grid (np.diff([origin, *times])) must be finite, and so must times[-1] + "
                             "the last width")
        self.take_output(output)
        if link not in LINKS:
            raise ValueError(f"unknown link {link!r}: use one of {', '.join(LINKS)}")
        self.code = TRANSFORMS[link]
        self.take_row_offset(offset)
        self.take_draws(draws, none="a survival curve needs at least 1 draw")
        self.picks = np.arange(self.D, dtype=np.int32)
        self.levels = np.empty(0)
        self.chunk = time_chunk()

    def take_summaries(self, quantiles, hdi_prob, levels, weights, groups):
        self.per_row = self.D >= 2  # (a summary over the draws needs two of them; the spec is checked all the same)
        self.q, self.hdi_k, _ = spec(max(self.D, 2), quantiles, hdi_prob, "identity")
        self.take_hdi_prob(hdi_prob)
        lv = np.asarray([] if levels is None else levels, dtype=np.float64)
        if lv.ndim != 1 or lv.size > MAX_LEVELS:
            raise ValueError(f"levels must be a vector of at most {MAX_LEVELS} survival levels, got shape {lv.shape}")
        if lv.size and not np.all((lv > 0.0) & (lv <= 1.0)):  # (a NaN fails both comparisons)
            raise ValueError("levels must lie in (0, 1]")
        self.levels = np.ascontiguousarray(lv)
        self.take_rows(weights, groups)
        self.ws_one = reduce_workspace_bytes(self.D, 1, self.G, False)
        self.ws_bytes = (self.J + 1) * self.ws_one
        limit = block_bytes(*PW_BLOCK)
        if self.ws_bytes + 64 * self.curves_row_bytes() > limit:
            raise ValueError(f"the partial sums of {self.J} times + 1 x {self.D} draws x {self.G} groups take {self.ws_bytes} bytes "
                             f"and a block of 64 rows {64 * self.curves_row_bytes()}, more than a block may take ({limit}, "
                             f"{PW_BLOCK[0]}): use fewer times, draws or groups")

    # ------------------------------------------------------------------ sizes
    def matrix_row_bytes(self) -> int:
        """Device bytes one row of a block costs :func:`survival_matrix`: its covariates, its ``D K`` predictions, the
        ``D K`` predictions of every time of a chunk, its state and its offset."""
        A = min(self.chunk, self.J)
        return 8 * self.p + (A + 1) * self.D * self.K * 8 + (2 + self.levels.size) * self.D * 8 + 8

    def curves_row_bytes(self) -> int:
        """... and :func:`survival_curves`: also the weight, the group and the summary of one slab."""
        return self.matrix_row_bytes() + 8 + 4 + 8 * (2 + self.q.size + 2)

    # ------------------------------------------------------------------ the run
    def hip(self):
        """The backend and the entry points; the CPU oracle has none: ``NotImplementedError`` naming
        ``pgb_surv_curves``."""
        be = self.pick_backend()
        surv = be.lib.surv_entry_points()
        return be, be.lib.arms_entry_points()[0], surv

    def chunks(self, be, predict_arms, surv, blk, offd, state, cnt, lens):
        """Generator over the chunks of the grid at one block of rows: ``pgb_predict_arms`` with the chunk's times as
        the arms, then ``pgb_surv_curves`` in place on the call's output -> ``(c0, c1, od)``, ``od`` ``[A][D][K][nb]``
        holding ``S`` in the cells of that output."""
        mem, nb, D, K, Q = be.mem, blk.nb, self.D, self.K, int(self.levels.size)
        for c0 in range(0, self.J, self.chunk):
            c1 = min(self.J, c0 + self.chunk)
            t, dt = self.times[c0:c1], self.dt[c0:c1]
            od = self.arms_block(be, predict_arms, blk, lens, arms=np.ascontiguousarray(t[:, None]))
            # output k of the arm-major matrix, without a copy: element (a, d, i) at a D K nb + d K nb + k nb + i
            rc = surv(mem.ptr(od[self.output * nb:]), D * K * nb, K * nb, D, c1 - c0, nb, None if offd is None else mem.ptr(offd),
                      self.code, t.ctypes.data, dt.ctypes.data, self.levels.ctypes.data if Q else None, Q, self.beyond,
                      int(c0 == 0), mem.ptr(state), mem.ptr(cnt), mem.stream_ptr)
            be.lib.check(rc, "pgb_surv_curves")
            yield c0, c1, od

    def slab(self, od, a: int, nb: int):
        """The ``[D][nb]`` matrix (leading dimension ``K nb``) of time ``a`` of a chunk's output."""
        return od[(a * self.D * self.K + self.output) * nb:]

    def run_matrix(self) -> np.ndarray:
        self.take_history()
        be, predict_arms, surv = self.hip()
        mem, D, K = be.mem, self.D, self.K
        out = np.empty((D, self.n, self.J))
        cnt = mem.from_host(np.zeros(1, np.int64))
        lens = np.zeros(D, np.int32)
        for blk in self.blocks(be, self.matrix_row_bytes(), predict=True):
            nb = blk.nb
            offd = None if self.off is None else mem.from_host(self.off[blk.r0:blk.r1])
            state = mem.empty((2 * D * nb,), np.float64)
            for c0, c1, od in self.chunks(be, predict_arms, surv, blk, offd, state, cnt, lens):
                got = mem.to_host(od).reshape(c1 - c0, D, K, nb)[:, :, self.output]
                out[:, blk.r0:blk.r1, c0:c1] = np.moveaxis(got, 0, 2)
        return out

    def run_curves(self) -> dict:
        self.take_history()
        be, predict_arms, surv = self.hip()
        lib, mem = be.lib, be.mem
        reduce_, finish, query = lib.rowreduce_entry_points()
        D, K, G, J, n, Q = self.D, self.K, self.G, self.J, self.n, int(self.levels.size)
        if int(query(D, 1, G, 0)) != self.ws_one:
            raise _abi.PGBError(f"pgb_row_reduce_workspace_bytes({D}, 1, {G}, 0) is not {self.ws_one}")
        words = self.ws_one // 8
        ws = mem.empty(((J + 1) * words,), np.float64)  # one workspace per time, then the one of the RMST
        cnt = mem.from_host(np.zeros(1, np.int64))
        lens = np.zeros(D, np.int32)
        nq = int(self.q.size)
        no_q = np.empty(0)
        if self.per_row:
            surv_stats, rmst_stats = np.empty((2 + nq + 2, n, J)), np.empty((2 + nq + 2, n))
            time_q = np.empty((nq, n, Q))

        def reduce_slab(md, ld, blk, wd, gd, j):
            rc = reduce_(mem.ptr(md), None, D, 1, blk.nb, ld, mem.ptr(wd), mem.ptr(gd), None, None, None, None, G, IDENTITY,
                         blk.r0, int(blk.r0 == 0), mem.ptr(ws[j * words:]), None, mem.stream_ptr)
            lib.check(rc, "pgb_row_reduce")

        for blk in self.blocks(be, self.curves_row_bytes(), predict=True, reserved=self.ws_bytes):
            r0, r1, nb = blk.r0, blk.r1, blk.nb
            wd, gd = mem.from_host(self.weights[r0:r1]), mem.from_host(self.gid[r0:r1])
            offd = None if self.off is None else mem.from_host(self.off[r0:r1])
            state = mem.empty(((2 + Q) * D * nb,), np.float64)
            for c0, c1, od in self.chunks(be, predict_arms, surv, blk, offd, state, cnt, lens):
                for a in range(c1 - c0):
                    md = self.slab(od, a, nb)
                    if self.per_row:
                        surv_stats[:, r0:r1, c0 + a] = summary_block(lib, mem, md, D, nb, K * nb, None, IDENTITY, self.q, self.hdi_k)
                    reduce_slab(md, K * nb, blk, wd, gd, c0 + a)
            rd = state[D * nb:]  # (the slab R; T[l] follows it)
            if self.per_row:
                rmst_stats[:, r0:r1] = summary_block(lib, mem, rd, D, nb, nb, None, IDENTITY, self.q, self.hdi_k)
                for l in range(Q):
                    got = summary_block(lib, mem, state[(2 + l) * D * nb:], D, nb, nb, None, IDENTITY, self.q, 0)
                    time_q[:, r0:r1, l] = got[2:2 + nq]
            reduce_slab(rd, nb, blk, wd, gd, J)
        avg = np.empty((J + 1, D, G))
        outd, wod = mem.empty((2 * D * G,), np.float64), mem.empty((G,), np.float64)
        counts = (C.c_int64 * 2)()
        for j in range(J + 1):
            rc = finish(mem.ptr(ws[j * words:]), D, 1, G, 0, None, mem.ptr(outd), mem.ptr(wod), counts, mem.stream_ptr)
            lib.check(rc, "pgb_row_reduce_finish")
            avg[j] = mem.to_host(outd).reshape(2, D, G)[0]
        res = {"group_labels": self.labels.copy(), "group_weight": mem.to_host(wod), "n_rows": self.n_rows.copy(), "n_draws": D,
               "n_nonfinite": int(mem.to_host(cnt)[0]), "n_list_trees": lens.astype(np.int64), "times": self.times.copy(),
               "beyond": self.beyond, "levels": self.levels.copy(), "q": self.q.copy()}
        if self.per_row:
            for name, st in (("surv", surv_stats), ("rmst", rmst_stats)):
                res.update({name + "_mean": st[0].copy(), name + "_sd": np.sqrt(st[1]), name + "_quantiles": st[2:2 + nq].copy(),
                            name + "_hdi": st[2 + nq:4 + nq].copy()})
            res["time_quantiles"] = time_q
        per_draw = {"surv_avg": np.ascontiguousarray(np.moveaxis(avg[:J], 0, 2)), "rmst_avg": avg[J].copy()}
        return with_draw_stats(res, per_draw, self.hdi_prob)


def survival_matrix(sampler, X, times, *, time_col=0, output=0, link="probit", offset=None, origin=0.0, draws=None,
                    backend=None) -> np.ndarray:
    """The survival probabilities of every stored draw at the rows of ``X`` and the grid ``times``, computed on the
    device: ``(D, n, J)``, ``S[d, i, j] = prod_{l <= j} (1 - link(f_d(x_i with times[l] in time_col) + offset_i))``.
    For small calls -- :func:`survival_curves` returns the summaries without this array leaving the device.  The
    arguments are those of :func:`survival_curves`."""
    return SurvJob(sampler, X, times, time_col, output, link, offset, origin, draws, backend).run_matrix()


def survival_curves(sampler, X, times, *, time_col=0, output=0, link="probit", offset=None, origin=0.0,
                    quantiles=DEFAULT_QUANTILES, hdi_prob=DEFAULT_HDI_PROB, levels=(0.5,), weights=None, groups=None,
                    draws=None, backend=None) -> dict:
    """Discrete-time survival curves of a fit on person-period rows (:func:`person_period`), on the device.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns (several chains are
    one pool).  ``X`` ``(n, p)``: one row per subject with the columns of the fit; column ``time_col`` is ignored -- the
    grid replaces it.  ``times`` ``(J,)``: finite and strictly increasing, ``origin < times[0]``, at most 4096.  The
    hazard of time ``t_l`` in draw ``d`` is ``p_l = link(f_d(t_l, x_i) + offset_i)`` of output ``output`` (``link``:
    ``"probit"`` or ``"logistic"``; ``offset`` ``(n,)``), the curve is ``S_j = prod_{l <= j} (1 - p_l)`` with ``1 - p``
    computed as the link at the negated predictor, and with ``dt = np.diff([origin, *times])`` the restricted mean
    survival time up to ``times[-1]`` is ``rmst = sum_j S_{j-1} dt_j`` (``S_{-1} = 1``): the curve is a step function.
    ``levels``: up to 4 survival levels in (0, 1]; the time a level ``u`` is reached is the first ``t_j`` with
    ``S_j <= u``, and ``beyond = times[-1] + dt[-1]`` where the curve stays above ``u`` on the whole grid.

    Returns, per row over the draws (``quantiles``, ``hdi_prob``: as in ``posterior_summary``; they need at least 2
    draws and are left out with one): ``surv_mean``, ``surv_sd`` ``(n, J)``, ``surv_quantiles`` ``(Q, n, J)``,
    ``surv_hdi`` ``(2, n, J)``; ``rmst_mean``, ``rmst_sd`` ``(n,)``, ``rmst_quantiles`` ``(Q, n)``, ``rmst_hdi``
    ``(2, n)``; ``time_quantiles`` ``(Q, n, len(levels))``, the posterior quantiles of the time a level is reached -- a
    value equal to ``beyond`` (returned under that key) says "not within the grid".  Per draw, as weighted means over
    the rows of a group (``weights``, ``groups``: as in ``average_prediction``): ``surv_avg`` ``(D, G, J)`` and
    ``rmst_avg`` ``(D, G)``, each with ``_mean``, ``_sd`` and ``_hdi`` over the draws.  And ``group_labels``,
    ``group_weight``, ``n_rows`` ``(G,)``; ``n_draws``; ``n_nonfinite``, the factors ``1 - p`` that were a NaN (they are
    multiplied in all the same); ``n_list_trees`` ``(D,)``, the trees of every draw that use the time column: all that
    is ever walked for the grid; ``times``, ``levels``, ``q``.

    The per-draw results of two calls with the same ``draws=`` are paired: the contrast of two designs (treated against
    control, say) per draw is their difference, taken on the host.  Per-row summaries of such a contrast are not
    computed here.

    Per block of rows one ``pgb_predict``; per chunk of at most ``PGB_SURV_TIME_CHUNK`` times (default and most: 64)
    one ``pgb_predict_arms`` and one ``pgb_surv_curves``; then one ``pgb_row_summary`` and one ``pgb_row_reduce`` per
    time.  A block and the partial sums -- 1 KiB per (time, draw, group) -- together take at most
    ``PGB_PW_BLOCK_BYTES`` of device scratch.  No bit of a result depends on the blocking or on the chunking."""
    job = SurvJob(sampler, X, times, time_col, output, link, offset, origin, draws, backend)
    job.take_summaries(quantiles, hdi_prob, levels, weights, groups)
    return job.run_curves()
