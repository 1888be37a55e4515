"""Friedman & Popescu's H-statistic of stored posterior draws on the device (``pgb_hstat_*``,
``include/pgbart_hstat.h``): which columns act TOGETHER, per draw and so with posterior bands.

``h2[a, b]`` is the share of the variance of the two-way partial dependence of ``(a, b)`` that the two one-way functions
do not explain; ``h2_total[a]`` the share of the variance of the fit that column ``a`` carries through interactions with
anything else.  The definition needs a partial dependence at every data point -- rows x rows predictions per function.
Two facts remove that cost.  The interaction term of a pair receives contributions only from the trees that use BOTH
columns (the use lists of ``include/pgbart_permimp.h``, intersected), and the weight with which a hybrid row "row i on
S, row r elsewhere" reaches a leaf is a product of factors that depend on ``i`` alone or on ``r`` alone.  So one pass
over the background rows leaves a few moments per leaf (``pgb_hstat_background``), one pass over the evaluation rows
combines them (``pgb_hstat_rows``) and reduces ``J``, ``T``, ``I`` and ``J_a + J_b + I_ab`` to partial sums that stay on
the device; ``pgb_hstat_finish`` turns them into variances and ratios.  The variance of the fit itself is
``pgb_row_reduce``'s ``var_fit`` of a ``pgb_predict`` block.  Nothing of size draws x rows leaves the device and nothing
of size rows x rows exists anywhere.

HIP backend only.  Every sum has a fixed order and the finish is sequential, so no bit of a result depends on the
blocking of the rows, on the chunking of the pairs, on the launch geometry or on which other pairs are asked for.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._stored import PW_BLOCK, Job, block_bytes, check_X, check_cols, row_blocks
from .average import check_weights, workspace_bytes
from .importance import hdi
from .summary import DEFAULT_HDI_PROB, TRANSFORMS, spec, summary_block

MAX_PAIRS = 4096  # PGB_HSTAT_MAX_PAIRS
PER_DRAW = ("h2", "h", "inter_sd", "h2_total", "total_inter_sd", "main_sd")


def check_pairs(pairs, cols: np.ndarray, p: int) -> np.ndarray:
    """The pairs of one call as ``(n_pairs, 2)`` column indices ordered ``a < b`` (``None``: all pairs of ``cols``)."""
    if pairs is None:
        c = np.sort(cols)
        return np.asarray([(a, b) for i, a in enumerate(c) for b in c[i + 1:]], np.int32).reshape(-1, 2)
    try:
        arr = np.asarray(list(pairs), dtype=np.int64)
    except (TypeError, ValueError):
        raise ValueError("pairs must be a list of 2-tuples of column indices") from None
    if arr.size == 0:
        return np.zeros((0, 2), np.int32)
    if arr.ndim != 2 or arr.shape[1] != 2:
        raise ValueError(f"pairs must be a list of 2-tuples of column indices, got shape {arr.shape}")
    if arr.min() < 0 or arr.max() >= p:
        raise ValueError(f"pairs must index the {p} columns of X")
    if np.any(arr[:, 0] == arr[:, 1]):
        raise ValueError(f"pairs must name two different columns, got {tuple(arr[arr[:, 0] == arr[:, 1]][0].tolist())}")
    arr = np.sort(arr, axis=1)
    if np.unique(arr, axis=0).shape[0] != arr.shape[0]:
        raise ValueError("pairs must not name a pair twice (in either order)")
    missing = np.setdiff1d(arr.ravel(), cols)
    if missing.size:
        raise ValueError(f"pairs names column {int(missing[0])}, which is not among cols")
    return np.ascontiguousarray(arr, dtype=np.int32)


class Chunk:
    """The columns and the pairs (slots of those columns) of one set of ``pgb_hstat_*`` calls."""

    def __init__(self, cols, pair_ids, pairs):
        self.cols = np.ascontiguousarray(cols, np.int32)
        self.pair_ids = np.asarray(pair_ids, np.int64)
        slot = {int(c): s for s, c in enumerate(self.cols)}
        self.slots = np.ascontiguousarray([[slot[int(a)], slot[int(b)]] for a, b in pairs[self.pair_ids]], np.int32).reshape(-1, 2)
        self.q, self.n_pairs = int(self.cols.size), int(self.pair_ids.size)
        self.ws_bytes = 0
        self.n_common = None

    def halves(self, pairs) -> list:
        if self.n_pairs > 1:
            cut = self.n_pairs // 2
            return [Chunk(np.unique(pairs[ids]), ids, pairs) for ids in (self.pair_ids[:cut], self.pair_ids[cut:])]
        if self.n_pairs == 0 and self.q > 1:
            return [Chunk(c, [], pairs) for c in (self.cols[:self.q // 2], self.cols[self.q // 2:])]
        return []


class HstatJob(Job):
    """One call of :func:`friedman_h`.  The arguments are taken in this order: ``X``, the draws, ``hdi_prob``, the
    columns, the pairs, the background, the weights, the background's weights, the history; the backend is asked for
    last."""

    def __init__(self, sampler, X, cols, pairs, background, weights, background_weights, draws, hdi_prob, rows, backend):
        super().__init__(sampler)
        if backend is not None:
            self.backend = lambda: backend
        self.take_X(X)
        self.take_draws(draws, none="the H-statistic needs at least 1 draw")
        if not 0.0 < float(hdi_prob) < 1.0:
            raise ValueError(f"hdi_prob must lie in (0, 1), got {hdi_prob!r}")
        self.hdi_prob = float(hdi_prob)
        self.cols = check_cols(np.arange(self.p) if cols is None else cols, self.p)
        if np.unique(self.cols).size != self.cols.size:
            raise ValueError("cols must not name a column twice")
        self.q = int(self.cols.size)
        self.pairs = check_pairs(pairs, self.cols, self.p)
        self.n_pairs = int(self.pairs.shape[0])
        if background is None:
            if background_weights is not None:
                raise ValueError("background_weights needs a background: without one the rows of X, with weights, are the background")
            self.Xb = self.X
        else:
            self.Xb = check_X(background)
            if self.Xb.shape[1] != self.p:
                raise ValueError(f"background must have the {self.p} columns of X, got shape {self.Xb.shape}")
        self.weights = check_weights(weights, self.n)
        if not np.sum(self.weights) > 0.0:
            raise ValueError("weights must have a positive total")
        if background is None:
            self.bweights = self.weights
        else:
            try:
                self.bweights = check_weights(background_weights, int(self.Xb.shape[0]))
            except ValueError as e:
                raise ValueError(str(e).replace("weights", "background_weights", 1).replace("of X", "of background")) from None
            if not np.sum(self.bweights) > 0.0:
                raise ValueError("background_weights must have a positive total")
        self.rows = bool(rows)
        if self.rows:
            self.sq, self.hdi_k, _ = spec(self.D, None, self.hdi_prob, "identity")
        self.take_history()

    # ------------------------------------------------------------------ sizes
    def row_bytes(self, ch: Chunk) -> int:
        """Device bytes one evaluation row of a block costs in a chunk: its covariates, its weight, its ``J`` of every
        (draw, column, output) and, with ``rows``, its ``T`` and ``I`` and their summaries."""
        per = 8 * self.p + 8 + 8 * self.D * ch.q * self.K
        if self.rows:
            per += 8 * (self.D + 4) * (ch.q + ch.n_pairs) * self.K
        return per

    def chunks(self, be) -> list:
        """The chunks of the call, each with its workspace inside the block rule: the pairs are halved until they fit;
        a column's own results come from the first chunk that holds it, the columns no pair names from chunks without
        pairs."""
        ws_bytes = be.lib.hstat_entry_points()[0]
        limit = block_bytes(*PW_BLOCK)
        todo = []
        for i0 in range(0, self.n_pairs, MAX_PAIRS):
            ids = np.arange(i0, min(self.n_pairs, i0 + MAX_PAIRS))
            todo.append(Chunk(np.unique(self.pairs[ids]), ids, self.pairs))
        named = np.unique(self.pairs) if self.n_pairs else np.zeros(0, np.int32)
        rest = np.setdiff1d(self.cols, named)
        if rest.size:
            todo.append(Chunk(rest, [], self.pairs))
        done, carr, picks = [], self.pool.as_c(), np.arange(self.D, dtype=np.int32)
        while todo:
            ch = todo.pop(0)
            got = C.c_int64(0)
            common = np.zeros((self.D, ch.n_pairs), np.int32)
            rc = ws_bytes(C.byref(carr), self.fidx.ctypes.data, self.D, self.m, self.p, ch.cols.ctypes.data, ch.q,
                          ch.slots.ctypes.data if ch.n_pairs else None, ch.n_pairs, picks.ctypes.data, self.D, C.byref(got),
                          common.ctypes.data if ch.n_pairs else None)
            be.lib.check(rc, "pgb_hstat_workspace_bytes")
            ch.ws_bytes, ch.n_common = int(got.value), common
            if ch.ws_bytes + 64 * self.row_bytes(ch) > limit:
                parts = ch.halves(self.pairs)
                if not parts:
                    what = f"the pair {tuple(self.pairs[ch.pair_ids[0]].tolist())}" if ch.n_pairs else f"column {int(ch.cols[0])}"
                    raise ValueError(f"{what} of {self.D} draws takes {ch.ws_bytes} bytes of moments, more than a block may take "
                                     f"({limit}, {PW_BLOCK[0]}): use fewer draws")
                todo = parts + todo
                continue
            done.append(ch)
        return done

    # ------------------------------------------------------------------ the run
    def var_fit(self, be) -> np.ndarray:
        """``var_fit (D, K)`` of the fit over the rows of ``X``: ``pgb_row_reduce`` of ``pgb_predict`` blocks, one group."""
        lib, mem = be.lib, be.mem
        reduce_, finish_, _ = lib.rowreduce_entry_points()
        D, K = self.D, self.K
        nbytes = workspace_bytes(D, K, 1, False)
        ws = mem.empty((nbytes // 8,), np.float64)
        for blk in self.blocks(be, 8 * (self.p + K * D) + 8 + 4, predict=True, reserved=nbytes):
            wd, gd = mem.from_host(self.weights[blk.r0:blk.r1]), mem.from_host(np.zeros(blk.nb, np.int32))
            rc = reduce_(mem.ptr(blk.md), None, D, K, blk.nb, blk.nb, mem.ptr(wd), mem.ptr(gd), None, None, None, None, 1,
                         TRANSFORMS["identity"], blk.r0, int(blk.r0 == 0), mem.ptr(ws), None, mem.stream_ptr)
            lib.check(rc, "pgb_row_reduce")
        od, wod = mem.empty((2 * D * K,), np.float64), mem.empty((1,), np.float64)
        counts = (C.c_int64 * 2)()
        rc = finish_(mem.ptr(ws), D, K, 1, 0, None, mem.ptr(od), mem.ptr(wod), counts, mem.stream_ptr)
        lib.check(rc, "pgb_row_reduce_finish")
        return np.ascontiguousarray(mem.to_host(od).reshape(2, D, K)[1])

    def run(self) -> dict:
        be = self.hip_backend("the H-statistic runs")
        lib, mem = be.lib, be.mem
        _, background, rows_, finish_ = lib.hstat_entry_points()
        D, K, n, p = self.D, self.K, self.n, self.p
        chunks = self.chunks(be)
        var_fit = self.var_fit(be)
        carr, picks = self.pool.as_c(), np.arange(D, dtype=np.int32)
        col_out = {key: np.full((D, self.q, K), np.nan) for key in ("main_var", "total_var", "h2_total")}
        pair_out = {key: np.full((D, self.n_pairs, K), np.nan) for key in ("inter_var", "h2")}
        n_common = np.zeros((D, self.n_pairs), np.int64)
        stats_t = np.empty((4, self.q, K, n)) if self.rows else None
        stats_i = np.empty((4, self.n_pairs, K, n)) if self.rows else None
        slot_of = {int(c): s for s, c in enumerate(self.cols)}
        seen = set()
        limit = block_bytes(*PW_BLOCK)
        for ch in chunks:
            jobs = (ch.cols.ctypes.data, ch.q, ch.slots.ctypes.data if ch.n_pairs else None, ch.n_pairs, picks.ctypes.data, D)
            ws = mem.empty((ch.ws_bytes // 8,), np.float64)
            nbk = int(self.Xb.shape[0])
            for r0, r1 in row_blocks(nbk, 8 * p + 8, limit - ch.ws_bytes):
                xd, vd = mem.from_host(self.Xb[r0:r1]), mem.from_host(self.bweights[r0:r1])
                rc = background(C.byref(carr), self.fidx.ctypes.data, D, self.m, mem.ptr(xd), r1 - r0, p, p, mem.ptr(vd), r0,
                                int(r0 == 0), *jobs, mem.ptr(ws), mem.stream_ptr)
                lib.check(rc, "pgb_hstat_background")
            for blk in self.blocks(be, self.row_bytes(ch), reserved=ch.ws_bytes):
                r0, nb = blk.r0, blk.nb
                wd = mem.from_host(self.weights[r0:blk.r1])
                jd = mem.empty((D * ch.q * K * nb,), np.float64)
                td = mem.empty((D * ch.q * K * nb,), np.float64) if self.rows else None
                idv = mem.empty((D * ch.n_pairs * K * nb,), np.float64) if self.rows and ch.n_pairs else None
                rc = rows_(C.byref(carr), self.fidx.ctypes.data, D, self.m, mem.ptr(blk.xd), nb, p, p, mem.ptr(wd), r0,
                           int(r0 == 0), *jobs, mem.ptr(ws), mem.ptr(jd), None if td is None else mem.ptr(td),
                           None if idv is None else mem.ptr(idv), mem.stream_ptr)
                lib.check(rc, "pgb_hstat_rows")
                if self.rows:  # (the per-row T and I are [D][items * K * nb] matrices pgb_row_summary takes as they are)
                    for buf, items, stats, where in ((td, ch.q, stats_t, [slot_of[int(c)] for c in ch.cols]),
                                                     (idv, ch.n_pairs, stats_i, ch.pair_ids)):
                        if buf is None:
                            continue
                        got = summary_block(lib, mem, buf, D, items * K * nb, items * K * nb, None, TRANSFORMS["identity"],
                                            self.sq, self.hdi_k)
                        stats[:, where, :, r0:blk.r1] = got.reshape(4, items, K, nb)
            outs = {key: np.empty((D, ch.q, K)) for key in col_out}
            outs.update({key: np.empty((D, max(ch.n_pairs, 1), K)) for key in pair_out})
            bad = C.c_int64(0)  # (the chunk's own count; the call's is taken below, once per column and pair)
            rc = finish_(mem.ptr(ws), D, ch.q, ch.n_pairs, K, var_fit.ctypes.data, *(outs[key].ctypes.data for key in
                         ("main_var", "total_var", "h2_total", "inter_var", "h2")), C.byref(bad), mem.stream_ptr)
            lib.check(rc, "pgb_hstat_finish")
            for key in pair_out:
                pair_out[key][:, ch.pair_ids] = outs[key][:, :ch.n_pairs]
            if ch.n_pairs:
                n_common[:, ch.pair_ids] = ch.n_common
            for s, c in enumerate(ch.cols.tolist()):
                if c in seen:
                    continue
                seen.add(c)
                for key in col_out:
                    col_out[key][:, slot_of[c]] = outs[key][:, s]
        nonfinite = sum(int(np.count_nonzero(~np.isfinite(arr))) for arr in (col_out["h2_total"], pair_out["h2"]))
        return self.results(col_out, pair_out, n_common, nonfinite, var_fit, stats_t, stats_i)

    def results(self, col_out, pair_out, n_common, nonfinite, var_fit, stats_t, stats_i) -> dict:
        K = self.K
        with np.errstate(invalid="ignore"):
            per_draw = {"h2": pair_out["h2"], "h": np.sqrt(pair_out["h2"]), "inter_sd": np.sqrt(pair_out["inter_var"]),
                        "h2_total": col_out["h2_total"], "total_inter_sd": np.sqrt(col_out["total_var"]),
                        "main_sd": np.sqrt(col_out["main_var"])}
        res = {"cols": self.cols.copy(), "pairs": self.pairs.copy(), "n_common_trees": n_common, "n_nonfinite": nonfinite,
               "n_draws": self.D, "var_fit": var_fit}
        for key in PER_DRAW:
            a = per_draw[key]                                           # (D, items, K)
            lo_hi = np.empty(a.shape[1:] + (2,))
            for s in range(a.shape[1]):
                for k in range(K):
                    lo_hi[s, k] = hdi(a[:, s, k], self.hdi_prob)
            with np.errstate(invalid="ignore"):
                res.update({key: a, key + "_mean": a.mean(axis=0), key + "_sd": a.std(axis=0), key + "_hdi": lo_hi})
        if self.rows:
            res["rows"] = {}
            for name, stats in (("total", stats_t), ("pair", stats_i)):
                by = np.ascontiguousarray(np.moveaxis(stats, 3, 1))     # (4, n, items, K)
                res["rows"][name] = {"mean": by[0], "sd": np.sqrt(by[1]), "hdi": np.ascontiguousarray(np.moveaxis(by[2:4], 0, -1))}
        if K == 1:  # (the K axis is dropped for one output)
            for key in PER_DRAW:
                res[key], res[key + "_mean"], res[key + "_sd"] = res[key][..., 0], res[key + "_mean"][..., 0], res[key + "_sd"][..., 0]
                res[key + "_hdi"] = res[key + "_hdi"][:, 0, :]
            res["var_fit"] = res["var_fit"][:, 0]
            if self.rows:
                for part in res["rows"].values():
                    part["mean"], part["sd"], part["hdi"] = part["mean"][..., 0], part["sd"][..., 0], part["hdi"][..., 0, :]
        return res


def friedman_h(sampler, X, cols=None, pairs=None, background=None, weights=None, background_weights=None, draws=None,
               hdi_prob: float = DEFAULT_HDI_PROB, rows: bool = False, backend=None) -> dict:
    """Friedman & Popescu's H-statistics of the columns ``cols`` (default: all) and the pairs ``pairs`` (default: all
    pairs of ``cols``) per stored draw, on the device.

    ``PD_S(x)`` is the partial dependence on the columns ``S``: the ``background``-weighted mean of the draw's
    prediction at the row that holds ``x`` on ``S`` and a background row elsewhere (a NaN is marginalised as always).
    With ``J_a = PD_a - PD_0``, ``I_ab = PD_ab - PD_a - PD_b + PD_0`` and ``T_a = f - PD_a - PD_{-a} + PD_0`` evaluated
    at the rows of ``X`` and variances taken over those rows with ``weights``:

    * ``h2[a, b] = var(I_ab) / var(J_a + J_b + I_ab)`` -- the denominator is the variance of the centred two-way
      partial dependence -- and ``h = sqrt(h2)``; ``inter_sd = sqrt(var(I_ab))`` is the same numerator in the units of
      the response, returned because H is known to blow up for pairs with weak main effects;
    * ``h2_total[a] = var(T_a) / var(f)`` and ``total_inter_sd = sqrt(var(T_a))``: ``a`` against everything else;
    * ``main_sd = sqrt(var(J_a))``.

    A numerator of exactly 0.0 gives 0.0 (a pair no tree of the draw uses together; a column whose trees use nothing
    else); otherwise the plain division, and an infinity or a NaN stays and is counted in ``n_nonfinite``.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns (several chains are
    one pool).  ``pairs``: a list of 2-tuples of column indices, each among ``cols``; they are returned ordered
    ``a < b``; ``pairs=[]`` gives the column results only.  ``background``: the matrix to marginalise over with
    ``background_weights`` (default: ``X`` itself with ``weights``, which is Friedman's definition).  ``weights``,
    ``background_weights``: finite and >= 0 with a positive total (default: ones).  ``draws``: indexes of the stored
    draws (default: all).

    Returns arrays over the draws -- the K axis is dropped for a fit with one output: ``h2``, ``h``, ``inter_sd``
    ``(D, n_pairs, K)``; ``h2_total``, ``total_inter_sd``, ``main_sd`` ``(D, q, K)``; each with ``_mean``, ``_sd``
    ``(items, K)`` and ``_hdi`` ``(items, K, 2)`` over the draws.  And ``pairs`` ``(n_pairs, 2)``, ``cols``,
    ``n_common_trees`` ``(D, n_pairs)`` (the trees of the draw that use both columns: all that is ever walked for the
    pair), ``var_fit`` ``(D, K)``, ``n_draws`` and ``n_nonfinite``.  ``rows=True`` (at least 2 draws) adds ``rows``:
    the posterior ``mean``, ``sd`` and ``hdi`` over the draws of the per-row ``T_a`` (``rows["total"]``, ``(n, q, K)``)
    and ``I_ab`` (``rows["pair"]``, ``(n, n_pairs, K)``) through ``pgb_row_summary``.

    Rows are processed in blocks and pairs in chunks whose moments fit ``PGB_PW_BLOCK_BYTES``; no bit of a result
    depends on either, nor on which other pairs or columns are asked for."""
    return HstatJob(sampler, X, cols, pairs, background, weights, background_weights, draws, hdi_prob, rows, backend).run()
