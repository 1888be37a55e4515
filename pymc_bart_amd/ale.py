"""Accumulated local effects (ALE; Apley & Zhu 2020) of stored posterior draws on the device (``pgb_predict_ale``,
``include/pgbart_ale.h``): the main effect of a column read off the rows the data hold, with posterior bands.

Partial dependence and ICE move a column across its whole grid at every row, so with correlated covariates they
evaluate the model at combinations the data never contain.  ALE moves a row only between the two edges of the bin its
own value lies in, averages that local difference over the rows of the bin and accumulates the averages along the
column.  Replacing one column of a row can change only the trees that use it, so the kernel walks, per (draw, column),
the trees of that draw's use list alone (``include/pgbart_permimp.h``) -- twice, once per edge.  Per block of rows one
``pgb_predict_ale`` call into device scratch and, per column, one ``pgb_row_reduce`` with the row's bin as its group,
into partial sums that stay on the device; ``pgb_row_reduce_finish`` turns them into the mean and the variance of the
local difference per (draw, output, bin).  Nothing of size draws x rows leaves the device and no copy of ``X`` is made.

HIP backend only.  The sums are ``pgb_row_reduce``'s (fixed order) and the finish below is sequential, so no bit of a
result depends on the blocking of the rows, on the chunking of the columns, on the launch geometry or on which other
columns are asked for.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._stored import PW_BLOCK, Job, block_bytes, check_cols
from .average import check_weights, workspace_bytes
from .importance import hdi
from .summary import DEFAULT_HDI_PROB, TRANSFORMS

MAX_BINS = 1024  # PGB_ALE_MAX_BINS


def ale_edges(x, bins: int) -> np.ndarray:
    """The default bin edges of a column ``x`` ``(n,)``: of its finite values, all distinct ones when there are at
    most ``bins + 1`` of them (a categorical code column gets one bin per step between neighbouring codes), otherwise
    the distinct values of the ``bins + 1`` empirical quantiles at ``linspace(0, 1, bins + 1)``
    (``method="inverted_cdf"``: every edge is a value of the column).  Ascending; fewer than 2 edges when the column
    has fewer than 2 distinct finite values."""
    bins = check_bins(bins)
    v = np.asarray(x, dtype=np.float64).ravel()
    v = np.sort(v[np.isfinite(v)])  # (one sort serves both the distinct values and the quantiles)
    if v.size == 0:
        return v
    first = np.concatenate([[True], v[1:] != v[:-1]])
    if int(first.sum()) <= bins + 1:
        return v[first]
    return np.unique(np.quantile(v, np.linspace(0.0, 1.0, bins + 1), method="inverted_cdf"))


def check_bins(bins) -> int:
    if isinstance(bins, (bool, np.bool_)) or not isinstance(bins, (int, np.integer)) or not 1 <= int(bins) <= MAX_BINS:
        raise ValueError(f"bins must be an integer in [1, {MAX_BINS}], got {bins!r}")
    return int(bins)


def check_edges(e, col: int) -> np.ndarray:
    """The edges of one column as the header wants them: 2 to ``MAX_BINS + 1`` finite, strictly increasing values."""
    try:
        e = np.asarray(e, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"edges of column {col} must be a vector of numbers") from None
    if e.ndim != 1 or e.size < 2:
        raise ValueError(f"edges of column {col} must be a vector of at least 2 values, got shape {e.shape}")
    if e.size > MAX_BINS + 1:
        raise ValueError(f"edges of column {col}: at most {MAX_BINS + 1} edges ({MAX_BINS} bins), got {e.size}")
    if not np.all(np.isfinite(e)):
        raise ValueError(f"edges of column {col} must be finite")
    if np.any(np.diff(e) <= 0.0):
        raise ValueError(f"edges of column {col} must be strictly increasing")
    return np.ascontiguousarray(e)


def finish(mean: np.ndarray, weight: np.ndarray) -> dict:
    """The host finish of one column from the reduce's ``mean`` ``(D, K, B + 1)`` and ``weight`` ``(B + 1,)`` (the last
    group is the missing bin).  Its order is part of the definition; every sum runs over ``b`` ascending from 0.0.

    * ``LE[d, k, b]`` = ``mean``, 0.0 for a bin of weight 0;
    * ``acc[..., 0] = 0``, ``acc[..., j] = acc[..., j - 1] + LE[..., j - 1]``;
    * ``c = (sum_b W_b * ((acc_b + acc_{b + 1}) / 2)) / sum_b W_b`` over the ``B`` real bins;
    * ``ale = acc - c`` at the edges;
    * ``importance = sqrt((sum_b W_b * mid_b^2) / sum_b W_b)`` with ``mid_b = (ale_b + ale_{b + 1}) / 2``."""
    B = mean.shape[-1] - 1
    W = weight[:B]
    LE = np.where(W > 0.0, mean[..., :B], 0.0)
    acc = np.zeros(mean.shape[:-1] + (B + 1,))
    for j in range(1, B + 1):
        acc[..., j] = acc[..., j - 1] + LE[..., j - 1]
    num, total = np.zeros(mean.shape[:-1]), 0.0
    for b in range(B):
        num = num + W[b] * ((acc[..., b] + acc[..., b + 1]) / 2.0)
        total = total + W[b]
    with np.errstate(invalid="ignore", divide="ignore"):
        ale = acc - (num / total)[..., None]
        sq = np.zeros(mean.shape[:-1])
        for b in range(B):
            mid = (ale[..., b] + ale[..., b + 1]) / 2.0
            sq = sq + W[b] * (mid * mid)
        importance = np.sqrt(sq / total)
    return {"local_effect": LE, "ale": ale, "importance": importance}


class AleJob(Job):
    """One call of :func:`accumulated_local_effects`.  The arguments are taken in this order: ``X``, the draws, ``bins``,
    ``hdi_prob``, the columns, ``edges``, the weights, the history; the backend is asked for last."""

    def __init__(self, sampler, X, cols, bins, edges, weights, draws, hdi_prob):
        super().__init__(sampler)
        self.take_X(X)
        self.take_draws(draws, none="accumulated local effects need at least 1 draw")
        self.bins = check_bins(bins)
        if not 0.0 < float(hdi_prob) < 1.0:
            raise ValueError(f"hdi_prob must lie in (0, 1), got {hdi_prob!r}")
        self.hdi_prob = float(hdi_prob)
        named = cols is not None
        asked = check_cols(np.arange(self.p) if cols is None else cols, self.p)
        if np.unique(asked).size != asked.size:
            raise ValueError("cols must not name a column twice")
        if edges is None:
            edges = {}
        if not isinstance(edges, dict):
            raise ValueError("edges must be a dict {column: vector of edges}")
        given = {}
        for key, e in edges.items():
            if isinstance(key, (bool, np.bool_)) or not isinstance(key, (int, np.integer)) or int(key) not in asked.tolist():
                raise ValueError(f"edges names column {key!r}, which is not among the columns asked for")
            given[int(key)] = check_edges(e, int(key))
        kept, skipped, self.edges = [], [], []
        for c in asked.tolist():
            e = given[c] if c in given else ale_edges(self.X[:, c], self.bins)
            if e.size < 2:
                if named:
                    raise ValueError(f"column {c} has fewer than 2 distinct finite values: it has no accumulated local effect")
                skipped.append(c)
                continue
            kept.append(c)
            self.edges.append(np.ascontiguousarray(e, dtype=np.float64))
        if not kept:
            raise ValueError("no column of X has 2 distinct finite values: nothing to compute")
        self.cols, self.skipped = np.asarray(kept, np.int32), np.asarray(skipped, np.int32)
        self.q = int(self.cols.size)
        self.weights = check_weights(weights, self.n)
        if not np.sum(self.weights) > 0.0:
            raise ValueError("weights must have a positive total")
        self.take_history()
        self.G = [int(e.size) for e in self.edges]  # (B + 1 groups: the bins and the missing bin)
        self.chunk = self.columns_per_chunk()

    # ------------------------------------------------------------------ sizes
    def fixed_bytes(self) -> int:
        """Device bytes that do not grow with the columns of a chunk: 64 rows of ``X`` and of the weight."""
        return 64 * self.row_bytes(0)

    def row_bytes(self, qc: int) -> int:
        """Device bytes one row of a block costs with ``qc`` columns in the chunk: its covariates, its weight, and per
        column its ``D K`` local differences and its bin."""
        return 8 * self.p + 8 + qc * (8 * self.K * self.D + 4)

    def column_bytes(self) -> int:
        """Device bytes one more column of a chunk costs at most: its scratch of a 64-row block, its edges and its
        partial sums (those of the column with the most bins)."""
        return 64 * (8 * self.K * self.D + 4) + 8 * max(self.G) + workspace_bytes(self.D, self.K, max(self.G), False)

    def reserved(self, cols: range) -> int:
        """What the columns ``cols`` of a chunk hold across all blocks of rows: their partial sums."""
        return sum(workspace_bytes(self.D, self.K, self.G[s], False) for s in cols)

    def columns_per_chunk(self) -> int:
        limit = block_bytes(*PW_BLOCK)
        qc = min(self.q, (limit - self.fixed_bytes()) // self.column_bytes())
        if qc < 1:
            raise ValueError(f"one column of {self.D} draws x {max(self.G) - 1} bins does not fit a block ({limit} bytes, "
                             f"{PW_BLOCK[0]}): use fewer draws or bins")
        return int(qc)

    # ------------------------------------------------------------------ the run
    def run(self) -> dict:
        be = self.hip_backend("accumulated local effects run")
        lib, mem = be.lib, be.mem
        ale_call = lib.predict_ale_entry_point()
        reduce_, finish_, _ = lib.rowreduce_entry_points()
        D, K = self.D, self.K
        carr = self.pool.as_c()
        picks = np.arange(D, dtype=np.int32)
        identity = TRANSFORMS["identity"]
        means, vars_, bin_weight, nonfinite = [], [], [], 0
        for c0 in range(0, self.q, self.chunk):
            slots = range(c0, min(self.q, c0 + self.chunk))
            cols = np.ascontiguousarray(self.cols[c0:c0 + self.chunk])
            qc = int(cols.size)
            edges = np.ascontiguousarray(np.concatenate([self.edges[s] for s in slots]))
            edge_off = np.concatenate([[0], np.cumsum([self.G[s] for s in slots])]).astype(np.int32)
            ws = [mem.empty((workspace_bytes(D, K, self.G[s], False) // 8,), np.float64) for s in slots]
            for blk in self.blocks(be, self.row_bytes(qc), reserved=self.reserved(slots)):
                r0, nb = blk.r0, blk.nb
                wd = mem.from_host(self.weights[r0:blk.r1])
                sd, bd = mem.empty((qc * D * K * nb,), np.float64), mem.empty((qc * nb,), np.int32)
                rc = ale_call(C.byref(carr), self.fidx.ctypes.data, D, self.m, mem.ptr(blk.xd), nb, self.p, self.p,
                              cols.ctypes.data, qc, edges.ctypes.data, edge_off.ctypes.data, picks.ctypes.data, D, mem.ptr(sd),
                              mem.ptr(bd), mem.stream_ptr)
                lib.check(rc, "pgb_predict_ale")
                for j, s in enumerate(slots):  # slab j is a [D][K][nb] matrix, row j of the bins its group vector
                    slab, grp = sd[j * D * K * nb:(j + 1) * D * K * nb], bd[j * nb:(j + 1) * nb]
                    rc = reduce_(mem.ptr(slab), None, D, K, nb, nb, mem.ptr(wd), mem.ptr(grp), None, None, None, None,
                                 self.G[s], identity, r0, int(r0 == 0), mem.ptr(ws[j]), None, mem.stream_ptr)
                    lib.check(rc, "pgb_row_reduce")
            for j, s in enumerate(slots):
                G = self.G[s]
                od, wod = mem.empty((2 * D * K * G,), np.float64), mem.empty((G,), np.float64)
                counts = (C.c_int64 * 2)()
                rc = finish_(mem.ptr(ws[j]), D, K, G, 0, None, mem.ptr(od), mem.ptr(wod), counts, mem.stream_ptr)
                lib.check(rc, "pgb_row_reduce_finish")
                nonfinite += int(counts[0])
                got = mem.to_host(od).reshape(2, D, K, G)
                means.append(got[0])
                vars_.append(got[1])
                bin_weight.append(mem.to_host(wod))
        return self.results(means, vars_, bin_weight, nonfinite)

    def results(self, means: list, vars_: list, bin_weight: list, nonfinite: int) -> dict:
        D, K, q = self.D, self.K, self.q
        res = {"cols": self.cols.copy(), "skipped": self.skipped.copy(), "edges": [e.copy() for e in self.edges],
               "n_draws": D, "n_nonfinite": nonfinite,
               "n_missing": np.asarray([int(np.isnan(self.X[:, c]).sum()) for c in self.cols], np.int64)}
        lists = {key: [] for key in ("ale", "mean", "sd", "hdi", "local_effect", "local_var", "bin_weight")}
        importance = np.empty((D, K, q))
        for s in range(q):
            B = self.G[s] - 1
            fin = finish(means[s], bin_weight[s])
            ale = fin["ale"]
            importance[:, :, s] = fin["importance"]
            lo_hi = np.empty((K, B + 1, 2))
            for k in range(K):
                for j in range(B + 1):
                    lo_hi[k, j] = hdi(ale[:, k, j], self.hdi_prob)
            for key, a in (("ale", ale), ("mean", ale.mean(axis=0)), ("sd", ale.std(axis=0)), ("hdi", lo_hi),
                           ("local_effect", fin["local_effect"]), ("local_var", np.ascontiguousarray(vars_[s][..., :B]))):
                lists[key].append(a)
            lists["bin_weight"].append(bin_weight[s][:B].copy())
        imp_hdi = np.empty((K, q, 2))
        for k in range(K):
            for s in range(q):
                imp_hdi[k, s] = hdi(importance[:, k, s], self.hdi_prob)
        res.update(lists)
        res.update({"importance": importance, "importance_mean": importance.mean(axis=0), "importance_hdi": imp_hdi})
        if K == 1:  # (the K axis is dropped for one output)
            for key in ("ale", "local_effect", "local_var"):
                res[key] = [a[:, 0] for a in res[key]]
            for key in ("mean", "sd", "hdi"):
                res[key] = [a[0] for a in res[key]]
            res["importance"] = res["importance"][:, 0]
            res["importance_mean"], res["importance_hdi"] = res["importance_mean"][0], res["importance_hdi"][0]
        return res


def accumulated_local_effects(sampler, X, cols=None, bins: int = 40, edges=None, weights=None, draws=None,
                              hdi_prob: float = DEFAULT_HDI_PROB) -> dict:
    """Accumulated local effects of the columns ``cols`` of ``X`` (default: all that vary) per stored draw, on the
    device.

    A column's edges ``e[0] < ... < e[B]`` are :func:`ale_edges` of it with ``bins`` (at most 1024), or ``edges[c]`` for
    the columns the dict ``edges`` names.  Bin ``b`` is ``(e[b], e[b + 1]]``; bin 0 also takes everything below ``e[0]``
    and bin ``B - 1`` everything above ``e[B]`` (the infinities too); a NaN lies in no bin.  The local difference of a
    row is the draw's prediction with the column set to the upper edge of the row's bin minus that with the lower
    edge, every other column as the row holds it (a NaN there is marginalised as always); a row with a NaN in the
    column contributes nothing.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns (several chains are
    one pool).  ``weights`` ``(n_rows,)``, finite and >= 0 with a positive total (default: ones); ``draws``: indexes of
    the stored draws (default: all).  A column with fewer than 2 distinct finite values has no ALE: named in ``cols`` it
    is refused, with ``cols=None`` it is left out and listed under ``skipped``.

    Returns lists over the columns kept (``B`` differs per column) -- the K axis is dropped for a fit with one output:
    ``ale`` ``(D, K, B + 1)``, the centred curve at the edges per draw (:func:`finish` states the formula), with
    ``mean``, ``sd`` ``(K, B + 1)`` and ``hdi`` ``(K, B + 1, 2)`` over the draws; ``local_effect`` ``(D, K, B)``, the
    weighted mean of the local difference over the rows of a bin (0.0 for a bin of weight 0, which only edges of
    your own can produce); ``local_var`` ``(D, K, B)``, its weighted variance across the rows of the bin -- zero for a
    column the model treats additively, hence a cheap interaction signal (NaN for a bin of weight 0); ``bin_weight``
    ``(B,)``; ``edges``.  And arrays: ``cols``, ``skipped``, ``n_missing`` ``(q,)`` (rows with a NaN in the column),
    ``importance`` ``(D, K, q)``, the weighted root mean square of the centred curve at the bins' midpoints, with
    ``importance_mean`` ``(K, q)`` and ``importance_hdi`` ``(K, q, 2)``; ``n_draws`` and ``n_nonfinite`` (local
    differences that were an infinity or a NaN; they are added all the same).

    Rows are processed in blocks and, where the scratch of a 64-row block or the partial sums of all columns exceed
    ``PGB_PW_BLOCK_BYTES``, columns in chunks; a single column that does not fit is refused.  No bit of a result
    depends on either."""
    return AleJob(sampler, X, cols, bins, edges, weights, draws, hdi_prob).run()
