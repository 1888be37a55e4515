"""The partition a fit puts on the rows: leaf ids, posterior proximity and nearest rows on the device
(``pgb_predict_leaf_codes``, ``pgb_prox_count``, ``pgb_prox_topk``; ``include/pgbart_proximity.h``).

Every other consumer of the stored draws reduces the leaf VALUES a row reaches.  Two rows are close, in the metric the
model learned, when they stop at the same node in many trees of many draws: that shared-leaf fraction is BART's
posterior proximity, the random-forest proximity averaged over the posterior.

* :func:`leaf_ids` -- the node where every row stops in every tree of every draw (sklearn's ``apply``, XGBoost's
  ``pred_leaf``), one byte each.
* :func:`proximity` -- the matrix of shared-leaf counts of query rows against reference rows.
* :func:`nearest_rows` -- the ``k`` reference rows nearest to every query row, and the query's mean similarity to all of
  them (a low value: a row far from everything in ``X_ref``); the ``(q, n)`` matrix never leaves the device.

HIP backend only; host matrices only.  Everything is an integer: no result depends on the blocking.  The reference rows
are processed in blocks (``PGB_PW_BLOCK_BYTES``, at least 64 rows) and the draws in chunks when the codes of all
``T = draws x m`` slots of a block do not fit (at least one draw); the query rows are not blocked -- a block holds their
codes of one chunk of draws and its ``q x rows`` distances.  With ``excluded`` columns a row stops at the first split on
one of them: the proximity in the subspace without those columns.  A row with a missing value stops at the split that
asks for it, and is close only to rows that stop at the same node.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._stored import PW_BLOCK, Job, block_bytes, check_X

MAX_K = 128                 # PGB_PROX_MAX_K (include/pgbart_proximity.h)
MAX_SLOTS = (1 << 31) - 1   # PGB_PROX_MAX_SLOTS
PAD = 0xFF                  # PGB_PROX_PAD


def words(n_slots: int) -> int:
    """``pgb_prox_words``: four slots to a word."""
    return (int(n_slots) + 3) // 4


def unpack_codes(code_words: np.ndarray, n_draws: int, m: int) -> np.ndarray:
    """The code matrix ``uint32 (W, nb)`` of ``n_draws * m`` slots as ``uint8 (n_draws, m, nb)``: slot ``4 w + b`` is
    byte ``b`` of word ``w`` (bits ``8 b .. 8 b + 7``)."""
    w = np.ascontiguousarray(code_words, dtype="<u4")
    W, nb = w.shape
    by = w.view(np.uint8).reshape(W, nb, 4).transpose(0, 2, 1).reshape(4 * W, nb)
    return np.ascontiguousarray(by[:n_draws * m].reshape(n_draws, m, nb))


def topk_workspace_bytes(q: int, k: int) -> int:
    """``pgb_prox_topk_workspace_bytes``: ``keys[q][k]`` then ``sum[q]``, 8 bytes each."""
    return 8 * (q * k + q)


class ProximityJob(Job):
    """One call of this module.  The job's rows -- the ones :meth:`Job.blocks` cuts into blocks -- are the REFERENCE rows;
    the query rows are ``Q``.  The arguments are taken in this order: ``X``, ``X_ref``, ``k`` and ``exclude_self``,
    ``excluded``, the draws, the number of slots, the history."""

    def __init__(self, sampler, X, X_ref=None, draws=None, excluded=None, k=None, exclude_self=False, what="the proximity"):
        super().__init__(sampler)
        self.Q = check_X(X)
        self.q = int(self.Q.shape[0])
        if X_ref is None:
            self.take_X(self.Q)
        else:
            self.take_X(X_ref)
            if self.p != int(self.Q.shape[1]):
                raise ValueError(f"X_ref must have the {int(self.Q.shape[1])} columns of X, got shape {self.X.shape}")
        self.exclude_self = bool(exclude_self)
        if self.exclude_self and X_ref is not None:
            raise ValueError("exclude_self leaves a row of X out of its own neighbours: it takes no X_ref")
        self.k = None
        if k is not None:
            self.k = int(k)
            if not 1 <= self.k <= MAX_K:
                raise ValueError(f"k must be in [1, {MAX_K}], got {k!r}")
            avail = self.n - int(self.exclude_self)
            if self.k > avail:
                raise ValueError(f"k = {self.k} neighbours of {avail} reference rows" + (" (the row itself left out)" if self.exclude_self else ""))
        self.take_excluded(excluded)
        self.take_draws(draws, none=f"{what} needs at least 1 draw")
        self.T = self.D * self.m
        if self.T > MAX_SLOTS:
            raise ValueError(f"{self.D} draws x {self.m} trees are {self.T} slots, more than {MAX_SLOTS}: use fewer draws")
        self.take_history()

    # ---------------------------------------------------------------------------------------------------- blocking
    def draw_chunks(self, rows_held: int) -> list:
        """The chunks ``[(d0, d1)]`` of the draw list: as many draws as let the codes of ``rows_held + 64`` rows take
        half of what a block may take, at least one."""
        fit = (block_bytes(*PW_BLOCK) // 2) // (4 * (rows_held + 64))
        step = max(1, min(self.D, 4 * fit // self.m))
        return [(d0, min(self.D, d0 + step)) for d0 in range(0, self.D, step)]

    def codes(self, be, entry, xd, nb: int, d0: int, d1: int):
        """``pgb_predict_leaf_codes`` of the draws ``d0 .. d1`` of the job at the ``nb`` device rows ``xd`` -> the device
        words ``[W][nb]``."""
        lib, mem, excl = be.lib, be.mem, self.excluded
        cd = mem.empty((words((d1 - d0) * self.m) * nb,), np.int32)
        fidx = np.ascontiguousarray(self.fidx[d0:d1])
        carr = self.pool.as_c()
        rc = entry(C.byref(carr), fidx.ctypes.data, d1 - d0, self.m, mem.ptr(xd), nb, self.p, self.p,
                   excl.ctypes.data if excl.size else None, int(excl.size), mem.ptr(cd), nb, mem.stream_ptr)
        lib.check(rc, "pgb_predict_leaf_codes")
        return cd

    # ------------------------------------------------------------------------------------------------------- calls
    def leaf_ids(self) -> np.ndarray:
        be = self.hip_backend("leaf ids run")
        entry = be.lib.proximity_entry_points()[0]
        chunks = self.draw_chunks(0)
        out = np.empty((self.D, self.m, self.n), np.uint8)
        wc = words((chunks[0][1] - chunks[0][0]) * self.m)
        for blk in self.blocks(be, 8 * self.p + 4 * wc):
            for d0, d1 in chunks:
                cw = be.mem.to_host(self.codes(be, entry, blk.xd, blk.nb, d0, d1)).view(np.uint32).reshape(-1, blk.nb)
                out[d0:d1, :, blk.r0:blk.r1] = unpack_codes(cw, d1 - d0, self.m)
        return out

    def distances(self, be, on_block):
        """The driver of :func:`proximity` and :func:`nearest_rows`: per block of reference rows the device distances
        ``uint32 [q][nb]`` of all draws, handed to ``on_block(blk, dist)``."""
        lib, mem = be.lib, be.mem
        codes_, count, _, _ = lib.proximity_entry_points()
        q, chunks = self.q, self.draw_chunks(self.q)
        wc = words((chunks[0][1] - chunks[0][0]) * self.m)
        qd = mem.from_host(self.Q)
        # one chunk: the query codes are made once and kept across the reference blocks
        kept = self.codes(be, codes_, qd, q, *chunks[0]) if len(chunks) == 1 else None
        reserved = 8 * self.p * q + 4 * wc * q + (topk_workspace_bytes(q, self.k) if self.k else 0)
        for blk in self.blocks(be, 8 * self.p + 4 * wc + 4 * q, reserved=reserved):
            nb = blk.nb
            dist = mem.empty((q * nb,), np.int32)
            for ci, (d0, d1) in enumerate(chunks):
                cq = kept if kept is not None else self.codes(be, codes_, qd, q, d0, d1)
                cr = self.codes(be, codes_, blk.xd, nb, d0, d1)
                rc = count(mem.ptr(cq), q, q, mem.ptr(cr), nb, nb, words((d1 - d0) * self.m), mem.ptr(dist), nb, int(ci == 0),
                           mem.stream_ptr)
                lib.check(rc, "pgb_prox_count")
            on_block(blk, dist)

    def proximity(self) -> dict:
        be = self.hip_backend("the proximity runs")
        matches = np.empty((self.q, self.n), np.uint32)

        def on_block(blk, dist):
            matches[:, blk.r0:blk.r1] = np.uint32(self.T) - be.mem.to_host(dist).view(np.uint32).reshape(self.q, blk.nb)

        self.distances(be, on_block)
        return {"matches": matches, "similarity": matches / float(self.T), "n_slots": self.T}

    def nearest(self) -> dict:
        be = self.hip_backend("the nearest rows run")
        lib, mem = be.lib, be.mem
        _, _, topk, query = lib.proximity_entry_points()
        q, k = self.q, self.k
        ws_bytes = topk_workspace_bytes(q, k)
        if int(query(q, k)) != ws_bytes:
            raise _abi.PGBError(f"pgb_prox_topk_workspace_bytes({q}, {k}) is not {ws_bytes}")
        ws = mem.empty((ws_bytes // 8,), np.float64)  # (8-byte words: keys[q][k], then sum[q])

        def on_block(blk, dist):
            rc = topk(mem.ptr(dist), blk.nb, q, blk.nb, blk.r0, 0 if self.exclude_self else -1, k, mem.ptr(ws), int(blk.r0 == 0),
                      mem.stream_ptr)
            lib.check(rc, "pgb_prox_topk")

        self.distances(be, on_block)
        got = mem.to_host(ws).view(np.uint64)
        keys, total = got[:q * k].reshape(q, k), got[q * k:]
        matches = (np.uint64(self.T) - (keys >> np.uint64(32))).astype(np.uint32)
        pairs = float(self.n - int(self.exclude_self)) * float(self.T)
        return {"index": (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), "matches": matches,
                "similarity": matches / float(self.T), "mean_similarity": (pairs - total.astype(np.float64)) / pairs,
                "n_slots": self.T}


def leaf_ids(sampler, X, draws=None, excluded=None) -> np.ndarray:
    """The node where every row of ``X`` stops in every tree of every draw, computed on the device: ``uint8 (D, m, n)``,
    the tree-local index of the node (0 is the root) -- sklearn's ``apply``, XGBoost's ``pred_leaf``.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns (several chains are
    one pool).  ``draws``: indexes of the stored draws (default: all).  ``excluded``: column indexes; a row stops AT a
    split on one of them, as it does at a split whose value is NaN for it -- nothing is marginalised.  Otherwise the
    row goes left exactly when ``sample_posterior``'s walk does, under all three split rules.  A history with a tree of
    more than 255 nodes is refused (the samplers build none).  Rows are processed in blocks (``PGB_PW_BLOCK_BYTES``)."""
    return ProximityJob(sampler, X, None, draws, excluded, what="leaf ids").leaf_ids()


def proximity(sampler, X, X_ref=None, draws=None, excluded=None) -> dict:
    """The posterior proximity of the rows of ``X`` to the rows of ``X_ref`` (``None``: of ``X`` to themselves): in how
    many of the ``T = D * m`` (draw, tree) slots two rows stop at the same node (:func:`leaf_ids`).

    Returns ``matches`` ``uint32 (q, n)``, ``similarity = matches / T`` ``float64 (q, n)`` and ``n_slots = T``.  The
    matrix of a set of rows against itself is symmetric with ``T`` on its diagonal.  The result is ``q x n`` on the
    host: for the neighbours of a few rows among many use :func:`nearest_rows`."""
    return ProximityJob(sampler, X, X_ref, draws, excluded).proximity()


def nearest_rows(sampler, X, X_ref=None, k: int = 10, draws=None, excluded=None, exclude_self: bool = False) -> dict:
    """The ``k`` rows of ``X_ref`` (``None``: of ``X`` itself) nearest to every row of ``X`` in the posterior proximity,
    selected on the device: the ``(q, n)`` matrix never leaves it.

    Returns ``index`` ``int64 (q, k)`` -- rows of ``X_ref``, nearest first, ties to the smaller index -- their ``matches``
    ``uint32 (q, k)`` and ``similarity`` ``(q, k)``, ``mean_similarity`` ``(q,)`` -- the mean of the similarity to ALL
    reference rows taken in: a low value is a query far from everything in ``X_ref``, to be read before its predictions
    are trusted -- and ``n_slots``.  ``exclude_self`` (only without ``X_ref``) leaves row ``i`` out of its own neighbours
    and out of its mean.  ``1 <= k <= 128``, and ``k`` at most the number of reference rows taken in."""
    return ProximityJob(sampler, X, X_ref, draws, excluded, k, exclude_self, what="nearest rows").nearest()
