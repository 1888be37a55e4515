"""How well a Bernoulli forest separates the classes, per posterior draw, on the device (``pgb_rank_keys``,
``pgb_rank_metrics``; ``include/pgbart_rank.h``): the ROC AUC, the two-sample Kolmogorov-Smirnov distance between the
scores of the two classes, and the true / false positive counts at given thresholds -- each with a posterior, each by
subgroup.  ``bayes_r2`` (the Brier score) and ``predictive_scores`` (the CRPS) measure calibration and sharpness; this
module measures discrimination.

A rank couples the rows inside every draw, as the argmax couples the arms in ``optimal_arm``: it is the transpose of
``posterior_summary``, order statistics over the ROWS, per draw.  The rows are laid out as 2 G segments (group, class);
per block of rows one ``pgb_predict`` writes the predictions of a chunk of draws into device scratch and one
``pgb_rank_keys`` turns them into order keys at their place in the layout; per chunk one ``pgb_rank_metrics`` sorts
every segment (the library's segmented radix sort) and counts.  Nothing of size draws x rows reaches the host.

EVERY RESULT IS AN INTEGER -- ``U2``, a count of (positive, negative) pairs, ``KSN``, ``tp``, ``fp`` -- so no bit
depends on the chunking of the draws, the blocking of the rows or the launch geometry, and the ratios returned are
divisions of exactly representable integers.

* :func:`discrimination` -- from a fit and ``X``.
* :func:`discrimination_matrix` -- from a ``(D, n)`` host matrix of scores.

HIP backend only.  Out of scope: observation weights (the sums would be floating-point and need a lane-sum convention
of their own), average precision / PR-AUC (a float sum over tie groups), gains, lift and Qini curves, Harrell's C for
censored times, and one-vs-rest AUC for fits with several outputs.  The segment layout and the sorted keys this module
leaves on the device are what any of them would build on.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._stored import PW_BLOCK, Job, block_bytes, row_blocks
from .average import check_groups
from .decision import with_draw_stats
from .summary import DEFAULT_HDI_PROB, TRANSFORMS

MAX_GROUPS = 256      # PGB_RANK_MAX_GROUPS (include/pgbart_rank.h)
MAX_THRESHOLDS = 64   # PGB_RANK_MAX_THRESHOLDS
MAX_KEYS = (1 << 31) - 1  # D x n of one pgb_rank_metrics call


def check_classes(y, n: int) -> np.ndarray:
    """``y`` as the class of every row: ``(n,)``, every value 0 or 1 -> int32."""
    try:
        y = np.asarray(y, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("y must hold 0 or 1 for every row of X") from None
    if y.shape != (n,):
        raise ValueError(f"y must hold one value per row: shape ({n},), got {y.shape}")
    if not np.all((y == 0.0) | (y == 1.0)):
        raise ValueError("y must hold 0 or 1 for every row (a NaN, a probability or another label is refused)")
    return y.astype(np.int32)


def check_thresholds(thresholds) -> np.ndarray:
    """The thresholds on the scale of the scores: at most 64, none NaN (the infinities are allowed)."""
    thr = np.asarray([] if thresholds is None else thresholds, dtype=np.float64)
    thr = thr.reshape(1) if thr.ndim == 0 else thr
    if thr.ndim != 1:
        raise ValueError(f"thresholds must be a vector, got shape {thr.shape}")
    if thr.size > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} thresholds per call, got {thr.size}")
    if np.any(np.isnan(thr)):
        raise ValueError("thresholds must not hold a NaN")
    return np.ascontiguousarray(thr)


class Layout:
    """The rows of a call as 2 G segments, ``s = 2 g + c``: ``seg_off`` ``(2 G + 1,)``, ``dest`` ``(n,)`` -- the rows of a
    segment in ascending row order, the segments in ascending ``s`` -- the labels and the class sizes of the groups."""

    def __init__(self, y, groups, n: int):
        if n < 2:
            raise ValueError(f"discrimination needs at least 2 rows, got {n}")
        cls = check_classes(y, n)
        self.labels, gid, _ = check_groups(groups, n, np.ones(n))
        self.G = G = int(self.labels.size)
        if G > MAX_GROUPS:
            raise ValueError(f"at most {MAX_GROUPS} groups per call, got {G}")
        s = 2 * gid.astype(np.int64) + cls
        sizes = np.bincount(s, minlength=2 * G)
        if np.any(sizes == 0):
            empty = int(np.argmin(sizes != 0))
            raise ValueError(f"group {self.labels[empty // 2].item()!r} holds no row with y == {empty % 2}: every group "
                             "must hold both classes")
        self.n_neg, self.n_pos = sizes[0::2].astype(np.int64), sizes[1::2].astype(np.int64)
        if np.any(self.n_pos.astype(object) * self.n_neg.astype(object) >= 1 << 52):
            raise ValueError("n_pos x n_neg of a group must be < 2^52")
        self.seg_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]), dtype=np.int64)
        order = np.argsort(s, kind="stable")
        self.dest = np.empty(n, np.int64)
        self.dest[order] = np.arange(n, dtype=np.int64)
        self.n = n


def pick_backend(given, hook=None):
    """The backend of the call: the one given, the sampler's, or the default one."""
    if given is not None:
        return given
    if hook is not None:
        return hook()
    from .sampler import default_backend

    return default_backend()


class RankRun:
    """The part of a call the two public functions share: the chunking of the draws, the calls of a chunk and the
    results.  ``row_bytes(dc)``: the device bytes one row of a row block costs with ``dc`` draws in the chunk."""

    code = TRANSFORMS["identity"]   # (discrimination sets its transform)

    def __init__(self, be, layout: Layout, thr: np.ndarray, D: int, hdi_prob: float = DEFAULT_HDI_PROB):
        self.be, self.lay, self.thr, self.D, self.hdi_prob = be, layout, thr, int(D), hdi_prob
        self.T = int(thr.size)
        self.n_out = 2 + 2 * self.T
        self.keys_fn, self.ws_query, self.metrics_fn = be.lib.rank_entry_points()   # (the oracle: NotImplementedError)

    def ws_bytes(self, dc: int) -> int:
        b = int(self.ws_query(dc, self.lay.n, self.lay.G))
        if b <= 0:
            raise ValueError(f"pgb_rank_workspace_bytes({dc}, {self.lay.n}, {self.lay.G}) refused the sizes")
        return b

    def reserved(self, dc: int) -> int:
        """Device bytes a chunk of ``dc`` draws holds across all its row blocks: the keys twice, the sort's storage,
        the counters, the layout and the results."""
        lay = self.lay
        return 8 * dc * lay.n + self.ws_bytes(dc) + 16 + 8 * (2 * lay.G + 1 + self.T) + 4 * (2 * lay.G * dc + 1) + 256 \
            + 8 * dc * lay.G * self.n_out

    def chunk_draws(self, row_bytes) -> int:
        """The draws per chunk: the chunk and one minimal row block must fit ``PGB_PW_BLOCK_BYTES`` (a call whose single
        draw does not is refused); within that, see below."""
        n, limit = self.lay.n, block_bytes(*PW_BLOCK)
        fits = lambda dc: self.reserved(dc) + min(n, 64) * row_bytes(dc) <= limit  # noqa: E731
        hi = min(self.D, MAX_KEYS // n)
        if hi < 1:
            raise ValueError(f"{n} rows are more than one call can rank ({MAX_KEYS} keys)")
        if not fits(1):
            raise ValueError(f"not even one draw of {n} rows fits a block: its keys, the sort's storage and a block of rows take "
                             f"{self.reserved(1) + min(n, 64) * row_bytes(1)} bytes, more than {PW_BLOCK[0]} = {limit} allows")
        # Not the largest chunk that fits: it would leave the row blocks their minimum of 64 rows, one pgb_predict each
        # (measured at 100 k rows x 1000 draws: 1565 blocks, 2.2 s per call instead of 0.4 s).  A chunk takes at most
        # half of what a block may take -- the other half is the row block's -- unless a single draw needs more; the
        # chunks are then made equal.
        half = lambda dc: self.reserved(dc) <= limit // 2  # noqa: E731
        lo = 1
        while lo < hi:   # (the bytes grow with dc: bisect for the largest that fits)
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if half(mid) else (lo, mid - 1)
        while lo > 1 and not fits(lo):   # (a wide X under a small knob: the minimal row block is what does not fit)
            lo -= 1
        n_chunks = -(-self.D // lo)
        return -(-self.D // n_chunks)

    def run(self, row_bytes, fill) -> dict:
        """``fill(c0, c1, put, reserved)`` walks the row blocks of the draws ``c0 .. c1`` and calls ``put(a_dev, nb, ld,
        off_dev, r0, r1)`` for each."""
        be, lay, D, T = self.be, self.lay, self.D, self.T
        lib, mem = be.lib, be.mem
        n, G = lay.n, lay.G
        Dc = self.chunk_draws(row_bytes)
        out = np.empty((D, G, self.n_out), np.int64)
        n_nan = 0
        self.chunks = []
        for c0 in range(0, D, Dc):
            c1 = min(D, c0 + Dc)
            dc = c1 - c0
            keys, ws = mem.empty((dc * n,), np.float64), mem.empty((self.ws_bytes(dc) // 8 + 1,), np.float64)
            cnt = mem.from_host(np.zeros(2, np.int64))

            def put(a_dev, nb, ld, off_dev, r0, r1, dc=dc, keys=keys, cnt=cnt):
                dd = mem.from_host(lay.dest[r0:r1])
                rc = self.keys_fn(mem.ptr(a_dev), dc, nb, ld, None if off_dev is None else mem.ptr(off_dev), self.code,
                                  mem.ptr(dd), n, mem.ptr(keys), mem.ptr(cnt), mem.stream_ptr)
                lib.check(rc, "pgb_rank_keys")

            fill(c0, c1, put, self.reserved(dc))
            got, counts = np.empty((dc, G, self.n_out), np.int64), (C.c_int64 * 2)()
            rc = self.metrics_fn(mem.ptr(keys), mem.ptr(ws), dc, n, lay.seg_off.ctypes.data, G,
                                 self.thr.ctypes.data if T else None, T, mem.ptr(cnt), got.ctypes.data, counts, mem.stream_ptr)
            lib.check(rc, "pgb_rank_metrics")
            out[c0:c1] = got
            n_nan += int(counts[0])
            self.chunks.append((c0, c1))
        if n_nan > 0:
            raise ValueError(f"{n_nan} of the {D * n} scores are NaN: the AUC of NaN scores is undefined")
        return self.result(out)

    def result(self, out: np.ndarray) -> dict:
        lay, T = self.lay, self.T
        n1, n0 = lay.n_pos.astype(np.float64), lay.n_neg.astype(np.float64)
        U2, KSN = out[:, :, 0].copy(), out[:, :, 1].copy()
        res = {"group_labels": lay.labels.copy(), "n_pos": lay.n_pos.copy(), "n_neg": lay.n_neg.copy(), "n_draws": self.D,
               "U2": U2, "KSN": KSN}
        per_draw = {"auc": U2 / (2.0 * n1 * n0), "ks": KSN / (n1 * n0)}   # (integers below 2^53: one rounding each)
        with_draw_stats(res, per_draw, self.hdi_prob)
        for key in per_draw:
            res[key + "_hdi"] = np.ascontiguousarray(res[key + "_hdi"].T)   # (2, G)
        if T:
            tp, fp = out[:, :, 2:2 + T].copy(), out[:, :, 2 + T:].copy()
            with np.errstate(invalid="ignore", divide="ignore"):
                precision = np.where(tp + fp == 0, np.nan, tp / np.maximum(tp + fp, 1).astype(np.float64))
            res.update({"thresholds": self.thr.copy(), "tp": tp, "fp": fp, "tpr": tp / n1[None, :, None],
                        "fpr": fp / n0[None, :, None], "precision": precision})
        return res


def discrimination(sampler, X, y, groups=None, thresholds=None, transform: str = "identity", offset=None, excluded=None,
                   draws=None, backend=None) -> dict:
    """ROC AUC, KS distance and threshold counts of every stored draw at the rows of ``X`` against the classes ``y``,
    by group, computed on the device.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns (several chains are
    one pool); a fit with one output.  ``X``: a host matrix ``(n, p)``, n >= 2 (a device-resident ``X`` is refused).
    ``y``: ``(n,)``, every value 0 or 1.  ``groups``: ``(n,)`` labels as in ``average_prediction`` (default: one group);
    at most 256, and every group must hold both classes.  The score of a row in a draw is ``T(f_d(x_i) + offset_i)`` with
    the ``transform``, ``offset`` and ``excluded`` of ``posterior_summary``; a monotone transform changes no rank, it
    sets the scale of ``thresholds``: at most 64 values on the scale of the score, none NaN; a row is called positive
    iff its score is >= the threshold (the rule of scikit-learn's ``roc_curve``).  ``draws``: indexes of the stored
    draws (default: all).

    Returns, per draw: ``auc`` and ``ks`` ``(D, G)`` -- ties count one half in the AUC; ``ks`` is the largest distance
    between the empirical distribution functions of the scores of the two classes -- each with ``_mean``, ``_sd``
    ``(G,)`` and ``_hdi`` ``(2, G)`` over the draws; with thresholds ``tp``, ``fp`` (int64), ``tpr``, ``fpr`` and
    ``precision`` ``(D, G, T)``, precision NaN where ``tp + fp == 0``.  And ``group_labels``, ``n_pos``, ``n_neg``
    ``(G,)``, ``n_draws``, and the integers themselves: ``U2`` (``auc = U2 / (2 n_pos n_neg)``) and ``KSN``
    (``ks = KSN / (n_pos n_neg)``), ``(D, G)`` int64.  A score that is a NaN is an error.

    The outer loop runs over chunks of draws, the inner one over blocks of rows: a chunk holds its keys twice and the
    sort's storage across all its row blocks.  That and one block of 64 rows must fit ``PGB_PW_BLOCK_BYTES``; a chunk
    takes at most half of it where more than one draw fits, so that the row blocks stay large, and the chunks are
    equal.  Every result is an integer: no bit depends on the chunking or the blocking.

    Not covered: observation weights, average precision, gains / lift / Qini curves, Harrell's C, one-vs-rest AUC of
    fits with several outputs (module docstring)."""
    if not isinstance(X, np.ndarray) and (hasattr(X, "data_ptr") or hasattr(X, "__cuda_array_interface__")):
        raise ValueError("X must be a host matrix: discrimination does not take a device-resident X (resident_rows)")
    job = Job(sampler)
    job.take_X(X)
    job.take_offset(offset)
    job.take_excluded(excluded)
    job.take_draws(draws, none="discrimination needs at least 1 draw")
    job.take_history()
    if job.K != 1:
        raise ValueError(f"discrimination takes a fit with one output, this one has {job.K}")
    if transform not in TRANSFORMS:
        raise ValueError(f"unknown transform {transform!r}: use one of {', '.join(TRANSFORMS)}")
    layout = Layout(y, groups, job.n)
    thr = check_thresholds(thresholds)
    be = pick_backend(backend, job.backend)
    run = RankRun(be, layout, thr, job.D)
    run.code = TRANSFORMS[transform]
    lib, mem, excl, carr = be.lib, be.mem, job.excluded, job.pool.as_c()

    def row_bytes(dc: int) -> int:   # the covariates, the chunk's predictions, dest, the offset
        return 8 * job.p + 8 * dc + 8 + 8 * (job.offset is not None)

    def fill(c0, c1, put, reserved):
        dc = c1 - c0
        fidx = np.ascontiguousarray(job.fidx[c0:c1])
        for blk in job.blocks(be, row_bytes(dc), reserved=reserved):
            md = mem.empty((dc * blk.nb,), np.float64)
            rc = lib.lib.pgb_predict(C.byref(carr), fidx.ctypes.data, dc, job.m, mem.ptr(blk.xd), blk.nb, job.p, job.p,
                                     excl.ctypes.data if excl.size else None, int(excl.size), mem.ptr(md), mem.stream_ptr)
            lib.check(rc, "pgb_predict")
            put(md, blk.nb, blk.nb, blk.od, blk.r0, blk.r1)

    res = run.run(row_bytes, fill)
    res["n_chunks"] = len(run.chunks)
    return res


def discrimination_matrix(scores, y, groups=None, thresholds=None, backend=None) -> dict:
    """:func:`discrimination` of a host matrix ``scores`` ``(D, n)`` -- one row of scores per draw; a vector is one
    draw -- against ``y``: the same results, transform identity, no tree walk.  The matrix is uploaded by chunks of
    draws and blocks of rows.  ``discrimination_matrix(posterior_summary(ps, X, transform="probit")["mean"][None, :],
    y)["auc"]`` is the AUC of the posterior mean, the one number ``sklearn.metrics.roc_auc_score(y, p_mean)`` gives."""
    try:
        scores = np.asarray(scores, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("scores must be a matrix of numbers (n_draws, n_rows)") from None
    if scores.ndim == 1:
        scores = scores[None, :]
    if scores.ndim != 2 or scores.shape[0] < 1:
        raise ValueError(f"scores must be a matrix (n_draws, n_rows) with at least 1 draw, got shape {scores.shape}")
    D, n = (int(v) for v in scores.shape)
    layout = Layout(y, groups, n)
    thr = check_thresholds(thresholds)
    be = pick_backend(backend)
    run = RankRun(be, layout, thr, D)
    mem = be.mem

    def row_bytes(dc: int) -> int:
        return 8 * dc + 8

    def fill(c0, c1, put, reserved):
        for r0, r1 in row_blocks(n, row_bytes(c1 - c0), block_bytes(*PW_BLOCK) - int(reserved)):
            put(mem.from_host(np.ascontiguousarray(scores[c0:c1, r0:r1])), r1 - r0, r1 - r0, None, r0, r1)

    res = run.run(row_bytes, fill)
    res["n_chunks"] = len(run.chunks)
    return res
