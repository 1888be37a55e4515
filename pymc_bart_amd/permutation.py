"""Permutation importance of stored posterior draws on the device (``pgb_predict_permuted``,
``include/pgbart_permimp.h``): how much worse does every draw of the fit get when column ``j`` of ``X`` is scrambled?

Scrambling a column can change only the trees that use it, so the kernel walks, per (draw, column), the trees of that
draw's USE LIST alone -- once at the row, once per repeat at the row with the column's value taken from a donor row --
and adds the difference to the draw's plain prediction.  The donor of a row is a keyed bijection computed per row
(``pgb_perm_index``): nothing is sorted, no permuted copy of ``X`` exists anywhere.  Per block of rows one
``pgb_predict`` call, one ``pgb_predict_permuted`` call into device scratch and ``pgb_row_reduce`` calls that add the
block to partial sums which stay on the device; ``pgb_row_reduce_finish`` turns them into per-draw results.  Nothing of
size draws x rows leaves the device.

HIP backend only.  The sums are ``pgb_row_reduce``'s (fixed order), the permutation depends on ``(random_seed, column,
repeat, row)`` alone: no bit of a result depends on the blocking of the rows, on the chunking of the columns, on the
launch geometry or on which other columns are asked for.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._stored import PW_BLOCK, Job, block_bytes, check_cols, check_seed, check_y
from .average import check_groups, check_weights, workspace_bytes
from .importance import hdi
from .summary import DEFAULT_HDI_PROB, TRANSFORMS

PRED, DELTA = 0, 1   # PGB_PERMIMP_PRED, PGB_PERMIMP_DELTA
MAX_REPEATS = 65535  # PGB_PERMIMP_MAX_REPEATS


class PermutationJob(Job):
    """One call of :func:`permutation_importance`.  The arguments are taken in this order: ``X``, the transform, the
    offset, the draws, the history, the columns, the seed, the repeats, the weights, the groups, ``y``; the backend is
    asked for last."""

    def __init__(self, sampler, X, y, cols, n_repeats, draws, weights, groups, transform, offset, random_seed):
        super().__init__(sampler)
        self.take_X(X)
        if transform not in TRANSFORMS:
            raise ValueError(f"unknown transform {transform!r}: use one of {', '.join(TRANSFORMS)}")
        self.code = TRANSFORMS[transform]
        self.take_offset(offset)
        self.take_draws(draws, none="permutation importance needs at least 1 draw")
        self.take_history()
        self.cols = check_cols(np.arange(self.p) if cols is None else cols, self.p)
        if np.unique(self.cols).size != self.cols.size:
            raise ValueError("cols must not name a column twice")
        self.seed = check_seed(random_seed)
        self.R = int(n_repeats)
        if not 1 <= self.R <= MAX_REPEATS:
            raise ValueError(f"n_repeats must lie in [1, {MAX_REPEATS}], got {n_repeats!r}")
        self.weights = check_weights(weights, self.n)
        self.labels, self.gid, self.n_rows = check_groups(groups, self.n, self.weights)
        self.G = int(self.labels.size)
        self.grouped = groups is not None
        self.y = self.centre = None
        if y is not None:
            if self.K > 1:
                raise ValueError(f"y takes a fit with one output, this one has {self.K}")
            self.y = check_y(y, self.n)
            total = np.bincount(self.gid, weights=self.weights, minlength=self.G)  # (bayes_r2's centre: its bits)
            self.centre = np.ascontiguousarray((np.bincount(self.gid, weights=self.weights * self.y, minlength=self.G) / total)[None, :])
        else:
            if transform != "identity":
                raise ValueError(f"without y the shift of the prediction itself is measured: transform must be 'identity', got {transform!r}")
            if self.offset is not None:
                raise ValueError("without y an offset has no effect: pass offset=None")
        self.q = int(self.cols.size)
        self.chunk = self.columns_per_chunk()

    # ------------------------------------------------------------------ sizes
    def fixed_bytes(self) -> int:
        """Device bytes that do not grow with the columns of a chunk: 64 rows of ``X``, of ``f``, of the weight, the
        group, ``y`` and the offset, and the partial sums of ``f`` itself."""
        has_y = self.y is not None
        return 64 * self.row_bytes(0) + (workspace_bytes(self.D, self.K, self.G, True) if has_y else 0)

    def row_bytes(self, qc: int) -> int:
        """Device bytes one row of a block costs with ``qc`` columns in the chunk."""
        has_y = self.y is not None
        per = 8 * (self.p + self.K * self.D) + 8 + 4 + 8 * has_y + 8 * self.K * (self.offset is not None)
        return per + 8 * self.K * self.D * qc * self.R

    def column_bytes(self) -> int:
        """Device bytes one more column of a chunk costs: its column of ``X``, its scratch of a 64-row block and its
        partial sums."""
        per_ws = workspace_bytes(self.D * self.R, self.K, self.G, self.y is not None) - 8 * (self.G * 64 + 2)
        return 8 * self.n + 64 * 8 * self.K * self.D * self.R + per_ws

    def reserved(self, qc: int) -> int:
        """What a chunk of ``qc`` columns holds across all blocks of rows: its columns of ``X`` and the partial sums."""
        has_y = self.y is not None
        return 8 * self.n * qc + workspace_bytes(self.D * qc * self.R, self.K, self.G, has_y) + \
            (workspace_bytes(self.D, self.K, self.G, True) if has_y else 0)

    def columns_per_chunk(self) -> int:
        limit = block_bytes(*PW_BLOCK)
        qc = min(self.q, (limit - self.fixed_bytes() - 8 * (self.G * 64 + 2)) // self.column_bytes())
        if qc < 1:
            raise ValueError(f"one column of {self.D} draws x {self.R} repeats x {self.G} groups over {self.n} rows does not fit "
                             f"a block ({limit} bytes, {PW_BLOCK[0]}): use fewer draws, repeats or groups")
        return int(qc)

    # ------------------------------------------------------------------ the run
    def run(self) -> dict:
        be = self.hip_backend("permutation importance runs")
        lib, mem = be.lib, be.mem
        permuted = lib.predict_permuted_entry_point()
        reduce_, finish, _ = lib.rowreduce_entry_points()
        D, K, G, R, n, has_y = self.D, self.K, self.G, self.R, self.n, self.y is not None
        ptr = lambda buf: None if buf is None else mem.ptr(buf)  # noqa: E731
        cd = None if self.centre is None else mem.from_host(self.centre)
        carr = self.pool.as_c()
        picks = np.arange(D, dtype=np.int32)
        n_out = 6 if has_y else 2
        base, parts, nonfinite, weight = None, [], 0, None
        for c0 in range(0, self.q, self.chunk):
            cols = np.ascontiguousarray(self.cols[c0:c0 + self.chunk])
            qc, first = int(cols.size), c0 == 0
            Dp = D * qc * R
            xcols = mem.from_host(np.ascontiguousarray(self.X[:, cols].T))
            ws = mem.empty((workspace_bytes(Dp, K, G, has_y) // 8,), np.float64)
            ws0 = mem.empty((workspace_bytes(D, K, G, True) // 8,), np.float64) if has_y and first else None
            for blk in self.blocks(be, self.row_bytes(qc), y=has_y, predict=has_y, reserved=self.reserved(qc)):
                r0, nb = blk.r0, blk.nb
                wd, gd = mem.from_host(self.weights[r0:blk.r1]), mem.from_host(self.gid[r0:blk.r1])
                sd = mem.empty((Dp * K * nb,), np.float64)
                rc = permuted(C.byref(carr), self.fidx.ctypes.data, D, self.m, mem.ptr(blk.xd), nb, self.p, self.p,
                              mem.ptr(xcols), n, r0, cols.ctypes.data, qc, R, self.seed, picks.ctypes.data, D, ptr(blk.md),
                              PRED if has_y else DELTA, mem.ptr(sd), mem.stream_ptr)
                lib.check(rc, "pgb_predict_permuted")
                if ws0 is not None:
                    rc = reduce_(mem.ptr(blk.md), None, D, K, nb, nb, mem.ptr(wd), mem.ptr(gd), ptr(blk.yd), ptr(blk.od), None,
                                 ptr(cd), G, self.code, r0, int(r0 == 0), mem.ptr(ws0), None, mem.stream_ptr)
                    lib.check(rc, "pgb_row_reduce")
                rc = reduce_(mem.ptr(sd), None, Dp, K, nb, nb, mem.ptr(wd), mem.ptr(gd), ptr(blk.yd), ptr(blk.od), None,
                             ptr(cd), G, self.code, r0, int(r0 == 0), mem.ptr(ws), None, mem.stream_ptr)
                lib.check(rc, "pgb_row_reduce")
            for buf, dd in ((ws0, D), (ws, Dp)):
                if buf is None:
                    continue
                od, wod = mem.empty((n_out * dd * K * G,), np.float64), mem.empty((G,), np.float64)
                counts = (C.c_int64 * 2)()
                rc = finish(mem.ptr(buf), dd, K, G, int(has_y), ptr(cd), mem.ptr(od), mem.ptr(wod), counts, mem.stream_ptr)
                lib.check(rc, "pgb_row_reduce_finish")
                nonfinite += int(counts[0])
                weight = mem.to_host(wod)
                got = mem.to_host(od).reshape(n_out, dd, K, G)
                if buf is ws0:
                    base = got
                else:
                    parts.append(got.reshape(n_out, D, qc, R, K, G))
        out = np.concatenate(parts, axis=2)  # (n_out, D, q, R, K, G)
        res = {"cols": self.cols.copy(), "n_repeats": R, "n_draws": D, "n_nonfinite": nonfinite,
               "group_labels": self.labels.copy(), "weight": weight}
        if has_y:
            res.update(self.loss_results(base[:, :, 0, :], out[:, :, :, :, 0, :]))
        else:
            mean, var = out[0], out[1]                                  # (D, q, R, K, G)
            res["shift"] = np.ascontiguousarray(np.moveaxis(mean.mean(axis=2), 2, 1))            # (D, K, q, G)
            res["sensitivity"] = np.ascontiguousarray(np.moveaxis((var + mean * mean).mean(axis=2), 2, 1))
            if K == 1:
                res["shift"], res["sensitivity"] = res["shift"][:, 0], res["sensitivity"][:, 0]
        if not self.grouped:
            for key in ("mse_permuted", "mse_base", "importance", "importance_mean", "importance_sd", "r2_drop", "shift",
                        "sensitivity"):
                if key in res:
                    res[key] = res[key][..., 0]
            if "importance_hdi" in res:
                res["importance_hdi"] = res["importance_hdi"][:, 0, :]
        return res

    def loss_results(self, base: np.ndarray, perm: np.ndarray) -> dict:
        """``base`` (6, D, G) and ``perm`` (6, D, q, R, G) of the reduce -> the results with ``y``, all with the G axis."""
        mse_base, mse_perm = base[3].copy(), perm[3].copy()
        imp = mse_perm.mean(axis=2) - mse_base[:, None, :]             # (D, q, G)
        lo_hi = np.empty((self.q, self.G, 2))
        for s in range(self.q):
            for g in range(self.G):
                lo_hi[s, g] = hdi(imp[:, s, g], DEFAULT_HDI_PROB)
        return {"mse_permuted": mse_perm, "mse_base": mse_base, "importance": imp, "importance_mean": imp.mean(axis=0),
                "importance_sd": imp.std(axis=0), "importance_hdi": lo_hi,
                "r2_drop": base[5][:, None, :] - perm[5].mean(axis=2)}


def permutation_importance(sampler, X, y=None, cols=None, n_repeats: int = 5, draws=None, weights=None, groups=None,
                           transform: str = "identity", offset=None, random_seed=0) -> dict:
    """Permutation importance of the columns ``cols`` of ``X`` (default: all) per stored draw, on the device.

    For column ``c`` and repeat ``r`` every row ``i`` takes its value of column ``c`` from the donor row
    ``pgb_perm_index(random_seed, c, r, n_rows, i)`` -- a pseudorandom bijection of the rows keyed by the column's index
    in ``X``, so a column's result never depends on which other columns are asked for.  (It is not a uniform draw from
    all permutations; below about 16 rows it cannot reach them evenly.)  A NaN donor value is marginalised as any NaN
    of a row is.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns (several chains are
    one pool).  ``weights``, ``groups``, ``draws``, ``transform`` and ``offset`` as in :func:`bayes_r2`.

    With ``y`` ``(n_rows,)`` (a fit with one output): ``mse_permuted`` ``(D, q, R[, G])``, the weighted mean squared
    error of every draw with the column scrambled; ``mse_base`` ``(D[, G])``, the same of the fit itself, with the bits
    of :func:`bayes_r2`'s ``mse``; ``importance = mse_permuted.mean(R) - mse_base`` ``(D, q[, G])``, a posterior of the
    loss increase, with ``importance_mean``, ``importance_sd`` ``(q[, G])`` and ``importance_hdi`` ``(q[, G], 2)``
    (94 %) over the draws; ``r2_drop`` ``(D, q[, G])``, the loss of Bayesian R-squared.  Under ``transform="logistic"``
    or ``"probit"`` with a 0 / 1 ``y`` the loss is the Brier score.  A column no tree of a draw uses has
    ``importance`` exactly 0.0 there.

    Without ``y`` (any number of outputs; ``transform`` must be ``"identity"``): ``shift`` and ``sensitivity``
    ``(D, K, q[, G])`` -- the K axis is dropped for one output -- the weighted mean over the rows of the change of the
    prediction and of its square, averaged over the repeats.

    Always: ``cols``, ``n_repeats``, ``n_draws``, ``n_nonfinite`` (transformed values, of the fit and of every permuted
    prediction, that were an infinity or a NaN; they are added all the same), ``group_labels`` and ``weight`` ``(G,)``.
    The G axis is there when ``groups`` is given.

    Rows are processed in blocks and, where the scratch of a 64-row block or the partial sums of all columns exceed
    ``PGB_PW_BLOCK_BYTES``, columns in chunks; a single column that does not fit is refused."""
    return PermutationJob(sampler, X, y, cols, n_repeats, draws, weights, groups, transform, offset, random_seed).run()
