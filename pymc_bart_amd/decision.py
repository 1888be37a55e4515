"""Choosing among candidate interventions with stored posterior draws, on the device (``pgb_predict_arms``,
``pgb_arm_decide``; ``include/pgbart_arms.h``): which of A arms is best for a row and with what posterior probability,
what assigning an arm costs in expectation, and what a rule is worth over the population, with a posterior band -- the
individualised-treatment-rule reading of a BART fit (Logan et al. 2019).

An arm sets the same ``s`` columns of every row (one column for a coded treatment, several for a one-hot one).  Changing
those columns can change only the trees that use one of them, so per draw the kernel walks the draw's UNION use list
alone -- once at the row and once per arm -- and adds the difference to the draw's plain prediction: A arms cost A + 1
short walks, not A full ones.  The argmax couples the arms inside every (draw, row); both reductions that follow it, over
the draws per row and over the rows per draw, finish on the device.  Per block of rows one ``pgb_predict``, one
``pgb_predict_arms`` and one ``pgb_arm_decide``; nothing of size arms x draws x rows reaches the host.

* :func:`arm_predictions` -- the predictions of every draw under every arm: the fused replacement of A
  ``sample_posterior`` calls on copies of ``X``.
* :func:`optimal_arm` -- the decision.

HIP backend only.  Every sum has a fixed order (sequential over the draws; 64 partials by row index mod 64, carried from
block to block, over the rows), so no bit of a result depends on the blocking of the rows or on the launch geometry.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._stored import MAX_OFFSET, PW_BLOCK, Job, block_bytes, check_cols
from .average import LANES, check_groups, check_weights
from .importance import hdi
from .summary import DEFAULT_HDI_PROB, TRANSFORMS

MAX_COLS = 16  # PGB_ARMS_MAX_COLS
MAX_ARMS = 64  # PGB_ARMS_MAX


def workspace_bytes(D: int, G: int, A: int) -> int:
    """The bytes of the partial sums of one call (``pgb_arm_decide_workspace_bytes``): 64 partials of 3 + 2 A sums per
    (draw, group), 64 of the weight per group, three counters."""
    return 8 * (D * G * (3 + 2 * A) * LANES + G * LANES + 3)


def check_arms(arms, s: int) -> np.ndarray:
    """``arms`` as the kernel reads them: ``(A, s)`` float64; a vector is ``(A, 1)`` for one column."""
    try:
        arms = np.asarray(arms, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("arms must be a matrix of numbers (n_arms, n_cols)") from None
    if arms.ndim == 1 and s == 1:
        arms = arms[:, None]
    if arms.ndim != 2 or arms.shape[1] != s or arms.shape[0] < 1:
        raise ValueError(f"arms must have shape (n_arms, {s}): one value per column of cols, got {arms.shape}")
    if arms.shape[0] > MAX_ARMS:
        raise ValueError(f"at most {MAX_ARMS} arms per call, got {arms.shape[0]}")
    return np.ascontiguousarray(arms)


def with_draw_stats(res: dict, per_draw: dict, hdi_prob: float) -> dict:
    """``res`` with every per-draw array ``(D, ...)`` of ``per_draw`` and its ``_mean``, ``_sd`` and ``_hdi`` over the
    draws."""
    for key, a in per_draw.items():
        flat = a.reshape(a.shape[0], -1)
        lo_hi = np.empty((flat.shape[1], 2))
        for j in range(flat.shape[1]):
            lo_hi[j] = hdi(flat[:, j], hdi_prob)
        with np.errstate(invalid="ignore"):
            res.update({key: a, key + "_mean": a.mean(axis=0), key + "_sd": a.std(axis=0),
                        key + "_hdi": lo_hi.reshape(a.shape[1:] + (2,))})
    return res


class ArmsJob(Job):
    """One call of this module.  The arguments are taken in this order: ``X``, the columns, the arms, the draws and --
    :func:`optimal_arm` only -- ``output``, the transform, the offset, the costs, the weights, the groups, the policy,
    ``hdi_prob``, the size of the partial sums; then the history.  The backend is asked for last."""

    def __init__(self, sampler, X, cols, arms, draws, backend):
        super().__init__(sampler)
        self.given_backend = backend
        self.take_X(X)
        self.cols = check_cols(np.atleast_1d(cols), self.p)
        if np.unique(self.cols).size != self.cols.size:
            raise ValueError("cols must not name a column twice")
        if self.cols.size > MAX_COLS:
            raise ValueError(f"at most {MAX_COLS} columns per arm, got {self.cols.size}")
        self.s = int(self.cols.size)
        self.arms = check_arms(arms, self.s)
        self.A = int(self.arms.shape[0])
        self.take_draws(draws, none="a decision needs at least 1 draw")
        self.picks = np.arange(self.D, dtype=np.int32)

    def take_output(self, output):
        if isinstance(output, (bool, np.bool_)) or not isinstance(output, (int, np.integer)) or not 0 <= int(output) < self.K:
            raise ValueError(f"output must be an integer in [0, {self.K}), got {output!r}")
        self.output = int(output)

    def take_row_offset(self, offset):
        """The offset of the one output a call reads: ``(n,)``."""
        self.off = None
        if offset is not None:
            off = np.asarray(offset, dtype=np.float64)
            if off.shape != (self.n,):
                raise ValueError(f"offset must hold one value per row of X: shape ({self.n},), got {off.shape}")
            if not np.all(np.isfinite(off)) or np.max(np.abs(off)) > MAX_OFFSET:
                raise ValueError(f"offset must be finite and within +-{MAX_OFFSET:g}")
            self.off = np.ascontiguousarray(off)

    def take_rows(self, weights, groups):
        """The weights and the groups of the averages over the rows."""
        self.weights = check_weights(weights, self.n)
        self.labels, self.gid, self.n_rows = check_groups(groups, self.n, self.weights)
        self.G = int(self.labels.size)

    def take_hdi_prob(self, hdi_prob):
        """The mass of the intervals over the draws of the per-draw results."""
        if not 0.0 < float(hdi_prob) < 1.0:
            raise ValueError(f"hdi_prob must lie in (0, 1), got {hdi_prob!r}")
        self.hdi_prob = float(hdi_prob)

    def take_decision(self, output, transform, offset, cost, maximize, weights, groups, policy, hdi_prob):
        self.take_output(output)
        transform = "identity" if transform is None else transform
        if transform not in TRANSFORMS:
            raise ValueError(f"unknown transform {transform!r}: use one of {', '.join(TRANSFORMS)}")
        self.code = TRANSFORMS[transform]
        self.take_row_offset(offset)
        self.cost = None
        if cost is not None:
            c = np.asarray(cost, dtype=np.float64)
            if c.shape != (self.A,):
                raise ValueError(f"cost must hold one value per arm: shape ({self.A},), got {c.shape}")
            if not np.all(np.isfinite(c)):
                raise ValueError("cost must be finite")
            self.cost = np.ascontiguousarray(c)
        self.sign = 1.0 if maximize else -1.0
        self.take_rows(weights, groups)
        self.policy = None
        if policy is not None:
            pol = np.asarray(policy)
            if pol.shape != (self.n,) or pol.dtype.kind not in "iu":
                raise ValueError(f"policy must hold one arm index per row of X: integers of shape ({self.n},), got "
                                 f"{pol.dtype} {pol.shape}")
            if pol.min() < 0 or pol.max() >= self.A:
                raise ValueError(f"policy must index the {self.A} arms")
            self.policy = np.ascontiguousarray(pol, dtype=np.int32)
        self.take_hdi_prob(hdi_prob)
        self.ws_bytes = workspace_bytes(self.D, self.G, self.A)
        if self.ws_bytes > block_bytes(*PW_BLOCK):
            raise ValueError(f"the partial sums of {self.D} draws x {self.G} groups x {self.A} arms take {self.ws_bytes} bytes, "
                             f"more than a block may take ({block_bytes(*PW_BLOCK)}, {PW_BLOCK[0]}): use fewer draws or groups")

    # ------------------------------------------------------------------ sizes
    def predict_row_bytes(self) -> int:
        """Device bytes one row of a block costs :func:`arm_predictions`: its covariates and its ``(A + 1) D K``
        predictions."""
        return 8 * self.p + (self.A + 1) * self.D * self.K * 8

    def decide_row_bytes(self) -> int:
        """... and :func:`optimal_arm`: also the scratch of the decide step (``umax`` and the best arm per draw), the
        weight, the group, the policy, the offset and the per-row outputs."""
        return self.predict_row_bytes() + 12 * self.D + 8 + 4 + 4 + 8 + self.A * (4 + 8 + 8) + 4

    # ------------------------------------------------------------------ the run
    def pick_backend(self):
        """The backend of the call: the one given, the sampler's, or the default one."""
        be = self.given_backend
        if be is None:
            if self.backend is not None:
                be = self.backend()
            else:
                from .sampler import default_backend

                be = default_backend()
        return be

    def hip(self):
        """The backend and the entry points; the CPU oracle has none: ``NotImplementedError`` naming
        ``pgb_predict_arms``."""
        be = self.pick_backend()
        return be, be.lib.arms_entry_points()

    def arms_block(self, be, predict_arms, blk, lens, arms=None):
        """``pgb_predict_arms`` of one block -> the device matrix ``[A][D][K][nb]``.  ``arms``: ``(A, s)`` float64 and
        contiguous (default: the job's own)."""
        mem, nb = be.mem, blk.nb
        arms = self.arms if arms is None else arms
        A = int(arms.shape[0])
        od = mem.empty((A * self.D * self.K * nb,), np.float64)
        carr = self.pool.as_c()
        rc = predict_arms(C.byref(carr), self.fidx.ctypes.data, self.D, self.m, mem.ptr(blk.xd), nb, self.p, self.p,
                          self.cols.ctypes.data, self.s, arms.ctypes.data, A, self.picks.ctypes.data, self.D,
                          mem.ptr(blk.md), mem.ptr(od), lens.ctypes.data, mem.stream_ptr)
        be.lib.check(rc, "pgb_predict_arms")
        return od

    def run_predictions(self) -> np.ndarray:
        self.take_history()
        be, (predict_arms, _, _, _) = self.hip()
        A, D, K = self.A, self.D, self.K
        out = np.empty((A, D, K, self.n))
        lens = np.zeros(D, np.int32)
        for blk in self.blocks(be, self.predict_row_bytes(), predict=True):
            od = self.arms_block(be, predict_arms, blk, lens)
            out[..., blk.r0:blk.r1] = be.mem.to_host(od).reshape(A, D, K, blk.nb)
        return out[:, :, 0] if K == 1 else out

    def run_decision(self) -> dict:
        self.take_history()
        be, (predict_arms, decide, finish, query) = self.hip()
        lib, mem = be.lib, be.mem
        A, D, K, G, n = self.A, self.D, self.K, self.G, self.n
        if int(query(D, G, A)) != self.ws_bytes:
            raise _abi.PGBError(f"pgb_arm_decide_workspace_bytes({D}, {G}, {A}) is not {self.ws_bytes}")
        ptr = lambda buf: None if buf is None else mem.ptr(buf)  # noqa: E731
        ws = mem.empty((self.ws_bytes // 8,), np.float64)
        nbest, mean, regret = np.empty((A, n), np.int32), np.empty((A, n)), np.empty((A, n))
        bayes = np.empty(n, np.int32)
        lens = np.zeros(D, np.int32)
        for blk in self.blocks(be, self.decide_row_bytes(), predict=True, reserved=self.ws_bytes):
            r0, r1, nb = blk.r0, blk.r1, blk.nb
            od = self.arms_block(be, predict_arms, blk, lens)
            wd, gd = mem.from_host(self.weights[r0:r1]), mem.from_host(self.gid[r0:r1])
            pd = None if self.policy is None else mem.from_host(self.policy[r0:r1])
            offd = None if self.off is None else mem.from_host(self.off[r0:r1])
            nd, md, rd = mem.empty((A * nb,), np.int32), mem.empty((A * nb,), np.float64), mem.empty((A * nb,), np.float64)
            bd = mem.empty((nb,), np.int32)
            # output k of the arm-major matrix, without a copy: element (a, d, i) at a D K nb + d K nb + k nb + i
            rc = decide(mem.ptr(od[self.output * nb:]), D * K * nb, K * nb, D, A, nb, mem.ptr(wd), mem.ptr(gd), ptr(pd), ptr(offd),
                        None if self.cost is None else self.cost.ctypes.data, self.sign, self.code, G, r0, int(r0 == 0),
                        mem.ptr(ws), mem.ptr(nd), mem.ptr(md), mem.ptr(rd), mem.ptr(bd), mem.stream_ptr)
            lib.check(rc, "pgb_arm_decide")
            nbest[:, r0:r1] = mem.to_host(nd).reshape(A, nb)
            mean[:, r0:r1] = mem.to_host(md).reshape(A, nb)
            regret[:, r0:r1] = mem.to_host(rd).reshape(A, nb)
            bayes[r0:r1] = mem.to_host(bd)
        n_out = 4 + 2 * A
        outd, wod = mem.empty((n_out * D * G,), np.float64), mem.empty((G,), np.float64)
        counts = (C.c_int64 * 3)()
        rc = finish(mem.ptr(ws), D, G, A, int(self.policy is not None), mem.ptr(outd), mem.ptr(wod), counts, mem.stream_ptr)
        lib.check(rc, "pgb_arm_decide_finish")
        out = mem.to_host(outd).reshape(n_out, D, G)
        res = {"p_best": np.ascontiguousarray(nbest.T) / float(D), "mean_utility": np.ascontiguousarray(mean.T),
               "expected_regret": np.ascontiguousarray(regret.T), "bayes_arm": bayes,
               "group_labels": self.labels.copy(), "group_weight": mem.to_host(wod), "n_rows": self.n_rows.copy(),
               "n_draws": D, "n_nonfinite": int(counts[0]), "n_list_trees": lens.astype(np.int64)}
        per_draw = {"value_optimal": out[0].copy(), "value_bayes": out[1].copy(), "regret_bayes": out[3].copy(),
                    "value_arm": np.ascontiguousarray(np.moveaxis(out[4:4 + A], 0, -1)),
                    "share_best": np.ascontiguousarray(np.moveaxis(out[4 + A:], 0, -1))}
        if self.policy is not None:
            per_draw["value_policy"] = out[2].copy()
        return with_draw_stats(res, per_draw, self.hdi_prob)


def arm_predictions(sampler, X, cols, arms, *, draws=None, backend=None) -> np.ndarray:
    """The predictions of every stored draw at the rows of ``X`` under each of the arms, computed on the device: the
    fused replacement of one ``sample_posterior`` call per arm on a copy of ``X`` whose columns ``cols`` hold the arm's
    values.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns (several chains are
    one pool).  ``cols``: 1 to 16 distinct columns; ``arms`` ``(A, len(cols))``, 1 to 64 arms (a vector for one
    column): any doubles -- a NaN is "unknown under this arm" and is marginalised as a NaN of a row is, the infinities
    are legal.  ``draws``: indexes of the stored draws (default: all).

    Returns ``(A, D, K, n)``, or ``(A, D, n)`` for a fit with one output.  A value is ``f + (A_a - A_self)``: the
    draw's plain prediction plus the change of the sum over the trees that use one of ``cols``
    (``include/pgbart_arms.h``); it differs from the prediction on the copy by the rounding of two more additions."""
    return ArmsJob(sampler, X, cols, arms, draws, backend).run_predictions()


def optimal_arm(sampler, X, cols, arms, *, output=0, transform=None, offset=None, cost=None, maximize=True, weights=None,
                groups=None, policy=None, draws=None, backend=None, hdi_prob: float = DEFAULT_HDI_PROB) -> dict:
    """Which arm is best for every row, with what posterior probability, and what a rule is worth over the rows, per
    stored draw, on the device.

    The utility of arm ``a`` in draw ``d`` at row ``i`` is ``u = sign * T(f_a + offset_i) - cost[a]``: ``f_a`` is
    :func:`arm_predictions`' value of output ``output``, ``T`` the ``transform`` of ``posterior_summary`` (default:
    identity), ``sign`` +1 with ``maximize`` and -1 without (the outcome is then a loss; utilities are its negative),
    ``cost`` ``(A,)`` finite (default: zeros).  The best arm of a (draw, row) is the first one no later arm beats; a
    NaN utility never wins unless all are NaN.

    ``weights`` ``(n,)``, ``groups`` ``(n,)``: as in ``average_prediction`` (a group of total weight 0 is refused).
    ``policy`` ``(n,)``: an arm index per row, a rule of your own to evaluate.

    Returns, per row: ``p_best`` ``(n, A)``, the share of the draws in which the arm is best; ``mean_utility``
    ``(n, A)``; ``expected_regret`` ``(n, A)``, the mean over the draws of what the arm loses against the draw's best
    one; ``bayes_arm`` ``(n,)``, the arm of the largest summed utility.  Per draw, as weighted means over the rows of
    a group: ``value_optimal`` (every row gets its draw's best arm: an upper bound no rule attains), ``value_bayes``
    (every row gets ``bayes_arm``), ``regret_bayes`` (their difference), with ``policy`` ``value_policy``, each
    ``(D, G)``; ``value_arm`` (everybody gets arm ``a``) and ``share_best`` (the weighted share of rows whose best arm
    is ``a``), each ``(D, G, A)``.  Each of them comes with ``_mean``, ``_sd`` and ``_hdi`` (``hdi_prob``) over the
    draws.  And ``group_labels``, ``group_weight``, ``n_rows`` ``(G,)``; ``n_draws``; ``n_nonfinite``, the utilities
    that were an infinity or a NaN (they are added all the same); ``n_list_trees`` ``(D,)``, the trees of every draw
    that use one of ``cols``: all that is ever walked for the arms.

    Rows are processed in blocks; a block and the partial sums -- 512 (3 + 2 A) bytes per (draw, group) -- together
    take at most ``PGB_PW_BLOCK_BYTES`` of device scratch.  No bit of a result depends on the blocking."""
    job = ArmsJob(sampler, X, cols, arms, draws, backend)
    job.take_decision(output, transform, offset, cost, maximize, weights, groups, policy, hdi_prob)
    return job.run_decision()
