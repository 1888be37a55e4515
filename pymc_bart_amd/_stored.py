"""The Python front end of the stored-draw entry points, stated once (the counterpart of the C host front end in
``csrc/``): what every consumer of a fit's stored draws -- scoring, PSIS-LOO, summaries, replicated observations, chain
diagnostics, SHAP, partial dependence, ICE -- does before and around its own kernel.

* the four block knobs and the one block rule (:func:`block_bytes`, :func:`row_blocks`, :func:`col_blocks`);
* the HIP-only check (:func:`hip_only`) and the pooled history of a sampler (:func:`chains`, :func:`history`);
* the argument checks, one function each, with the texts the callers have always raised;
* :class:`Job`, the validated arguments of one call that walks the trees per block of rows, and its block driver
  :meth:`Job.blocks`; :func:`matrix_blocks`, the driver of the functions that take a ``(D, n)`` host matrix;
* :func:`fill_lik` and :func:`drop_k_axis`.

The bytes a row (or a column) of a block costs stay with each caller: they differ, and they belong to its kernels.
"""

from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _abi

MAX_OFFSET = 1.0e6  # PGB_MAX_OFFSET
PW_BLOCK = ("PGB_PW_BLOCK_BYTES", 1 << 16)  # (the knob of every consumer in this module; the sweeps name their own)


# ------------------------------------------------------------------------------------------ environment and backend
def block_bytes(env_name: str, floor: int) -> int:
    """Device bytes one block may take: the environment's ``env_name``, default 1 GiB, at least ``floor``.  The knobs
    are ``PGB_PW_BLOCK_BYTES`` (floor 64 KiB: scoring, PSIS, summaries, replicated observations, diagnostics),
    ``PGB_SHAP_BLOCK_BYTES`` (4 KiB), ``PGB_PDP_BLOCK_BYTES`` (4 KiB) and ``PGB_ICE_BLOCK_BYTES`` (64 KiB)."""
    return max(int(floor), int(os.environ.get(env_name, 1 << 30)))


def row_blocks(n: int, bytes_per_row: int, limit: int) -> list:
    """The row blocks ``[(r0, r1)]`` of ``n`` rows: as many rows as ``limit`` bytes hold, rounded down to a multiple
    of 64, at least 64 and at most ``n``.  (``shap.blocks`` and ``pdp.blocks`` used to leave out the "at most ``n``":
    the list is the same, because a block that starts at row 0 and is longer than ``n`` ends at ``n`` all the same.)"""
    rows = max(64, min(n, limit // bytes_per_row // 64 * 64))
    return [(r0, min(n, r0 + rows)) for r0 in range(0, n, rows)]


def col_blocks(n_cols: int, bytes_per_col: int, limit: int) -> list:
    """The column blocks ``[(c0, c1)]`` of ``n_cols`` whole columns: as many as ``limit`` bytes hold, at least one."""
    step = max(1, min(n_cols, limit // bytes_per_col))
    return [(c0, min(n_cols, c0 + step)) for c0 in range(0, n_cols, step)]


def hip_only(backend, what: str):
    """``backend`` (``None``: the default one) if it is the HIP library; ``PGBError`` "``what`` on the HIP backend
    only" otherwise."""
    from .sampler import default_backend

    be = backend if backend is not None else default_backend()
    if be.lib.backend_name != "hip-gfx950":
        raise _abi.PGBError(f"{what} on the HIP backend only, not on {be.lib.backend_name}")
    return be


# ---------------------------------------------------------------------------------------------------------- history
def chains(sampler) -> list:
    parts = getattr(sampler, "_chain_samplers", None)
    parts = list(parts) if parts is not None else [sampler]
    for part in parts:
        if not all(hasattr(part, a) for a in ("pool", "forest_idx", "m")):
            raise TypeError("sampler must be what _get_posterior_sampler(op) or PosteriorSampler.from_history returns")
    return parts


def history(sampler) -> tuple:
    """-> (the chains of the sampler, the pool and the forest table of all of them as one history)."""
    from .trees import pooled_history

    parts = chains(sampler)
    cached = getattr(sampler, "pooled_history", None)  # (the multi-chain sampler keeps it)
    pool, table = cached() if cached is not None else pooled_history(parts)
    return parts, pool, table


# -------------------------------------------------------------------------------------------------- argument checks
def check_X(X, resident: bool = False):
    """``X`` as the kernels read it: a host matrix made float64, two-dimensional and contiguous, or -- ``resident`` --
    the device matrix ``_device.device_rows`` returned, looked at by its shape only."""
    if not resident:
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X[:, None]
    if len(X.shape) != 2 or int(X.shape[0]) < 1 or int(X.shape[1]) < 1:
        raise ValueError(f"X must be a matrix (n_rows, p), got shape {tuple(X.shape)}")
    return X if resident else np.ascontiguousarray(X)


def check_y(y, n: int) -> np.ndarray:
    y = np.asarray(y, dtype=np.float64)
    if y.shape != (n,):
        raise ValueError(f"y must hold one value per row of X: shape ({n},), got {y.shape}")
    if not np.all(np.isfinite(y)):
        raise ValueError("y must be finite")
    return np.ascontiguousarray(y)


def check_offset(offset, K: int, n: int):
    if offset is None:
        return None
    off = np.asarray(offset, dtype=np.float64)
    if off.shape == (n,) and K == 1:
        off = off[None, :]
    if off.shape != (K, n):
        raise ValueError(f"offset must have shape (n_outputs, n_rows) = ({K}, {n}), got {off.shape}")
    if not np.all(np.isfinite(off)) or np.max(np.abs(off)) > MAX_OFFSET:
        raise ValueError(f"offset must be finite and within +-{MAX_OFFSET:g}")
    return np.ascontiguousarray(off)


def check_excluded(excluded, p: int) -> np.ndarray:
    excl = np.asarray([] if excluded is None else excluded, dtype=np.int64).ravel()
    if excl.size and (excl.min() < 0 or excl.max() >= p):
        raise ValueError(f"excluded must index the {p} columns of X")
    return np.ascontiguousarray(excl, dtype=np.int32)


def check_draws(draws, total: int) -> np.ndarray:
    """The indexes of the stored draws of one call (``None``: all ``total``)."""
    if draws is None:
        return np.arange(total, dtype=np.int64)
    idx = np.asarray(draws, dtype=np.int64).ravel()
    if idx.size and (idx.min() < 0 or idx.max() >= total):
        raise ValueError(f"draws must index the {total} stored draws")
    return idx


def check_seed(random_seed) -> int:
    seed = int(random_seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"random_seed must be an integer in [0, 2^64), got {random_seed!r}")
    return seed


def check_cols(cols, p: int) -> np.ndarray:
    """The columns of a partial-dependence or ICE sweep."""
    cols = np.asarray(cols, dtype=np.int64)
    if cols.ndim != 1 or cols.size < 1:
        raise ValueError(f"cols must be a non-empty vector of column indices, got shape {cols.shape}")
    if cols.min() < 0 or cols.max() >= p:
        raise ValueError(f"cols must index the {p} columns of X")
    return np.ascontiguousarray(cols, dtype=np.int32)


def check_picks(picks: np.ndarray, n_draws: int, none: str) -> np.ndarray:
    """The draws a sweep picks (its caller has checked their shape; the picks of a curve lie along the last axis):
    at least one, each a stored draw; ``none`` is what the caller says when there is nothing to pick."""
    if picks.shape[-1] < 1 or n_draws < 1:
        raise ValueError(none)
    if picks.min() < 0 or picks.max() >= n_draws:
        raise ValueError(f"picks must index the {n_draws} stored draws")
    return np.ascontiguousarray(picks, dtype=np.int32)


# --------------------------------------------------------------------------------------------------------- the jobs
@dataclass
class Block:
    """One block of rows ``r0 .. r1`` on the device: the rows of ``X``, of the offset and of ``y`` (``None`` where the
    job has none) and the block's matrix ``md`` -- the predictions ``[D][K][nb]`` of :meth:`Job.predict`, or what the
    consumer puts there.  Whoever holds the record keeps the buffers alive."""

    r0: int
    r1: int
    xd: object
    od: object = None
    yd: object = None
    md: object = None

    @property
    def nb(self) -> int:
        return self.r1 - self.r0


class Job:
    """Everything of one call that walks the stored trees per block of rows, validated on the host before a backend is
    touched.  A consumer takes its arguments in its own order -- that order decides which of two faults is reported --
    through ``take_X``, ``take_offset``, ``take_excluded``, ``take_draws`` and, last, ``take_history``; what it adds of
    its own (a family, ``y``, a summary spec, a seed) it checks in between."""

    offset = None
    excluded = np.empty(0, np.int32)

    def __init__(self, sampler):
        self.sampler = sampler
        self.parts = parts = chains(sampler)
        self.K = int(parts[0].n_outputs)
        self.m = int(parts[0].m)
        self.backend = parts[0]._get_backend if hasattr(parts[0], "_get_backend") else None  # (the hook, not its result)

    def take_X(self, X):
        self.X = check_X(X)
        self.n, self.p = (int(v) for v in self.X.shape)

    def take_offset(self, offset):
        self.offset = check_offset(offset, self.K, self.n)

    def take_excluded(self, excluded):
        self.excluded = check_excluded(excluded, self.p)

    def take_draws(self, draws, none: str | None = None):
        """``none``: what to say when no draw is left (``None``: the consumer has a check of its own)."""
        self._idx = check_draws(draws, int(sum(part.forest_idx.shape[0] for part in self.parts)))  # several chains: one pool
        if none is not None and self._idx.size < 1:
            raise ValueError(none)
        self.D = int(self._idx.size)

    def take_history(self):
        _, self.pool, table = history(self.sampler)
        self.fidx = np.ascontiguousarray(np.asarray(table)[self._idx], dtype=np.int32)

    def hip_backend(self, what: str):
        return hip_only(self.backend() if self.backend is not None else None, what)

    def predict(self, be, xd, nb: int):
        """``pgb_predict`` of the job's draws at the ``nb`` device rows ``xd`` -> the device matrix ``[D][K][nb]``
        (``K * nb`` columns over the draws)."""
        lib, mem, excl = be.lib, be.mem, self.excluded
        md = mem.empty((self.D * self.K * nb,), np.float64)
        carr = self.pool.as_c()
        rc = lib.lib.pgb_predict(C.byref(carr), self.fidx.ctypes.data, self.D, self.m, mem.ptr(xd), nb, self.p, self.p,
                                 excl.ctypes.data if excl.size else None, int(excl.size), mem.ptr(md), mem.stream_ptr)
        lib.check(rc, "pgb_predict")
        return md

    def blocks(self, be, bytes_per_row: int, y: bool = False, predict: bool = False, reserved: int = 0):
        """Generator over the row blocks of the call (``PGB_PW_BLOCK_BYTES``): uploads the block's rows of ``X``, of
        ``y`` if asked to and of the offset, runs :meth:`predict` into ``md`` if asked to, and hands out the
        :class:`Block`.  ``reserved``: device bytes the consumer holds across all blocks; they come off what a block
        may take."""
        mem = be.mem
        for r0, r1 in row_blocks(self.n, bytes_per_row, block_bytes(*PW_BLOCK) - int(reserved)):
            blk = Block(r0, r1, mem.from_host(self.X[r0:r1]))
            if y:
                blk.yd = mem.from_host(self.y[r0:r1])
            if self.offset is not None:
                blk.od = mem.from_host(np.ascontiguousarray(self.offset[:, r0:r1]))
            if predict:
                blk.md = self.predict(be, blk.xd, r1 - r0)
            yield blk


def matrix_blocks(be, bytes_per_col: int, *arrays):
    """Generator over the column blocks of host arrays ``(D, n)`` or ``(n,)`` (``None`` stays ``None``), for the
    functions that take a matrix of draws: ``(r0, r1, the device copy of every array's columns r0 .. r1)``."""
    n = int(arrays[0].shape[-1])
    for r0, r1 in row_blocks(n, bytes_per_col, block_bytes(*PW_BLOCK)):
        yield (r0, r1) + tuple(None if a is None else be.mem.from_host(np.ascontiguousarray(a[..., r0:r1])) for a in arrays)


# ---------------------------------------------------------------------------------------------------- small helpers
def fill_lik(lik, job):
    """The family, the number of params per draw and their host matrix of ``job`` in a ``PointwiseLik`` / ``PpcLik``."""
    lik.family = _abi.FAMILIES[job.family]
    lik.n_params = job.n_par
    lik.params_host = job.params.ctypes.data if job.n_par else None
    return lik


def drop_k_axis(res: dict, keys=("mean", "sd", "var", "quantiles", "hdi")) -> dict:
    """The trailing axis of one output taken off the arrays of a summary dict (``None`` stays)."""
    for key in keys:
        if res[key] is not None:
            res[key] = res[key][..., 0]
    return res
