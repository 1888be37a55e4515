"""The numbers behind individual conditional expectation curves (``include/pgbart_ice.h``).

A curve is the mean over chosen posterior draws of the prediction along one covariate's observed values with every
other covariate held at an instance row's values.  On the HIP backend one ``pgb_predict_ice`` call produces every
curve of a (columns x instances) sweep: no probe matrix is built, the packed trees are uploaded once and nothing of
size draws x rows reaches the host.  A backend whose library lacks the entry point (the CPU oracle) builds each probe
matrix, predicts it and sums in pick order -- the same numbers, the slow way.

The public call is :func:`pymc_bart_amd.partial.individual_conditional_expectation`; the samplers' ``ice_mean``
methods (:class:`~pymc_bart_amd.trees.PosteriorSampler`, the multi-chain sampler of ``utils``) end here.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._device import device_rows
from ._stored import block_bytes, check_cols, check_picks, check_X, col_blocks


def _checked(X, resident: bool, instances, cols, picks, n_draws: int):
    """The arguments of one ``ice_mean`` call, validated on the host before a backend is touched."""
    X = check_X(X, resident)
    p = int(X.shape[1])
    inst = np.asarray(instances, dtype=np.float64)
    if inst.ndim == 1:
        inst = inst[None, :]
    if inst.ndim != 2 or inst.shape[0] < 1 or inst.shape[1] != p:
        raise ValueError(f"instances must have shape (n_inst, p = {p}), got {inst.shape}")
    cols = check_cols(cols, p)
    picks = np.asarray(picks, dtype=np.int64)
    if picks.ndim != 3 or picks.shape[:2] != (cols.size, inst.shape[0]):
        raise ValueError(f"picks must have shape (n_cols, n_inst, n_picks) = ({cols.size}, {inst.shape[0]}, n_picks), "
                         f"got {picks.shape}")
    picks = check_picks(picks, n_draws, "no draws to average: picks must name at least one of the stored draws per curve")
    return X, np.ascontiguousarray(inst), cols, picks


def _on_host(predict, X, inst, cols, picks, K: int) -> np.ndarray:
    """The loop a backend without ``pgb_predict_ice`` runs: the probe matrix of every curve, its predictions for the
    picked draws (``predict(X, draw_indices, excluded) -> (n_picks, K, n_rows)``), summed in pick order, divided once."""
    n, p = X.shape
    out = np.empty((cols.size, inst.shape[0], K, n))
    for c, j in enumerate(cols.tolist()):
        others = [v for v in range(p) if v != j]
        for r in range(inst.shape[0]):
            probe = X.copy()
            probe[:, others] = inst[r, others]
            pred = np.asarray(predict(probe, picks[c, r].tolist(), None))
            total = pred[0].copy()
            for s in range(1, pred.shape[0]):
                total += pred[s]
            out[c, r] = total / pred.shape[0]
    return out


def ice_mean(be, pool, table, m: int, K: int, predict, X, instances, cols, picks) -> np.ndarray:
    """``(n_cols, n_inst, K, n_rows)``: entry ``[c, r, k, i]`` is the mean over the draws ``picks[c, r, :]`` (rows of
    ``table``, summed in that order, divided once) of output ``k`` predicted at instance row ``r`` with its column
    ``cols[c]`` replaced by ``X[i, cols[c]]``.  ``be``: the backend; ``predict``: the sampler's ``sample_posterior``,
    used by a backend without ``pgb_predict_ice``."""
    mem, lib = be.mem, be.lib
    X, resident = device_rows(mem, X)  # (a device tensor: dense and row-major from here on)
    n_draws = int(np.asarray(table).shape[0])
    X, inst, cols, picks = _checked(X, resident, instances, cols, picks, n_draws)
    n, p = (int(v) for v in X.shape)
    n_cols, n_inst, n_picks = (int(v) for v in picks.shape)
    if not hasattr(lib.lib, "pgb_predict_ice"):
        return _on_host(predict, mem.to_host(X) if resident else X, inst, cols, picks, K)
    call = lib.ice_entry_point()
    fidx = np.ascontiguousarray(table, dtype=np.int32)
    xd = X if resident else mem.from_host(X)
    idev = mem.from_host(inst)
    carr = pool.as_c()
    out = np.empty((n_cols, n_inst, K, n))
    for c0, c1 in col_blocks(n_cols, 8 * n_inst * K * n, block_bytes("PGB_ICE_BLOCK_BYTES", 1 << 16)):
        cb, pb = np.ascontiguousarray(cols[c0:c1]), np.ascontiguousarray(picks[c0:c1])
        od = mem.empty(((c1 - c0) * n_inst * K * n,), np.float64)
        rc = call(C.byref(carr), fidx.ctypes.data, n_draws, int(m), mem.ptr(xd), n, p, p, mem.ptr(idev), n_inst, p,
                  cb.ctypes.data, c1 - c0, pb.ctypes.data, n_picks, mem.ptr(od), mem.stream_ptr)
        lib.check(rc, "pgb_predict_ice")
        out[c0:c1] = mem.to_host(od).reshape(c1 - c0, n_inst, K, n)
    return out
