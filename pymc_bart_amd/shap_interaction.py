"""Which columns work together: exact SHAP interaction values of the stored posterior draws, on the device
(``pgb_predict_shap_interactions``, ``include/pgbart_shap_interaction.h``).

The players and the value of a coalition are those of :mod:`pymc_bart_amd.shap`.  Entry ``[d, k, i, a, b]`` with
``a != b`` is the share of the pair of columns ``cols[a]``, ``cols[b]`` in output ``k`` of draw ``d`` at row ``i`` (the
SHAP interaction index, split evenly between ``[a, b]`` and ``[b, a]``); ``[d, k, i, a, a]`` is the main effect of
``cols[a]``: its attribution less its shares with EVERY other column, chosen or not.  Over all columns the matrix is
symmetric, row ``a`` sums to the attribution ``shap_values`` reports and ``base + values.sum((-2, -1))`` is the plain
prediction.  A column whose value is NaN in a row has a row and a column of exactly ``0.0`` there.

A term of a leaf costs ``O(u^4)`` in the number ``u`` of distinct columns on its path, so a history with a leaf of more
than 32 slots (path columns plus a regressor off the path) is refused.  HIP backend only: a backend whose library lacks
``pgb_predict_shap_interactions`` (the CPU oracle) raises ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._device import device_rows
from ._stored import hip_only, history
from .shap import blocks, checked, chosen_draws, summary_result


def _checked_cols(cols, p: int) -> np.ndarray:
    """``cols`` validated against the ``p`` columns of ``X``: a vector of distinct indices; ``None``: every column."""
    if cols is None:
        return np.arange(p, dtype=np.int32)
    idx = np.asarray(cols)
    if idx.ndim != 1:
        raise ValueError(f"cols must be a vector of column indices, got shape {idx.shape}")
    if idx.size < 1:
        raise ValueError("no columns to relate: cols must name at least one column of X")
    if idx.dtype.kind not in "iu":
        raise ValueError(f"cols must be integers, got dtype {idx.dtype}")
    idx = idx.astype(np.int64)
    if idx.min() < 0 or idx.max() >= p:
        raise ValueError(f"cols must index the {p} columns of X")
    if np.unique(idx).size != idx.size:
        raise ValueError("cols must not name a column twice")
    return np.ascontiguousarray(idx, dtype=np.int32)


def _entry(lib):
    """``pgb_predict_shap_interactions`` of the backend's library; ``NotImplementedError`` naming it when the library
    has none."""
    return lib.shap_interactions_entry_point()


def device_blocks(be, pool, table, m: int, K: int, X, cols, picks):
    """Generator over the row blocks of a sweep on the HIP backend: ``(r0, r1, buffer, base)``, ``buffer`` the device
    array ``[n_picks][K][q][q][r1 - r0]`` of that block (valid until the next one is asked for), ``base`` ``(n_picks,
    K)``.  The arguments are those :func:`~pymc_bart_amd.shap.checked` and :func:`_checked_cols` return."""
    mem, lib = be.mem, be.lib
    call = _entry(lib)
    n, p = (int(v) for v in X.shape)
    n_picks, q = int(picks.size), int(cols.size)
    fidx = np.ascontiguousarray(table, dtype=np.int32)
    xd = X if mem.is_resident(X) else mem.from_host(X)
    carr = pool.as_c()
    base = np.empty((n_picks, K))
    for r0, r1 in blocks(n_picks * K * q * q, n):
        od = mem.empty((n_picks * K * q * q * (r1 - r0),), np.float64)
        rc = call(C.byref(carr), fidx.ctypes.data, int(fidx.shape[0]), int(m), mem.ptr(xd) + 8 * r0 * p, r1 - r0, p, p,
                  cols.ctypes.data, q, picks.ctypes.data, n_picks, mem.ptr(od), base.ctypes.data, mem.stream_ptr)
        lib.check(rc, "pgb_predict_shap_interactions")
        yield r0, r1, od, base


def shap_interaction_sweep(be, pool, table, m: int, K: int, X, picks, cols=None):
    """``(values (n_picks, K, n_rows, q, q), base (n_picks, K), the columns (q,))`` of the draws ``picks`` (rows of ``table``; they may
    repeat) at the rows of ``X`` (a host matrix, or a device matrix: ``PosteriorSampler.resident_rows``) between the
    columns ``cols`` (``None``: all).  One ``pgb_predict_shap_interactions`` call per block of rows; the result does not
    depend on the blocking."""
    mem, lib = be.mem, be.lib
    X, resident = device_rows(mem, X)  # (a device tensor: dense and row-major from here on)
    X, picks = checked(X, resident, picks, int(np.asarray(table).shape[0]))
    n, p = (int(v) for v in X.shape)
    cols = _checked_cols(cols, p)
    _entry(lib)
    q = int(cols.size)
    out = np.empty((picks.size, K, n, q, q))
    base = None
    for r0, r1, od, b in device_blocks(be, pool, table, m, K, X, cols, picks):
        out[:, :, r0:r1] = np.moveaxis(mem.to_host(od).reshape(picks.size, K, q, q, r1 - r0), 4, 2)
        base = b.copy()
    return out, base, cols


def shap_interaction_values(sampler, X, cols=None, draws=None, samples=None, random_seed=None) -> dict:
    """Exact SHAP interaction values of posterior draws at the rows of ``X``.

    ``sampler``, ``draws``, ``samples`` and ``random_seed`` are :func:`pymc_bart_amd.shap_values`'s.  ``cols``: the
    distinct columns whose ``q x q`` block is wanted, in the order given (``None``: every column); the entries do not
    depend on which other columns are chosen.

    Returns ``{"values": (D, K, n_rows, q, q), "base": (D, K), "draws": the indices, "cols": the columns}``; the ``K``
    axis is dropped when the sampler has one output."""
    parts, pool, table = history(sampler)
    n_draws = int(np.asarray(table).shape[0])
    picks = chosen_draws(n_draws, draws, samples, random_seed)
    K, m = int(parts[0].n_outputs), int(parts[0].m)
    values, base, cols = shap_interaction_sweep(parts[0]._get_backend(), pool, table, m, K, X, picks, cols)
    if K == 1:
        values, base = values[:, 0], base[:, 0]
    return {"values": values, "base": base, "draws": np.asarray(picks, dtype=np.int64).copy(), "cols": cols.astype(np.int64)}


def shap_interaction_summary(sampler, X, cols=None, draws=None, samples=None, random_seed=None,
                             quantiles=(0.03, 0.5, 0.97), hdi_prob=0.94) -> dict:
    """Posterior summaries of the interaction values of :func:`shap_interaction_values`, computed where they lie: per
    block of rows one ``pgb_predict_shap_interactions`` call writes ``[D][K q q rows]`` into device scratch and one
    ``pgb_row_summary`` call reads the mean, the variance, the quantiles and the highest-density interval of every
    (output, pair, row) over the draws -- the ``(D, K, n_rows, q, q)`` array never reaches the host.  Between 2 and
    16384 draws.

    Returns ``mean``, ``sd``, ``var`` ``(K, n_rows, q, q)``, ``quantiles`` ``(Q, K, n_rows, q, q)``, ``hdi`` ``(2, K,
    n_rows, q, q)`` (``None`` without ``hdi_prob``), ``strength`` ``(K, q, q)`` -- the mean over the rows of ``|mean|``
    --, ``base_mean`` ``(K,)``, and ``q``, ``hdi_prob``, ``n_draws``, ``draws``, ``cols``; the ``K`` axis is dropped when
    the sampler has one output.  Blocks stay under ``PGB_SHAP_BLOCK_BYTES``; the result does not depend on it."""
    from .summary import spec, summary_block

    parts, pool, table = history(sampler)
    n_draws = int(np.asarray(table).shape[0])
    picks = chosen_draws(n_draws, draws, samples, random_seed)
    K, m = int(parts[0].n_outputs), int(parts[0].m)
    q, hdi_k, code = spec(int(np.asarray(picks).size), quantiles, hdi_prob, "identity")
    X, picks = checked(X, False, picks, n_draws)
    n, p = (int(v) for v in X.shape)
    cols = _checked_cols(cols, p)
    be = parts[0]._get_backend()
    _entry(be.lib)
    be = hip_only(be, "posterior summaries run")
    lib, mem = be.lib, be.mem
    D, Q, nq = int(picks.size), int(q.size), int(cols.size)
    stats = np.empty((2 + Q + 2, K, nq, nq, n))
    base = None
    for r0, r1, od, b in device_blocks(be, pool, table, m, K, X, cols, picks):
        width = K * nq * nq * (r1 - r0)
        stats[..., r0:r1] = summary_block(lib, mem, od, D, width, width, None, code, q, hdi_k).reshape(-1, K, nq, nq, r1 - r0)
        base = b.copy()
    by = np.ascontiguousarray(np.moveaxis(stats, 4, 2))  # (rows of the summary, K, n, q, q)
    return summary_result(by, Q, hdi_k, base, K, "strength",
                           {"q": q.copy(), "hdi_prob": None if hdi_prob is None else float(hdi_prob), "n_draws": D,
                            "draws": np.asarray(picks, dtype=np.int64).copy(), "cols": cols.astype(np.int64)})
