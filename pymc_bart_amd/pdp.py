"""The numbers behind partial dependence (``include/pgbart_pdp.h``).

Entry ``[c, s, k, i]`` of a sweep is the prediction of stored draw ``picks[c, s]``, output ``k``, at a row whose column
``cols[c]`` holds ``X[i, cols[c]]`` with every other column marginalised by the trees' own training counts: exactly
``sample_posterior(X, picks[c], excluded = all but cols[c])``.  On the HIP backend one ``pgb_predict_pdp`` call
produces every (column, draw) of a sweep: the packed trees are uploaded once, and a column its forests test with
``x <= v`` splits only is evaluated once per interval between the split values and looked up per row.  A backend whose
library lacks the entry point (the CPU oracle) loops ``sample_posterior`` over the columns -- the same numbers.

The public call is :func:`pymc_bart_amd.partial.partial_dependence`; the samplers' ``pdp_sweep`` methods
(:class:`~pymc_bart_amd.trees.PosteriorSampler`, the multi-chain sampler of ``utils``) end here.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._device import device_rows
from ._stored import block_bytes, check_cols, check_picks, check_X, col_blocks, row_blocks

ROUTES = (0, 1, 2)  # PGB_PDP_ROUTE_AUTO, _DIRECT, _PROFILE


def checked(X, resident: bool, cols, picks, n_draws: int, route):
    """The arguments of one ``pdp_sweep`` call, validated on the host before a backend is touched."""
    X = check_X(X, resident)
    cols = check_cols(cols, int(X.shape[1]))
    picks = np.asarray(picks, dtype=np.int64)
    if picks.ndim != 2 or picks.shape[0] != cols.size:
        raise ValueError(f"picks must have shape (n_cols, n_picks) = ({cols.size}, n_picks), got {picks.shape}")
    picks = check_picks(picks, n_draws, "no draws to predict: picks must name at least one of the stored draws per column")
    if isinstance(route, bool) or route not in ROUTES:
        raise ValueError(f"route must be 0 (auto), 1 (direct) or 2 (profile where eligible), got {route!r}")
    return X, cols, picks


def _on_host(predict, X, cols, picks) -> np.ndarray:
    """The loop a backend without ``pgb_predict_pdp`` runs: per column ``predict(X, draw_indices, excluded) ->
    (n_picks, K, n_rows)`` with every other column excluded."""
    p = int(X.shape[1])
    return np.stack([np.asarray(predict(X, picks[c].tolist(), [v for v in range(p) if v != j]))
                     for c, j in enumerate(cols.tolist())])


def blocks(n_cols: int, n_picks: int, K: int, n: int):
    """The blocks ``(c0, c1, r0, r1)`` of one sweep: whole columns while ``PGB_PDP_BLOCK_BYTES`` holds at least one
    (all rows of each), rows of one column otherwise (multiples of 64)."""
    per_col = 8 * n_picks * K * n
    limit = block_bytes("PGB_PDP_BLOCK_BYTES", 1 << 12)
    if per_col <= limit:
        return [(c0, c1, 0, n) for c0, c1 in col_blocks(n_cols, per_col, limit)]
    return [(c, c + 1, r0, r1) for c in range(n_cols) for r0, r1 in row_blocks(n, 8 * n_picks * K, limit)]


def device_blocks(be, pool, table, m: int, K: int, X, cols, picks, route: int = 0, taken=None):
    """Generator over the blocks of a sweep on the HIP backend: ``(c0, c1, r0, r1, buffer)``, ``buffer`` the device
    array ``[c1 - c0][n_picks][K][r1 - r0]`` of that block (valid until the next one is asked for).  The arguments are
    those :func:`checked` returns; ``taken``: a list that receives ``(c0, c1, r0, r1, routes of the block's columns)``."""
    mem, lib = be.mem, be.lib
    call = lib.pdp_entry_point()
    n, p = (int(v) for v in X.shape)
    n_cols, n_picks = (int(v) for v in picks.shape)
    fidx = np.ascontiguousarray(table, dtype=np.int32)
    xd = X if mem.is_resident(X) else mem.from_host(X)
    carr = pool.as_c()
    for c0, c1, r0, r1 in blocks(n_cols, n_picks, K, n):
        cb, pb = np.ascontiguousarray(cols[c0:c1]), np.ascontiguousarray(picks[c0:c1])
        od = mem.empty(((c1 - c0) * n_picks * K * (r1 - r0),), np.float64)
        rt = np.zeros(c1 - c0, np.int32)
        rc = call(C.byref(carr), fidx.ctypes.data, int(fidx.shape[0]), int(m), mem.ptr(xd) + 8 * r0 * p, r1 - r0, p, p,
                  cb.ctypes.data, c1 - c0, pb.ctypes.data, n_picks, int(route), mem.ptr(od), rt.ctypes.data, mem.stream_ptr)
        lib.check(rc, "pgb_predict_pdp")
        if taken is not None:
            taken.append((c0, c1, r0, r1, rt.tolist()))
        yield c0, c1, r0, r1, od


def pdp_sweep(be, pool, table, m: int, K: int, predict, X, cols, picks, route: int = 0, taken=None) -> np.ndarray:
    """``(n_cols, n_picks, K, n_rows)``: entry ``[c, s, k, i]`` is output ``k`` of the draw ``picks[c, s]`` (a row of
    ``table``) predicted at ``X[i, cols[c]]`` with every other column excluded.  ``be``: the backend; ``predict``: the
    sampler's ``sample_posterior``, used by a backend without ``pgb_predict_pdp``.  ``route``: 0 lets the library
    choose per column, 1 walks every row, 2 takes the profile route for every eligible column -- the result is the
    same.  ``taken``: a list that receives, per block, ``(c0, c1, r0, r1, [route of each column: 1 direct, 2 profile])``."""
    mem, lib = be.mem, be.lib
    X, resident = device_rows(mem, X)  # (a device tensor: dense and row-major from here on)
    n_draws = int(np.asarray(table).shape[0])
    X, cols, picks = checked(X, resident, cols, picks, n_draws, route)
    if not hasattr(lib.lib, "pgb_predict_pdp"):
        return _on_host(predict, X, cols, picks)
    n = int(X.shape[0])
    n_cols, n_picks = (int(v) for v in picks.shape)
    out = np.empty((n_cols, n_picks, K, n))
    for c0, c1, r0, r1, od in device_blocks(be, pool, table, m, K, X, cols, picks, route, taken):
        out[c0:c1, :, :, r0:r1] = mem.to_host(od).reshape(c1 - c0, n_picks, K, r1 - r0)
    return out
