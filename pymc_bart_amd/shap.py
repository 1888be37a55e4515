"""Why a row got its prediction: exact Shapley attributions of the stored posterior draws, on the device
(``pgb_predict_shap``, ``include/pgbart_shap.h``).

The players are the columns of ``X``; the value of a coalition is what ``sample_posterior`` returns with every column
outside it ``excluded`` -- marginalised by the trees' own training counts, the "path-dependent" conditional expectation
TreeSHAP is defined on.  Entry ``[d, k, i, j]`` is the share of column ``j`` in output ``k`` of draw ``d`` at row
``i``; ``base[d, k]`` is the draw's prediction with every column excluded, and ``base + values.sum(-1)`` is the plain
prediction of the row (efficiency).  A column whose value is NaN in a row gets exactly ``0.0`` there.  Because the whole
posterior of trees is kept, the attributions come draw by draw: :func:`shap_summary` reads their mean, sd, quantiles
and highest-density interval on the device.

The attributions are those of the linear predictor (the sum of trees), whatever the likelihood family.  HIP backend
only: a backend whose library lacks ``pgb_predict_shap`` (the CPU oracle) raises ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._device import device_rows
from ._stored import block_bytes, check_picks, check_X, hip_only, history, row_blocks


def checked(X, resident: bool, picks, n_draws: int):
    """The arguments of one sweep, validated on the host before a backend is touched."""
    X = check_X(X, resident)
    picks = np.asarray(picks, dtype=np.int64)
    if picks.ndim != 1:
        raise ValueError(f"picks must be a vector of draw indices, got shape {picks.shape}")
    return X, check_picks(picks, n_draws, "no draws to attribute: picks must name at least one of the stored draws")


def blocks(cells_per_row: int, n: int):
    """The row blocks ``(r0, r1)`` of one sweep of ``n`` rows: multiples of 64 rows whose ``cells_per_row`` doubles
    each (attributions: ``n_picks K p``; interactions: ``n_picks K q q``) stay under ``PGB_SHAP_BLOCK_BYTES`` (at
    least 64 rows)."""
    return row_blocks(n, 8 * cells_per_row, block_bytes("PGB_SHAP_BLOCK_BYTES", 1 << 12))


def _entry(lib):
    """``pgb_predict_shap`` of the backend's library; ``NotImplementedError`` naming it when the library has none."""
    return lib.shap_entry_point()


def device_blocks(be, pool, table, m: int, K: int, X, picks):
    """Generator over the row blocks of a sweep on the HIP backend: ``(r0, r1, buffer, base)``, ``buffer`` the device
    array ``[n_picks][K][p][r1 - r0]`` of that block (valid until the next one is asked for), ``base`` ``(n_picks, K)``.
    The arguments are those :func:`checked` returns."""
    mem, lib = be.mem, be.lib
    call = _entry(lib)
    n, p = (int(v) for v in X.shape)
    n_picks = int(picks.size)
    fidx = np.ascontiguousarray(table, dtype=np.int32)
    xd = X if mem.is_resident(X) else mem.from_host(X)
    carr = pool.as_c()
    base = np.empty((n_picks, K))
    for r0, r1 in blocks(n_picks * K * p, n):
        od = mem.empty((n_picks * K * p * (r1 - r0),), np.float64)
        rc = call(C.byref(carr), fidx.ctypes.data, int(fidx.shape[0]), int(m), mem.ptr(xd) + 8 * r0 * p, r1 - r0, p, p,
                  picks.ctypes.data, n_picks, mem.ptr(od), base.ctypes.data, mem.stream_ptr)
        lib.check(rc, "pgb_predict_shap")
        yield r0, r1, od, base


def shap_sweep(be, pool, table, m: int, K: int, X, picks):
    """``(values (n_picks, K, n_rows, p), base (n_picks, K))`` of the draws ``picks`` (rows of ``table``; they may
    repeat) at the rows of ``X`` (a host matrix, or a device matrix: ``PosteriorSampler.resident_rows``).  One
    ``pgb_predict_shap`` call per block of rows; the result does not depend on the blocking."""
    mem, lib = be.mem, be.lib
    X, resident = device_rows(mem, X)  # (a device tensor: dense and row-major from here on)
    X, picks = checked(X, resident, picks, int(np.asarray(table).shape[0]))
    _entry(lib)
    n, p = (int(v) for v in X.shape)
    out = np.empty((picks.size, K, n, p))
    base = None
    for r0, r1, od, b in device_blocks(be, pool, table, m, K, X, picks):
        out[:, :, r0:r1, :] = np.swapaxes(mem.to_host(od).reshape(picks.size, K, p, r1 - r0), 2, 3)
        base = b.copy()
    return out, base


def chosen_draws(n_draws: int, draws, samples, random_seed) -> np.ndarray:
    if draws is not None and samples is not None:
        raise ValueError("give draws= (indices of stored draws) or samples= (how many to draw at random), not both")
    if draws is not None:
        idx = np.asarray(draws, dtype=np.int64)
        if idx.ndim != 1:
            raise ValueError(f"draws must be a vector of draw indices, got shape {idx.shape}")
        return idx
    if samples is not None:
        if int(samples) < 1:
            raise ValueError(f"samples must be >= 1, got {samples!r}")
        return np.random.default_rng(random_seed).integers(0, n_draws, size=int(samples))
    return np.arange(n_draws, dtype=np.int64)


def shap_values(sampler, X, draws=None, samples=None, random_seed=None) -> dict:
    """Exact Shapley attributions of posterior draws at the rows of ``X``.

    ``sampler``: what ``_get_posterior_sampler(op)`` or ``PosteriorSampler.from_history`` returns (several chains count
    as one history).  ``draws``: indices of the stored draws (they may repeat); or ``samples``: that many draws chosen
    by one ``default_rng(random_seed).integers(0, n_draws, samples)`` call; neither: every stored draw.

    Returns ``{"values": (D, K, n_rows, p), "base": (D, K), "draws": the indices}``; the ``K`` axis is dropped when the
    sampler has one output."""
    parts, pool, table = history(sampler)
    n_draws = int(np.asarray(table).shape[0])
    picks = chosen_draws(n_draws, draws, samples, random_seed)
    K, m = int(parts[0].n_outputs), int(parts[0].m)
    values, base = shap_sweep(parts[0]._get_backend(), pool, table, m, K, X, picks)
    if K == 1:
        values, base = values[:, 0], base[:, 0]
    return {"values": values, "base": base, "draws": np.asarray(picks, dtype=np.int64).copy()}


def summary_result(by, Q: int, hdi_k, base, K: int, strength_key: str, extra: dict) -> dict:
    """The dict a summary returns, from ``by`` -- the rows of ``pgb_row_summary`` (mean, variance, ``Q`` quantiles,
    HDI) over ``(K, n_rows, ...)`` -- and the draws' ``base``: ``strength_key`` names the mean over the rows of
    ``|mean|``, the ``K`` axis is dropped when the sampler has one output, ``extra`` is added as it is."""
    res = {"mean": by[0].copy(), "sd": np.sqrt(by[1]), "var": by[1].copy(), "quantiles": by[2:2 + Q].copy(),
           "hdi": by[2 + Q:4 + Q].copy() if hdi_k else None, strength_key: np.abs(by[0]).mean(axis=1),
           "base_mean": base.mean(axis=0)}
    if K == 1:
        for key in ("mean", "sd", "var", strength_key, "base_mean"):
            res[key] = res[key][0]
        res["quantiles"] = res["quantiles"][:, 0]
        if res["hdi"] is not None:
            res["hdi"] = res["hdi"][:, 0]
    res.update(extra)
    return res


def shap_summary(sampler, X, draws=None, samples=None, random_seed=None, quantiles=(0.03, 0.5, 0.97),
                 hdi_prob=0.94) -> dict:
    """Posterior summaries of the attributions of :func:`shap_values`, computed where they lie: per block of rows one
    ``pgb_predict_shap`` call writes ``[D][K p rows]`` into device scratch and one ``pgb_row_summary`` call reads the
    mean, the variance, the quantiles and the highest-density interval of every (output, column, row) over the draws
    -- the ``(D, K, n_rows, p)`` array never reaches the host.  Between 2 and 16384 draws.

    Returns ``mean``, ``sd``, ``var`` ``(K, n_rows, p)``, ``quantiles`` ``(Q, K, n_rows, p)``, ``hdi`` ``(2, K, n_rows,
    p)`` (``None`` without ``hdi_prob``), ``importance`` ``(K, p)`` -- the mean over the rows of ``|mean|`` --,
    ``base_mean`` ``(K,)``, and ``q``, ``hdi_prob``, ``n_draws``, ``draws``; the ``K`` axis is dropped when the sampler
    has one output.  Blocks stay under ``PGB_SHAP_BLOCK_BYTES``; the result does not depend on it."""
    from .summary import spec, summary_block

    parts, pool, table = history(sampler)
    n_draws = int(np.asarray(table).shape[0])
    picks = chosen_draws(n_draws, draws, samples, random_seed)
    K, m = int(parts[0].n_outputs), int(parts[0].m)
    q, hdi_k, code = spec(int(np.asarray(picks).size), quantiles, hdi_prob, "identity")
    X, picks = checked(X, False, picks, n_draws)
    be = parts[0]._get_backend()
    _entry(be.lib)
    be = hip_only(be, "posterior summaries run")
    lib, mem = be.lib, be.mem
    n, p = (int(v) for v in X.shape)
    D, Q = int(picks.size), int(q.size)
    stats = np.empty((2 + Q + 2, K, p, n))
    base = None
    for r0, r1, od, b in device_blocks(be, pool, table, m, K, X, picks):
        width = K * p * (r1 - r0)
        stats[:, :, :, r0:r1] = summary_block(lib, mem, od, D, width, width, None, code, q, hdi_k).reshape(-1, K, p, r1 - r0)
        base = b.copy()
    by = np.ascontiguousarray(np.swapaxes(stats, 2, 3))  # (rows of the summary, K, n, p)
    return summary_result(by, Q, hdi_k, base, K, "importance",
                           {"q": q.copy(), "hdi_prob": None if hdi_prob is None else float(hdi_prob), "n_draws": D,
                            "draws": np.asarray(picks, dtype=np.int64).copy()})
