"""Host reference of the predictive scores: a small C shim around ``include/pgbart_score.h`` -- the header the device
kernel compiles -- built with gcc like ``tests/_rowsummary_host.py``.  It exports the header's ``pgb_score_column``
over the columns of a matrix, and :func:`public` restates the host arithmetic of ``pymc_bart_amd/scores.py`` from the
formulas of the issue, independently of that module."""
import ctypes as C

import numpy as np

from _host_build import build

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include "pgbart_score.h"
int score_nout(int n_q) { return PGB_SCORE_NOUT(n_q); }
/* out[6 + 2 n_q][n] of a[D][ld]'s first n columns against y[n] */
int score_columns(const double* a, int D, int64_t n, int64_t ld, const double* y, const double* q, int n_q, double* out) {
  uint64_t* key = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)D);
  double* wk = (double*)malloc(sizeof(double) * (size_t)D);
  if (!key || !wk) return 1;
  double o[PGB_SCORE_NOUT(PGB_ROWSUM_MAX_Q)];
  for (int64_t i = 0; i < n; ++i) {
    pgb_score_column(a + i, ld, D, y[i], q, n_q, key, wk, o);
    for (int r = 0; r < PGB_SCORE_NOUT(n_q); ++r) out[(size_t)r * (size_t)n + (size_t)i] = o[r];
  }
  free(key);
  free(wk);
  return 0;
}
"""

SIGNATURES = {"score_columns": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])}
ROWS = ("mean", "var", "abs_err", "pair_sum", "n_below", "n_equal")


def lib():
    return build("score_host", SHIM, SIGNATURES)


def nout(n_q: int) -> int:
    return int(lib().score_nout(int(n_q)))


def columns(a, y, q=()) -> np.ndarray:
    """``(6 + 2 Q, n)`` = [mean, var, abs_err, pair_sum, n_below, n_equal, q..., pinball...] of the columns of ``a``
    (D, n) against ``y`` (n,): the header's pgb_score_column."""
    a = np.ascontiguousarray(a, np.float64)
    D, n = a.shape
    y = np.ascontiguousarray(y, np.float64)
    q = np.ascontiguousarray(q, np.float64)
    assert 2 <= D <= 16384 and q.size <= 16 and y.shape == (n,)
    out = np.empty((nout(q.size), n))
    assert out.shape[0] == 6 + 2 * q.size
    assert lib().score_columns(a.ctypes.data, D, n, n, y.ctypes.data, q.ctypes.data if q.size else None, q.size,
                               out.ctypes.data) == 0
    return out


def column(x, y: float, q=()) -> dict:
    """One column ``x`` (D,) against one ``y``: the six fixed outputs by name, ``q`` and ``pinball`` as arrays."""
    q = np.asarray(q, np.float64)
    s = columns(np.asarray(x, np.float64)[:, None], np.array([float(y)]), q)[:, 0]
    out = dict(zip(ROWS, s[:6]))
    out["q"], out["pinball"] = s[6:6 + q.size], s[6 + q.size:]
    return out


def merged_levels(quantiles, intervals):
    """-> (the levels of the call: the quantiles, then the interval ends not among them; where the ends are (I, 2))."""
    levels = [float(v) for v in quantiles]
    ends = []
    for c in intervals:
        pair = []
        for level in ((1.0 - c) / 2.0, (1.0 + c) / 2.0):
            if level not in levels:
                levels.append(level)
            pair.append(levels.index(level))
        ends.append(pair)
    return np.array(levels, np.float64), np.array(ends, np.int64).reshape(-1, 2)


def public(a, y, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95), intervals=(0.5, 0.9)) -> dict:
    """The header's numbers in the layout of ``score_matrix``: every key of it that is an array over the columns of
    ``a`` (D, n), and the totals, by the issue's formulas."""
    a = np.asarray(a, np.float64)
    y = np.asarray(y, np.float64)
    D, n = a.shape
    levels, ends = merged_levels(quantiles, intervals)
    Q, L = len(quantiles), levels.size
    s = columns(a, y, levels)
    mean, var, abs_err, pair_sum, below, equal = s[:6]
    crps = abs_err - pair_sum / (float(D) * float(D))
    sq = (mean - y) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        dss = np.where(var == 0.0, np.inf, sq / var + np.log(var))
    iscore, covered = np.empty((len(intervals), n)), np.empty((len(intervals), n), bool)
    for i, c in enumerate(intervals):
        lo, hi, alpha = s[6 + ends[i, 0]], s[6 + ends[i, 1]], 1.0 - c
        iscore[i] = (hi - lo) + (2.0 / alpha) * np.maximum(lo - y, 0.0) + (2.0 / alpha) * np.maximum(y - hi, 0.0)
        covered[i] = (lo <= y) & (y <= hi)
    pinball = s[6 + L:6 + L + Q]
    return {"crps": crps, "crps_fair": abs_err - pair_sum / (float(D) * float(D - 1)), "squared_error": sq, "dss": dss,
            "n_zero_var": int((var == 0.0).sum()), "pit": (below + 0.5 * equal) / D, "n_below": below.astype(np.int64),
            "n_equal": equal.astype(np.int64), "mean": mean, "sd": np.sqrt(var), "quantiles": s[6:6 + Q], "pinball": pinball,
            "interval_score": iscore, "covered": covered, "mean_crps": float(crps.mean()),
            "se_crps": float(crps.std() / np.sqrt(n)) if n > 1 else 0.0, "mean_pinball": pinball.mean(axis=1),
            "mean_interval_score": iscore.mean(axis=1), "coverage": covered.mean(axis=1),
            "rmse": float(np.sqrt(sq.mean())), "n_draws": D}
