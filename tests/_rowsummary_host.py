"""Host reference of the per-row posterior summaries: a small C shim around ``include/pgbart_rowsummary.h`` -- the
header the device kernel compiles -- built with gcc like ``tests/_psis_host.py``.  It exports the header's
``pgb_rowsum_column`` over the columns of a matrix."""
import ctypes as C

import numpy as np

from _host_build import build

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include "pgbart_rowsummary.h"
int rowsum_max_draws(void) { return PGB_ROWSUM_MAX_DRAWS; }
int rowsum_max_q(void) { return PGB_ROWSUM_MAX_Q; }
/* out[2 + n_q + 2][n] of a[D][ld]'s first n columns; off: [n] or NULL */
int rowsum_columns(const double* a, int D, int64_t n, int64_t ld, const double* off, int transform, const double* q,
                   int n_q, int hdi_k, double* out) {
  const pgb_lltabs tb = pgb_lltabs_default();
  uint64_t* key = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)D);
  double* wk = (double*)malloc(sizeof(double) * (size_t)D);
  if (!key || !wk) return 1;
  double o[PGB_ROWSUM_NOUT(PGB_ROWSUM_MAX_Q)];
  for (int64_t i = 0; i < n; ++i) {
    pgb_rowsum_column(a + i, ld, D, off ? off + i : NULL, transform, q, n_q, hdi_k, &tb, key, wk, o);
    for (int r = 0; r < PGB_ROWSUM_NOUT(n_q); ++r) out[(size_t)r * (size_t)n + (size_t)i] = o[r];
  }
  free(key);
  free(wk);
  return 0;
}
/* the sorted column itself, transformed: t[D] */
void rowsum_sorted(const double* a, int D, int64_t ld, const double* off, int transform, double* t) {
  const pgb_lltabs tb = pgb_lltabs_default();
  uint64_t* key = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)D);
  for (int d = 0; d < D; ++d) key[d] = pgb_rowsum_key(a[(int64_t)d * ld]);
  for (int start = D / 2 - 1; start >= 0; --start) pgb_rowsum_sift(key, start, D);
  for (int end = D - 1; end > 0; --end) {
    const uint64_t v = key[0];
    key[0] = key[end];
    key[end] = v;
    pgb_rowsum_sift(key, 0, end);
  }
  for (int d = 0; d < D; ++d) t[d] = pgb_rowsum_value(pgb_rowsum_unkey(key[d]), off != NULL, off ? *off : 0.0, transform, &tb);
  free(key);
}
double rowsum_value(double x, int transform) {
  const pgb_lltabs tb = pgb_lltabs_default();
  return pgb_rowsum_value(x, 0, 0.0, transform, &tb);
}
"""

TRANSFORMS = {"identity": 0, "exp": 1, "logistic": 2, "probit": 3}
SIGNATURES = {"rowsum_columns": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                           C.c_int, C.c_void_p]),
              "rowsum_sorted": (None, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
              "rowsum_value": (C.c_double, [C.c_double, C.c_int])}


def lib():
    return build("rowsum_host", SHIM, SIGNATURES)


def max_draws() -> int:
    return int(lib().rowsum_max_draws())


def max_q() -> int:
    return int(lib().rowsum_max_q())


def hdi_k(D: int, prob) -> int:
    return 0 if prob is None else max(int(np.floor(prob * D)), 1)


def summary(a, q=(), k: int = 0, transform="identity", offset=None) -> np.ndarray:
    """``(2 + Q + 2, n)`` = [mean, var, q..., hdi_lo, hdi_hi] of the columns of ``a`` (D, n): the header's
    pgb_rowsum_column with the integer ``k`` as hdi_k."""
    a = np.ascontiguousarray(a, np.float64)
    D, n = a.shape
    q = np.ascontiguousarray(q, np.float64)
    assert 2 <= D <= max_draws() and q.size <= max_q() and k >= 0
    off = None if offset is None else np.ascontiguousarray(offset, np.float64)
    assert off is None or off.shape == (n,)
    out = np.empty((2 + q.size + 2, n))
    code = transform if isinstance(transform, int) else TRANSFORMS[transform]
    assert lib().rowsum_columns(a.ctypes.data, D, n, n, None if off is None else off.ctypes.data, code,
                                q.ctypes.data if q.size else None, q.size, int(k), out.ctypes.data) == 0
    return out


def sorted_column(x, transform="identity", offset=None) -> np.ndarray:
    """The header's order of one vector, offset and transform applied: ``t[0 .. D)``."""
    x = np.ascontiguousarray(x, np.float64)
    t = np.empty(x.size)
    off = None if offset is None else C.byref(C.c_double(float(offset)))
    lib().rowsum_sorted(x.ctypes.data, x.size, 1, off, TRANSFORMS[transform], t.ctypes.data)
    return t


def value(x, transform) -> np.ndarray:
    """The header's transform of every element of ``x``."""
    L = lib()
    code = TRANSFORMS[transform]
    return np.array([L.rowsum_value(float(v), code) for v in np.ravel(x)]).reshape(np.shape(x))


def public(a, quantiles, hdi_prob, transform="identity", offset=None) -> dict:
    """The header's numbers in the layout of ``summarize_matrix``: arrays over the columns of ``a`` (D, n)."""
    q = np.asarray([] if quantiles is None else quantiles, np.float64)
    k = hdi_k(a.shape[0], hdi_prob)
    s = summary(a, q, k, transform, offset)
    return {"mean": s[0], "var": s[1], "sd": np.sqrt(s[1]), "quantiles": s[2:2 + q.size],
            "hdi": s[2 + q.size:4 + q.size] if k else None}
