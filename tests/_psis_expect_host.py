"""Host reference of the PSIS-weighted expectations: a small C shim around ``include/pgbart_psis.h`` -- the header the
device kernel compiles -- built with gcc like ``tests/_psis_host.py``.  It exports the header's
``pgb_psis_row_expect`` over the columns of two matrices."""
import ctypes as C

import numpy as np

from _host_build import build

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include "pgbart_psis.h"
double psis_g_max(void) { return PGB_PSIS_G_MAX; }
int psis_kind_value(void) { return PGB_PSIS_G_VALUE; }
int psis_kind_pit(void) { return PGB_PSIS_G_PIT; }
/* out[2 + n_e][n] = (elpd_loo_i, k_i, E_0[, E_1]) of the first n columns of ll[D][ld] and g[D][ldg] */
int psis_expect_rows(const double* ll, int D, int64_t n, int64_t ld, int M, const double* g, int64_t ldg, const double* y,
                     int kind, double* out) {
  const pgb_lltabs tb = pgb_lltabs_default();
  const int n_e = kind == PGB_PSIS_G_VALUE ? 2 : 1;
  double* wk = (double*)malloc(sizeof(double) * PGB_PSIS_WORK_DOUBLES(M));
  int32_t* iw = (int32_t*)malloc(sizeof(int32_t) * PGB_PSIS_WORK_INTS(M));
  if (!wk || !iw) return 1;
  for (int64_t i = 0; i < n; ++i) {
    double o[4];
    pgb_psis_row_expect(ll + i, ld, g + i, ldg, y ? y[i] : 0.0, kind, D, M, &tb, wk, iw, o);
    for (int c = 0; c < 2 + n_e; ++c) out[(size_t)c * (size_t)n + (size_t)i] = o[c];
  }
  free(wk);
  free(iw);
  return 0;
}
"""

KINDS = {"value": 0, "pit": 1}
SIGNATURES = {"psis_expect_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                             C.c_void_p, C.c_int, C.c_void_p]),
              "psis_g_max": (C.c_double, None)}


def lib():
    L = build("psis_expect_host", SHIM, SIGNATURES)
    assert L.psis_kind_value() == KINDS["value"] and L.psis_kind_pit() == KINDS["pit"]
    return L


def g_max() -> float:
    return float(lib().psis_g_max())


def expect(ll, g, M: int, y=None, kind: str = "value", n=None):
    """``(2 + n_e, n)`` = (elpd_loo_i, k_i, E_0[, E_1]) of the first ``n`` columns of ``ll`` (D, ld) and ``g``
    (D, ldg) with tail length ``M``: the header's pgb_psis_row_expect."""
    ll = np.ascontiguousarray(ll, np.float64)
    g = np.ascontiguousarray(g, np.float64)
    D, ld = ll.shape
    n = ld if n is None else int(n)
    assert g.shape[0] == D and g.shape[1] >= n and 1 <= M < D
    yy = None
    if kind == "pit":
        yy = np.ascontiguousarray(y, np.float64)
        assert yy.shape == (n,)
    out = np.empty((2 + (2 if kind == "value" else 1), n))
    rc = lib().psis_expect_rows(ll.ctypes.data, D, n, ld, int(M), g.ctypes.data, g.shape[1],
                                None if yy is None else yy.ctypes.data, KINDS[kind], out.ctypes.data)
    assert rc == 0
    return out
