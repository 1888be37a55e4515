"""Host reference of PSIS-LOO: a small C shim around ``include/pgbart_psis.h`` -- the header the device kernel
compiles -- built with gcc like ``tests/_pointwise_host.py``.  It exports the header's ``pgb_psis_row`` over the
columns of a matrix."""
import ctypes as C

import numpy as np

from _host_build import build

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include "pgbart_psis.h"
int psis_max_draws(void) { return PGB_PSIS_MAX_DRAWS; }
int psis_max_tail(void) { return PGB_PSIS_MAX_TAIL; }
/* out[2][n] = (elpd_loo_i, k_i) of ll[D][ld]'s first n columns */
int psis_rows(const double* ll, int D, int64_t n, int64_t ld, int M, double* out) {
  const pgb_lltabs tb = pgb_lltabs_default();
  double* wk = (double*)malloc(sizeof(double) * PGB_PSIS_WORK_DOUBLES(M));
  int32_t* iw = (int32_t*)malloc(sizeof(int32_t) * PGB_PSIS_WORK_INTS(M));
  if (!wk || !iw) return 1;
  for (int64_t i = 0; i < n; ++i) {
    double o2[2];
    pgb_psis_row(ll + i, ld, D, M, &tb, wk, iw, o2);
    out[i] = o2[0];
    out[(size_t)n + i] = o2[1];
  }
  free(wk);
  free(iw);
  return 0;
}
double psis_sqrt(double x) { const pgb_lltabs tb = pgb_lltabs_default(); return pgb_psis_sqrt(x, &tb); }
double psis_log1p(double x) { const pgb_lltabs tb = pgb_lltabs_default(); return pgb_psis_log1p(x, &tb); }
double psis_expm1(double x) { const pgb_lltabs tb = pgb_lltabs_default(); return pgb_psis_expm1(x, &tb); }
"""

SIGNATURES = {"psis_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p]),
              **{f: (C.c_double, [C.c_double]) for f in ("psis_sqrt", "psis_log1p", "psis_expm1")}}


def lib():
    return build("psis_host", SHIM, SIGNATURES)


def max_draws() -> int:
    return int(lib().psis_max_draws())


def max_tail() -> int:
    return int(lib().psis_max_tail())


def psis(ll, M: int):
    """(elpd_loo_i, k_i), each (n,), of the matrix ``ll`` (D, n) with tail length ``M``: the header's pgb_psis_row."""
    ll = np.ascontiguousarray(ll, np.float64)
    D, n = ll.shape
    assert 1 <= M < D and M <= max_tail() and 2 <= D <= max_draws()
    out = np.empty((2, n))
    assert lib().psis_rows(ll.ctypes.data, D, n, n, int(M), out.ctypes.data) == 0
    return out[0], out[1]
