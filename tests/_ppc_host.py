"""Host reference of the replicated observations: a small C shim around ``include/pgbart_ppc.h`` -- the header the
device kernel compiles -- built with gcc like ``tests/_rowsummary_host.py``.  It exports the header's ``pgb_ppc_value``
over a ``(D, K, n)`` array of predictors with the global index of its first row, the PIT counts and the flag counts.
``lib(max_tries=1)`` is a second build with ``-DPGB_PPC_MAX_TRIES=1``."""
import ctypes as C

import numpy as np

from _host_build import build
from pymc_bart_amd import _abi

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_ppc.h"
int ppc_max_tries(void) { return PGB_PPC_MAX_TRIES; }
double ppc_poisson_switch(void) { return PGB_PPC_POISSON_SWITCH; }
double ppc_max_rate(void) { return PGB_PPC_MAX_RATE; }
int ppc_rng_first(void) { return (int)PGB_PPC_RNG_FIRST; }
int ppc_rng_last(void) { return (int)PGB_PPC_RNG_LAST; }
int ppc_sampler_purposes(int* out) {
  out[0] = PGB_RNG_PROPOSE; out[1] = PGB_RNG_SELECT; out[2] = PGB_RNG_LEAF; out[3] = PGB_RNG_RESAMPLE;
  out[4] = PGB_RNG_FINAL; out[5] = PGB_RNG_MIX;
  return 6;
}
/* out[D][n] (or NULL) of mu[D][K][ld] (+ offset[K][ld]) at global rows row0 .. row0 + n; params[D][n_params] raw;
 * y[n] and pit[2][n] (added to) or NULL; flags[2] = (capped, exhausted) pairs.  Returns 1 + d when the params of draw d
 * are outside the family's domain. */
int ppc_fill(int family, int K, const double* mu, int D, int64_t n, int64_t ld, uint64_t row0, const double* params,
             int n_params, const double* offset, uint64_t seed, double* out, const double* y, int32_t* pit,
             int64_t* flags) {
  const pgb_lltabs tb = pgb_lltabs_default();
  flags[0] = flags[1] = 0;
  for (int d = 0; d < D; ++d) {
    double q[PGB_PW_NPAR];
    if (pgb_logpdf_prepare(family, params + (size_t)d * (size_t)n_params, q, &tb) != 0) return 1 + d;
    for (int64_t i = 0; i < n; ++i) {
      double m[PGB_MAX_OUTPUTS];
      for (int k = 0; k < K; ++k) {
        m[k] = mu[((size_t)d * (size_t)K + (size_t)k) * (size_t)ld + (size_t)i];
        if (offset) m[k] = m[k] + offset[(size_t)k * (size_t)ld + (size_t)i];
      }
      uint32_t fl = 0;
      const double v = pgb_ppc_value(family, K, m, q, seed, (uint32_t)d, row0 + (uint64_t)i, &tb, &fl);
      if (fl & PGB_PPC_CAPPED) ++flags[0];
      if (fl & PGB_PPC_EXHAUSTED) ++flags[1];
      if (out) out[(size_t)d * (size_t)n + (size_t)i] = v;
      if (y) {
        int below, equal;
        pgb_ppc_compare(v, y[i], &below, &equal);
        pit[i] += below;
        pit[(size_t)n + (size_t)i] += equal;
      }
    }
  }
  return 0;
}
"""

FAMILIES = {k: v for k, v in _abi.FAMILIES.items() if k not in ("callback", "compiled")}
SIGNATURES = {"ppc_fill": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_uint64, C.c_void_p,
                                     C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
              "ppc_poisson_switch": (C.c_double, None), "ppc_max_rate": (C.c_double, None)}


def lib(max_tries=None):
    return build("ppc_host", SHIM, SIGNATURES, () if max_tries is None else (f"-DPGB_PPC_MAX_TRIES={int(max_tries)}",))


def poisson_switch() -> float:
    return float(lib().ppc_poisson_switch())


def max_rate() -> float:
    return float(lib().ppc_max_rate())


def purposes():
    """-> (the header's purposes, the sampler's PGB_RNG_*)."""
    L = lib()
    buf = (C.c_int * 8)()
    n = L.ppc_sampler_purposes(buf)
    return list(range(L.ppc_rng_first(), L.ppc_rng_last() + 1)), [int(buf[i]) for i in range(n)]


def fill(family, mu, params=None, row0=0, seed=0, offset=None, y=None, values=True, max_tries=None):
    """``mu`` (D, K, n) [+ ``offset`` (K, n)], ``params`` (D, n_params) as the likelihood gives them -> (y_rep (D, n) or
    None, pit counts (2, n) int32 or None, (n_capped, n_exhausted))."""
    mu = np.ascontiguousarray(mu, np.float64)
    D, K, n = mu.shape
    code = family if isinstance(family, int) else FAMILIES[family]
    par = np.zeros((D, 0)) if params is None else np.ascontiguousarray(params, np.float64).reshape(D, -1)
    off = None if offset is None else np.ascontiguousarray(offset, np.float64).reshape(K, n)
    out = np.empty((D, n)) if values else None
    yy = None if y is None else np.ascontiguousarray(y, np.float64)
    assert yy is None or yy.shape == (n,)
    pit = None if y is None else np.zeros((2, n), np.int32)
    flags = np.zeros(2, np.int64)
    rc = lib(max_tries).ppc_fill(code, K, mu.ctypes.data, D, n, n, int(row0), par.ctypes.data if par.size else None,
                                 par.shape[1], None if off is None else off.ctypes.data, int(seed),
                                 None if out is None else out.ctypes.data, None if yy is None else yy.ctypes.data,
                                 None if pit is None else pit.ctypes.data, flags.ctypes.data)
    assert rc == 0, f"the params of draw {rc - 1} are outside the family's domain"
    return out, pit, (int(flags[0]), int(flags[1]))


def constant(family, mu, D, n, params=(), **kw):
    """``D x n`` values at the constant predictor(s) ``mu`` (a scalar or K values) and constant params."""
    m = np.atleast_1d(np.asarray(mu, np.float64))
    arr = np.broadcast_to(m[None, :, None], (D, m.size, n))
    par = np.broadcast_to(np.asarray(params, np.float64)[None, :], (D, len(params)))
    return fill(family, arr, par, **kw)
