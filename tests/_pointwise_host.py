"""Host reference of the pointwise log-likelihood: a small C shim around ``include/pgbart_logpdf.h`` -- the header the
device kernels compile -- built with gcc the way ``pymc_bart_amd/compiled.py`` builds host code (its flags,
``-ffp-contract=off``).  It exports the header's ``pgb_logpdf`` over rows and its reduction over draws."""
import ctypes as C

import numpy as np

from _host_build import build
from pymc_bart_amd import _abi

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#define PGB_COMPILED_NO_ENTRY_POINTS
#include "pgbart_logpdf.h"
int pw_chunk(void) { return PGB_PW_CHUNK; }
/* out[i] = the clamped log density of row i (mu is [K][n]); *n_clamped counts the rows that met the clamp; 1 when the
 * params are outside the family's domain */
int pw_logpdf_rows(int family, int K, int64_t n, const double* y, const double* mu, const double* params, double* out,
                   int64_t* n_clamped) {
  const pgb_lltabs tb = pgb_lltabs_default();
  double q[PGB_PW_NPAR];
  if (pgb_logpdf_prepare(family, params, q, &tb) != 0) return 1;
  int64_t nc = 0;
  for (int64_t i = 0; i < n; ++i) {
    double m[PGB_MAX_OUTPUTS];
    for (int k = 0; k < K; ++k) m[k] = mu[(size_t)k * (size_t)n + (size_t)i];
    const double raw = pgb_logpdf_raw(family, K, y[i], m, q, &tb);
    nc += pgb_pw_is_clamped(raw);
    out[i] = pgb_logpdf(family, K, y[i], m, q, &tb);
  }
  *n_clamped = nc;
  return 0;
}
/* out[3][n] = (lppd_i, mean_i, var_i) of ll[D][n] */
void pw_reduce(const double* ll, int D, int64_t n, double* out) {
  const pgb_lltabs tb = pgb_lltabs_default();
  for (int64_t i = 0; i < n; ++i) {
    double o3[3];
    pgb_pw_reduce(ll + i, n, D, &tb, o3);
    out[i] = o3[0];
    out[(size_t)n + i] = o3[1];
    out[2 * (size_t)n + i] = o3[2];
  }
}
double pw_clamp(double x) { return pgb_clamp_loglik(x); }
"""

SIGNATURES = {"pw_logpdf_rows": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_int64)]),
              "pw_reduce": (None, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]),
              "pw_clamp": (C.c_double, [C.c_double])}


def lib():
    return build("pw_host", SHIM, SIGNATURES)


def chunk() -> int:
    return int(lib().pw_chunk())


def logpdf(family: str, y, mu, params=(), return_clamped=False):
    """The header's clamped log density at ``y`` (n) and ``mu`` ((K, n) or (n,))."""
    y = np.ascontiguousarray(y, np.float64).ravel()
    mu = np.ascontiguousarray(np.atleast_2d(np.asarray(mu, np.float64)))
    K, n = mu.shape
    assert n == y.size
    prm = np.ascontiguousarray(np.concatenate([np.asarray(params, np.float64).ravel(), np.zeros(1)]))
    out = np.empty(n)
    nc = C.c_int64(0)
    rc = lib().pw_logpdf_rows(_abi.FAMILIES[family], K, n, y.ctypes.data, mu.ctypes.data, prm.ctypes.data,
                              out.ctypes.data, C.byref(nc))
    if rc != 0:
        raise ValueError(f"params {list(params)} are outside the domain of {family}")
    return (out, int(nc.value)) if return_clamped else out


def matrix(family: str, y, mu_draws, params=None, offset=None, return_clamped=False):
    """``mu_draws`` is (D, K, n) as ``sample_posterior`` returns it; ``params`` (D, n_params) or None."""
    mu_draws = np.asarray(mu_draws, np.float64)
    D = mu_draws.shape[0]
    out = np.empty((D, mu_draws.shape[2]))
    total = 0
    for d in range(D):
        mu = mu_draws[d] if offset is None else mu_draws[d] + np.asarray(offset, np.float64).reshape(mu_draws[d].shape)
        out[d], nc = logpdf(family, y, mu, () if params is None else params[d], return_clamped=True)
        total += nc
    return (out, total) if return_clamped else out


def reduce(ll):
    """(lppd_i, mean_i, var_i), each (n,), of the matrix ``ll`` (D, n): the header's chunked reduction."""
    ll = np.ascontiguousarray(ll, np.float64)
    D, n = ll.shape
    out = np.empty((3, n))
    lib().pw_reduce(ll.ctypes.data, D, n, out.ctypes.data)
    return out
