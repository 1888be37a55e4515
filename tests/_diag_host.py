"""Host reference of the chain diagnostics: a small C shim around ``include/pgbart_diag.h`` -- the header the device
kernel compiles -- built with gcc like ``tests/_rowsummary_host.py``.  It exports the header's ``pgb_diag_column`` over
the columns of a matrix, and the pieces the exact tests look at."""
import ctypes as C
import math

import numpy as np

from _host_build import build

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include "pgbart_diag.h"
int diag_max_draws(void) { return PGB_DIAG_MAX_DRAWS; }
int diag_max_draws_mean(void) { return PGB_DIAG_MAX_DRAWS_MEAN; }
int diag_max_chains(void) { return PGB_DIAG_MAX_CHAINS; }
int diag_nout(void) { return PGB_DIAG_NOUT; }
/* out[PGB_DIAG_NOUT][n] of a[n_chains n_per_chain][ld]'s first n columns */
int diag_columns(const double* a, int n_chains, int n_per_chain, int64_t n, int64_t ld, int transform, int stats,
                 const double* z, double tau_floor, double* out) {
  const int h = n_per_chain / 2, J = 2 * n_chains, S = J * h;
  uint64_t* key = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)S);
  double* wk = (double*)malloc(sizeof(double) * (3 * (size_t)S + 3 * (size_t)J));
  if (!key || !wk) return 1;
  double o[PGB_DIAG_NOUT];
  for (int64_t i = 0; i < n; ++i) {
    pgb_diag_column(a + i, ld, n_chains, n_per_chain, transform, stats, z, tau_floor, pgb_tab_exp(), key, wk, wk + S,
                    wk + 2 * (size_t)S, wk + 3 * (size_t)S, o);
    for (int r = 0; r < PGB_DIAG_NOUT; ++r) out[(size_t)r * (size_t)n + (size_t)i] = o[r];
  }
  free(key);
  free(wk);
  return 0;
}
double diag_exp(double x) { return pgb_exp_t(x, pgb_tab_exp()); }
/* the average ranks (1-based) of x[0 .. S) by the header's order and searches */
void diag_ranks(const double* x, int S, double* rank) {
  uint64_t* key = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)S);
  double* t = (double*)malloc(sizeof(double) * (size_t)S);
  for (int p = 0; p < S; ++p) t[p] = pgb_diag_x(x[p], PGB_DIAG_IDENTITY, 0.0, NULL);
  pgb_diag_sort(t, S, key);
  for (int p = 0; p < S; ++p) {
    const uint64_t k = pgb_rowsum_key(pgb_diag_x(x[p], PGB_DIAG_IDENTITY, 0.0, NULL));
    rank[p] = (double)(pgb_diag_lower(t, S, k) + pgb_diag_upper(t, S, k) + 1) / 2.0;
  }
  free(key);
  free(t);
}
"""

TRANSFORMS = {"identity": 0, "exp_shift": 1}
ALL, MEAN_ONLY = 0, 1
ROWS = ("rhat2_bulk", "rhat2_folded", "ess_bulk", "ess_tail_lo", "ess_tail_hi", "ess_mean", "mean", "var", "constant",
        "reserved")
SIGNATURES = {"diag_columns": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                         C.c_double, C.c_void_p]),
              "diag_exp": (C.c_double, [C.c_double]), "diag_ranks": (None, [C.c_void_p, C.c_int, C.c_void_p])}


def lib():
    return build("diag_host", SHIM, SIGNATURES)


def max_draws() -> int:
    return int(lib().diag_max_draws())


def max_draws_mean() -> int:
    return int(lib().diag_max_draws_mean())


def max_chains() -> int:
    return int(lib().diag_max_chains())


def kept(n_chains: int, n_per_chain: int) -> int:
    return 2 * n_chains * (n_per_chain // 2)


def columns(a, n_chains: int, transform="identity", stats: int = ALL, z=None, tau_floor=None) -> np.ndarray:
    """``(10, n)`` of the columns of ``a`` (n_chains * n_per_chain, n): the header's pgb_diag_column, with the z table
    and the floor of ``pymc_bart_amd.diagnostics`` unless given."""
    from pymc_bart_amd import diagnostics

    a = np.ascontiguousarray(a, np.float64)
    D, n = a.shape
    assert D % n_chains == 0
    npc = D // n_chains
    S = kept(n_chains, npc)
    assert npc >= 4 and n_chains <= max_chains() and S <= (max_draws_mean() if stats == MEAN_ONLY else max_draws())
    if z is None:
        z = diagnostics.z_table(S)
    z = np.ascontiguousarray(z, np.float64)
    assert z.shape == (2 * S - 1,)
    if tau_floor is None:
        tau_floor = 1.0 / math.log10(S)
    out = np.empty((int(lib().diag_nout()), n))
    code = transform if isinstance(transform, int) else TRANSFORMS[transform]
    assert lib().diag_columns(a.ctypes.data, n_chains, npc, n, n, code, int(stats), z.ctypes.data, float(tau_floor),
                              out.ctypes.data) == 0
    return out


def exp_t(x) -> np.ndarray:
    """The header's ``pgb_exp_t`` of every element of ``x``."""
    L = lib()
    return np.array([L.diag_exp(float(v)) for v in np.ravel(x)]).reshape(np.shape(x))


def ranks(x) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float64)
    r = np.empty(x.size)
    lib().diag_ranks(x.ctypes.data, x.size, r.ctypes.data)
    return r


def public(a, n_chains: int, transform="identity") -> dict:
    """The header's numbers in the layout of ``diagnose_matrix``: arrays over the columns of ``a``."""
    s = columns(a, n_chains, transform)
    return {"rhat": np.sqrt(np.maximum(s[0], s[1])), "ess_bulk": s[2], "ess_tail": np.minimum(s[3], s[4]), "ess_mean": s[5],
            "mcse_mean": np.sqrt(s[7] / s[5]), "mean": s[6], "sd": np.sqrt(s[7]), "n_constant": int(np.sum(s[8] != 0.0))}
