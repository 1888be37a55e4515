"""Test helpers of the SHAP interaction tests (``test_shap_interaction.py``, ``test_shap_interaction_gpu.py``) and of
``tools/shap_interaction_accuracy.py``; the pools, the leaves, the groups and the magnitude are ``_shap_host``'s.

* :func:`rows` -- the host build of ``include/pgbart_shap_interaction.h`` (the header the device kernel compiles)
  through a small C shim built with gcc, as ``_shap_host.lib()`` does it: the packer, the slot limit and
  ``pgb_shapx_row`` over rows and picks.
* :func:`brute_force` -- the definition: all ``2^p`` coalitions, each evaluated by ``_predict_exact.walk`` with the
  columns outside it excluded, combined with the interaction weights in ``Fraction`` arithmetic.
* :func:`leafwise` / :func:`restated` -- the header's leaf-wise form restated in Python over a number type: ``float``
  follows the stated order of operations (the bits of the header), ``Fraction`` is exact (and agrees with
  :func:`brute_force`).
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
from fractions import Fraction

import numpy as np

import _predict_exact as ex
import _shap_host as host
from _host_build import build
from pymc_bart_amd import _abi

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_shap_interaction.h"
int shapx_max_u(void) { return PGB_SHAPX_MAX_U; }
static int all_continuous(const pgb_tree_arrays* t) {
  if (!t->rule) return 1;
  for (int g = 0; g < t->total_nodes; ++g)
    if (t->var[g] >= 0 && t->rule[g] != PGB_RULE_CONTINUOUS) return 0;
  return 1;
}
/* the largest slot count over the leaves of the pool (negative: the packer's error) */
int shapx_slots(const pgb_tree_arrays* trees, int p) {
  pgb_shap_pack pk;
  const int rc = pgb_shap_pack_build(trees, p, &pk);
  if (rc) return rc;
  const int s = pgb_shapx_pack_slots(&pk);
  pgb_shap_pack_free(&pk);
  return s;
}
/* out[n_picks][K][q][q][n], base[n_picks][K]; general != 0: the rule dispatch even for a continuous pool; slow != 0: no
 * leaf takes the unrolled evaluation.  -3: a leaf has more than PGB_SHAPX_MAX_U slots */
int shapx_rows(const pgb_tree_arrays* trees, const int32_t* fidx, int m, const double* X, int64_t n, int p, int64_t ldx,
               const int32_t* cols, int q, const int32_t* picks, int n_picks, int general, int slow, double* out,
               double* base) {
  pgb_shap_pack pk;
  const int rc = pgb_shap_pack_build(trees, p, &pk);
  if (rc) return rc;
  if (pgb_shapx_pack_slots(&pk) > PGB_SHAPX_MAX_U) {
    pgb_shap_pack_free(&pk);
    return -3;
  }
  int32_t* pos = (int32_t*)malloc(sizeof(int32_t) * (size_t)p);
  for (int j = 0; j < p; ++j) pos[j] = -1;
  for (int c = 0; c < q; ++c) pos[cols[c]] = c;
  const int K = trees->n_outputs;
  const int lin = trees->slope && trees->xbar && trees->svar;
  const pgb_shap_view v = pgb_shap_pack_view(&pk, pk.buf, trees->value, lin ? trees->slope : NULL, K);
  const int cont = !general && all_continuous(trees);
  for (int s = 0; s < n_picks; ++s) {
    const int32_t* forest = fidx + (size_t)picks[s] * (size_t)m;
    pgb_shap_base(&v, forest, m, base + (size_t)s * K);
    for (int64_t i = 0; i < n; ++i)
      pgb_shapx_row(&v, forest, m, X + i * ldx, 1, cont, pos, q, slow, out + (size_t)s * K * q * q * n + i, n);
  }
  free(pos);
  pgb_shap_pack_free(&pk);
  return 0;
}
"""

SIGNATURES = {"shapx_rows": (C.c_int, [C.POINTER(_abi.TreeArraysC), C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int,
                                       C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p]),
              "shapx_slots": (C.c_int, [C.POINTER(_abi.TreeArraysC), C.c_int])}


def lib():
    return build("shapx_host", SHIM, SIGNATURES)


def max_u() -> int:
    return int(lib().shapx_max_u())


def slots(pool, p: int) -> int:
    carr = pool.as_c()
    return int(lib().shapx_slots(C.byref(carr), p))


def rows(pool, fidx, X, cols=None, picks=None, ldx=None, general: bool = False, slow: bool = False):
    """``(values (n_picks, K, q, q, n), base (n_picks, K))`` of the header's host build -- the layout of
    ``pgb_predict_shap_interactions``."""
    X = np.ascontiguousarray(X, np.float64)
    n, p = X.shape
    fidx = np.ascontiguousarray(fidx, np.int32)
    picks = np.ascontiguousarray(np.arange(fidx.shape[0]) if picks is None else picks, np.int32)
    cols = np.ascontiguousarray(np.arange(p) if cols is None else cols, np.int32)
    K, q = int(pool.n_outputs), int(cols.size)
    if ldx is not None and ldx != p:
        wide = np.full((n, ldx), 777.0)
        wide[:, :p] = X
        X = wide
    out = np.full((picks.size, K, q, q, n), np.nan)
    base = np.full((picks.size, K), np.nan)
    carr = pool.as_c()
    rc = lib().shapx_rows(C.byref(carr), fidx.ctypes.data, fidx.shape[1], X.ctypes.data, n, p, X.shape[1], cols.ctypes.data, q,
                          picks.ctypes.data, picks.size, int(general), int(slow), out.ctypes.data, base.ctypes.data)
    assert rc == 0, rc
    return out, base


# ------------------------------------------------------------------ the definition
def pair_weights(p: int):
    """``|S|! (p - |S| - 2)! / (2 (p - 1)!)`` for ``|S| = 0 .. p - 2``."""
    f = math.factorial
    return [Fraction(f(s) * f(p - s - 2), 2 * f(p - 1)) for s in range(p - 1)]


def brute_force(pool, fidx, X):
    """``(Phi (D, K, p, p, n), phi (D, K, p, n), base (D, K), R (D, K, n))`` in ``Fraction``: every coalition through
    ``walk``; ``phi`` the Shapley values of the same coalitions, ``Phi_ii = phi_i - sum_j Phi_ij``."""
    X = np.asarray(X, np.float64)
    n, p = X.shape
    fidx = np.asarray(fidx)
    D, K = fidx.shape[0], int(pool.n_outputs)
    v = {}
    for size in range(p + 1):
        for S in itertools.combinations(range(p), size):
            v[frozenset(S)] = ex.walk(pool, fidx, X, excluded=[j for j in range(p) if j not in S]).R
    W1 = host.shapley_weights(p)
    phi = np.empty((D, K, p, n), object)
    for j in range(p):
        acc = np.full((D, K, n), Fraction(0), object)
        for S, vs in v.items():
            if j not in S:
                acc = acc + W1[len(S)] * (v[S | {j}] - vs)
        phi[:, :, j, :] = acc
    W2 = pair_weights(p) if p > 1 else []
    Phi = np.full((D, K, p, p, n), Fraction(0), object)
    for i in range(p):
        for j in range(i + 1, p):
            acc = np.full((D, K, n), Fraction(0), object)
            for S, vs in v.items():
                if i not in S and j not in S:
                    acc = acc + W2[len(S)] * (v[S | {i, j}] - v[S | {i}] - v[S | {j}] + vs)
            Phi[:, :, i, j, :] = acc
            Phi[:, :, j, i, :] = acc
    for i in range(p):
        Phi[:, :, i, i, :] = phi[:, :, i, :] - sum(Phi[:, :, i, j, :] for j in range(p) if j != i)
    base = v[frozenset()]
    return Phi, phi, base[:, :, 0], v[frozenset(range(p))]


# ------------------------------------------------------------------ the leaf-wise form, restated
def _product(z, o, skip, N, n_coef):
    """The first ``n_coef`` coefficients of ``prod over e not in skip of (z_e + o_e t)``, in slot order: the header's
    recurrence."""
    c = [N(0)] * max(n_coef, 1)
    c[0] = N(1)
    for e in range(len(z)):
        if e in skip:
            continue
        for k in range(len(c) - 1, 0, -1):
            c[k] = c[k] * z[e] + c[k - 1] * o[e]
        c[0] = c[0] * z[e]
    return c


def _divide(full, ze, oe):
    """``full / (ze + oe t)`` exactly (``Fraction``; ``oe`` is 0 or 1, the factor is not 0)."""
    n = len(full) - 1
    if oe == 1:
        q = [Fraction(0)] * n
        q[n - 1] = full[n]
        for k in range(n - 1, 0, -1):
            q[k - 1] = full[k] - ze * q[k]
        return q
    return [full[k] / ze for k in range(n)]


def _term(z, o, cols, w, coef, Phi, N):
    """One term over the live slots ``z, o, cols`` in the header's order: r_e = g_e; the pairs i < j; the diagonal."""
    u = len(z)
    if u == 0:
        return

    def weights(n):
        W = [N(1) / N(n)]
        for k in range(1, n):
            W.append((W[-1] * N(k)) / N(n - k))
        return W

    W1, W2 = weights(u), (weights(u - 1) if u > 1 else [])
    exact = N is Fraction and u > 5          # Fractions only: one full product, the factors divided out
    full = _product(z, o, (), N, u + 1) if exact else None

    def others(skip):
        n_coef = u - len(skip) + 1           # (the header keeps u and u - 1 coefficients)
        if exact and all(not (z[e] == 0 and o[e] == 0) for e in skip):
            c = full
            for e in skip:
                c = _divide(c, z[e], o[e])
            return c
        return _product(z, o, skip, N, n_coef)

    r = []
    for e in range(u):
        c = others((e,))
        s = N(0)
        for k in range(u):
            s = s + W1[k] * c[k]
        r.append((o[e] - z[e]) * s)
    for i in range(u):
        for j in range(i + 1, u):
            c = others((i, j))
            s2 = N(0)
            for k in range(u - 1):
                s2 = s2 + W2[k] * c[k]
            h = N(1) / N(2) * (((o[i] - z[i]) * (o[j] - z[j])) * s2)
            r[i] = r[i] - h
            r[j] = r[j] - h
            for k, ck in enumerate(coef):
                Phi[k][cols[i]][cols[j]] = Phi[k][cols[i]][cols[j]] + (ck * w) * h
                Phi[k][cols[j]][cols[i]] = Phi[k][cols[j]][cols[i]] + (ck * w) * h
    for e in range(u):
        for k, ck in enumerate(coef):
            Phi[k][cols[e]][cols[e]] = Phi[k][cols[e]][cols[e]] + (ck * w) * r[e]


def leafwise(pool, forest, x, N=float):
    """``Phi [K][p][p]`` of one row and one forest by the header's leaf-wise form over the number type ``N``."""
    x = np.asarray(x, np.float64)
    p, K = x.shape[0], int(pool.n_outputs)
    value = np.asarray(pool.value, np.float64).reshape(-1, K)
    slope = np.asarray(pool.slope, np.float64).reshape(-1, K)
    Phi = [[[N(0)] * p for _ in range(p)] for _ in range(K)]
    for t in np.asarray(forest).tolist():
        for node, path in host.leaves(pool, int(t), N):
            z, o, cols = [], [], []
            w = N(1)
            for j, members in host.groups_of(path):
                zz = members[0][4]
                for mb in members[1:]:
                    zz = zz * mb[4]
                xv = float(x[j])
                if math.isnan(xv):
                    w = w * zz
                    continue
                on = all(ex._goes_left(mb[1], xv, mb[3]) == (mb[2] == 0) for mb in members)
                z.append(zz)
                o.append(N(1) if on else N(0))
                cols.append(j)
            _term(z, o, cols, w, [N(float(v)) for v in value[node]], Phi, N)
            js = int(pool.svar[node])
            if js < 0 or js >= p or math.isnan(float(x[js])):
                continue
            d = N(float(x[js])) - N(float(pool.xbar[node]))
            coef = [N(float(v)) * d for v in slope[node]]
            if js in cols:
                z[cols.index(js)] = N(0)
            else:
                z, o, cols = z + [N(0)], o + [N(1)], cols + [js]
            _term(z, o, cols, w, coef, Phi, N)
    return Phi


def restated(pool, fidx, X, N=float):
    """:func:`leafwise` over forests and rows: ``Phi (D, K, p, p, n)``."""
    X = np.asarray(X, np.float64)
    n, p = X.shape
    fidx = np.asarray(fidx)
    D, K = fidx.shape[0], int(pool.n_outputs)
    Phi = np.empty((D, K, p, p, n), np.float64 if N is float else object)
    for d in range(D):
        for i in range(n):
            ph = leafwise(pool, fidx[d], X[i], N)
            for k in range(K):
                for a in range(p):
                    Phi[d, k, a, :, i] = ph[k][a]
    return Phi
