"""Test helpers of the Shapley attribution tests (``test_shap.py``, ``test_shap_gpu.py``) and of
``tools/shap_accuracy.py``.

* :func:`rows` -- the host build of ``include/pgbart_shap.h`` (the header the device kernel compiles) through a small
  C shim built with gcc like ``tests/_rowsummary_host.py``: the packer and ``pgb_shap_row`` over rows and picks.
* :func:`records` -- the packer's leaf records and members as structured arrays.
* :func:`brute_force` -- the definition: all ``2^p`` coalitions, each evaluated by ``_predict_exact.walk`` with the
  columns outside it excluded, combined with the Shapley weights in ``Fraction`` arithmetic.
* :func:`leafwise` -- the header's leaf-wise form restated in Python over a number type: ``float`` follows the stated
  order of operations (the bits of the header), ``Fraction`` is exact (and agrees with :func:`brute_force`).
* :func:`magnitude` -- per entry ``M = sum |coef|`` over the leaf terms and their number ``T``.
* :func:`pools` -- the hand-built pools of the tests; :func:`chain_pool` -- one chain tree over distinct columns.
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
from fractions import Fraction

import numpy as np

import _predict_exact as ex
from _host_build import build
from _predict_exact import Leaf, Split
from pymc_bart_amd import _abi

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_shap.h"
int shap_max_u(void) { return PGB_SHAP_MAX_U; }
int shap_fast_u(void) { return PGB_SHAP_FAST_U; }
int shap_member_bytes(void) { return (int)sizeof(pgb_shap_member); }
int shap_leaf_bytes(void) { return (int)sizeof(pgb_shap_leaf); }
void shap_weights(int u, double* w) { pgb_shap_weights(u, w); }
static int all_continuous(const pgb_tree_arrays* t) {
  if (!t->rule) return 1;
  for (int g = 0; g < t->total_nodes; ++g)
    if (t->var[g] >= 0 && t->rule[g] != PGB_RULE_CONTINUOUS) return 0;
  return 1;
}
/* out[n_picks][K][p][n], base[n_picks][K]; general != 0: the rule dispatch even for a continuous pool */
int shap_rows(const pgb_tree_arrays* trees, const int32_t* fidx, int m, const double* X, int64_t n, int p, int64_t ldx,
              const int32_t* picks, int n_picks, int general, double* out, double* base) {
  pgb_shap_pack pk;
  const int rc = pgb_shap_pack_build(trees, p, &pk);
  if (rc) return rc;
  const int K = trees->n_outputs;
  const int lin = trees->slope && trees->xbar && trees->svar;
  const pgb_shap_view v = pgb_shap_pack_view(&pk, pk.buf, trees->value, lin ? trees->slope : NULL, K);
  const int cont = !general && all_continuous(trees);
  for (int s = 0; s < n_picks; ++s) {
    const int32_t* forest = fidx + (size_t)picks[s] * (size_t)m;
    pgb_shap_base(&v, forest, m, base + (size_t)s * K);
    for (int64_t i = 0; i < n; ++i)
      pgb_shap_row(&v, forest, m, X + i * ldx, 1, p, cont, out + (size_t)s * K * p * n + i, n);
  }
  pgb_shap_pack_free(&pk);
  return 0;
}
/* the records: counts first (leaf == NULL), then the copies */
int shap_records(const pgb_tree_arrays* trees, int p, int64_t* n_leaves, int64_t* n_members, void* leaf, void* member,
                 int32_t* off) {
  pgb_shap_pack pk;
  const int rc = pgb_shap_pack_build(trees, p, &pk);
  if (rc) return rc;
  *n_leaves = pk.n_leaves;
  *n_members = pk.n_members;
  if (leaf) {
    memcpy(leaf, pk.buf + pk.o_leaf, sizeof(pgb_shap_leaf) * (size_t)pk.n_leaves);
    memcpy(member, pk.buf + pk.o_member, sizeof(pgb_shap_member) * (size_t)pk.n_members);
    memcpy(off, pk.buf + pk.o_off, sizeof(int32_t) * ((size_t)pk.n_trees + 1));
  }
  pgb_shap_pack_free(&pk);
  return 0;
}
"""

MEMBER = np.dtype([("var", np.int32), ("rule", np.int32), ("side", np.int32), ("flags", np.int32),
                   ("split", np.float64), ("frac", np.float64)])
LEAF = np.dtype([("node", np.int32), ("first", np.int32), ("n_members", np.int32), ("n_groups", np.int32),
                 ("svar", np.int32), ("sgroup", np.int32), ("xbar", np.float64)])
HEAD, TAIL = 1, 2
SIGNATURES = {"shap_rows": (C.c_int, [C.POINTER(_abi.TreeArraysC), C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int,
                                      C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
              "shap_records": (C.c_int, [C.POINTER(_abi.TreeArraysC), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
              "shap_weights": (None, [C.c_int, C.c_void_p])}


def lib():
    L = build("shap_host", SHIM, SIGNATURES)
    assert L.shap_member_bytes() == MEMBER.itemsize and L.shap_leaf_bytes() == LEAF.itemsize
    return L


def max_u() -> int:
    return int(lib().shap_max_u())


def fast_u() -> int:
    return int(lib().shap_fast_u())


def weights(u: int) -> np.ndarray:
    w = np.zeros(u)
    lib().shap_weights(u, w.ctypes.data)
    return w


def rows(pool, fidx, X, picks=None, ldx=None, general: bool = False):
    """``(values (n_picks, K, p, n), base (n_picks, K))`` of the header's host build -- the layout of
    ``pgb_predict_shap``."""
    X = np.ascontiguousarray(X, np.float64)
    n, p = X.shape
    fidx = np.ascontiguousarray(fidx, np.int32)
    picks = np.ascontiguousarray(np.arange(fidx.shape[0]) if picks is None else picks, np.int32)
    K = int(pool.n_outputs)
    if ldx is not None and ldx != p:
        wide = np.full((n, ldx), 777.0)
        wide[:, :p] = X
        X = wide
    out = np.full((picks.size, K, p, n), np.nan)
    base = np.full((picks.size, K), np.nan)
    carr = pool.as_c()
    rc = lib().shap_rows(C.byref(carr), fidx.ctypes.data, fidx.shape[1], X.ctypes.data, n, p, X.shape[1], picks.ctypes.data,
                         picks.size, int(general), out.ctypes.data, base.ctypes.data)
    assert rc == 0, rc
    return out, base


def records(pool, p: int):
    """``(leaf records, members, tree_leaf_off)`` of the header's packer."""
    carr = pool.as_c()
    nl, nm = C.c_int64(), C.c_int64()
    assert lib().shap_records(C.byref(carr), p, C.byref(nl), C.byref(nm), None, None, None) == 0
    leaf, member = np.zeros(nl.value, LEAF), np.zeros(nm.value, MEMBER)
    off = np.zeros(pool.n_trees + 1, np.int32)
    assert lib().shap_records(C.byref(carr), p, C.byref(nl), C.byref(nm), leaf.ctypes.data, member.ctypes.data,
                              off.ctypes.data) == 0
    return leaf, member, off


# ------------------------------------------------------------------ the definition
def shapley_weights(p: int):
    f = math.factorial
    return [Fraction(f(s) * f(p - s - 1), f(p)) for s in range(p)]


def brute_force(pool, fidx, X):
    """``(phi (D, K, p, n), base (D, K), R (D, K, n))`` in ``Fraction``: every coalition through ``walk``."""
    X = np.asarray(X, np.float64)
    n, p = X.shape
    fidx = np.asarray(fidx)
    D, K = fidx.shape[0], int(pool.n_outputs)
    v = {}
    for size in range(p + 1):
        for S in itertools.combinations(range(p), size):
            v[frozenset(S)] = ex.walk(pool, fidx, X, excluded=[j for j in range(p) if j not in S]).R
    W = shapley_weights(p)
    phi = np.empty((D, K, p, n), object)
    for j in range(p):
        acc = np.full((D, K, n), Fraction(0), object)
        for S, vs in v.items():
            if j not in S:
                acc = acc + W[len(S)] * (v[S | {j}] - vs)
        phi[:, :, j, :] = acc
    base = v[frozenset()]
    for i in range(1, n):
        assert np.all(base[:, :, i] == base[:, :, 0])  # (the base value does not depend on the row)
    return phi, base[:, :, 0], v[frozenset(range(p))]


# ------------------------------------------------------------------ the leaf-wise form, restated
def leaves(pool, t: int, N=float):
    """The leaves of tree ``t`` depth-first, left first: ``(node, [(var, rule, side, split, frac)] in path order)``."""
    base = int(pool.node_off[t])
    out = []

    def rec(k, path):
        g = base + k
        if pool.var[g] < 0:
            out.append((g, list(path)))
            return
        l, r = int(pool.left[g]), int(pool.right[g])
        cl, cr = int(pool.count[base + l]), int(pool.count[base + r])
        tot = cl + cr
        for side, c, child in ((0, cl, l), (1, cr, r)):
            frac = N(c) / N(tot) if tot > 0 else N(0)
            rec(child, path + [(int(pool.var[g]), int(pool.rule[g]), side, float(pool.split[g]), frac)])

    rec(0, [])
    return out


def groups_of(path):
    """``[(column, [members in path order])]`` in order of first appearance."""
    cols = []
    for mb in path:
        if mb[0] not in cols:
            cols.append(mb[0])
    return [(j, [mb for mb in path if mb[0] == j]) for j in cols]


def _others(z, o, j, N, fast_exact):
    """The coefficients of ``prod over e != j of (z_e + o_e t)``, in slot order."""
    u = len(z)
    if fast_exact:  # Fractions only: the full product, the factor j divided out (recomputed when it is 0)
        full, zj, oj = fast_exact
        if oj == 1:
            q = [N(0)] * u
            q[u - 1] = full[u]
            for k in range(u - 1, 0, -1):
                q[k - 1] = full[k] - zj * q[k]
            return q
        if zj != 0:
            return [full[k] / zj for k in range(u)]
    c = [N(0)] * max(u, 1)
    c[0] = N(1)
    for e in range(u):
        if e == j:
            continue
        for k in range(len(c) - 1, 0, -1):
            c[k] = c[k] * z[e] + c[k - 1] * o[e]
        c[0] = c[0] * z[e]
    return c


def _term(z, o, cols, w, coef, phi, N):
    """One term over the live slots ``z, o, cols``: ``phi[k][col] += (coef_k * w) * g``."""
    u = len(z)
    if u == 0:
        return
    W = [N(1) / N(u)]
    for k in range(1, u):
        W.append((W[-1] * N(k)) / N(u - k))
    full = None
    if N is Fraction and u > 6:
        full = [N(0)] * (u + 1)
        full[0] = N(1)
        for e in range(u):
            for k in range(u, 0, -1):
                full[k] = full[k] * z[e] + full[k - 1] * o[e]
            full[0] = full[0] * z[e]
    for j in range(u):
        c = _others(z, o, j, N, (full, z[j], o[j]) if full is not None else None)
        s = N(0)
        for k in range(u):
            s = s + W[k] * c[k]
        g = (o[j] - z[j]) * s
        for k, ck in enumerate(coef):
            phi[k][cols[j]] = phi[k][cols[j]] + (ck * w) * g


def leafwise(pool, forest, x, N=float):
    """``(phi [K][p], base [K], M [K], T)`` of one row and one forest by the header's leaf-wise form over the number
    type ``N``; ``M`` (``Fraction``) and ``T``: the magnitude and the number of the leaf terms."""
    x = np.asarray(x, np.float64)
    p, K = x.shape[0], int(pool.n_outputs)
    value = np.asarray(pool.value, np.float64).reshape(-1, K)
    slope = np.asarray(pool.slope, np.float64).reshape(-1, K)
    phi = [[N(0)] * p for _ in range(K)]
    base = [N(0)] * K
    M, T = [Fraction(0)] * K, 0
    for t in np.asarray(forest).tolist():
        for node, path in leaves(pool, int(t), N):
            z, o, cols = [], [], []
            w, zall, first = N(1), N(1), True
            for j, members in groups_of(path):
                zz = members[0][4]
                for mb in members[1:]:
                    zz = zz * mb[4]
                zall = zz if first else zall * zz
                first = False
                xv = float(x[j])
                if math.isnan(xv):
                    w = w * zz
                    continue
                on = all(ex._goes_left(mb[1], xv, mb[3]) == (mb[2] == 0) for mb in members)
                z.append(zz)
                o.append(N(1) if on else N(0))
                cols.append(j)
            val = [N(float(v)) for v in value[node]]
            for k in range(K):
                base[k] = base[k] + val[k] * zall
                M[k] += abs(Fraction(float(value[node, k])))
            T += 1
            _term(z, o, cols, w, val, phi, N)
            js = int(pool.svar[node])
            if js < 0 or js >= p or math.isnan(float(x[js])):
                continue
            d = N(float(x[js])) - N(float(pool.xbar[node]))
            coef = [N(float(v)) * d for v in slope[node]]
            if js in cols:
                z[cols.index(js)] = N(0)
            else:
                z, o, cols = z + [N(0)], o + [N(1)], cols + [js]
            for k in range(K):
                M[k] += abs(Fraction(float(slope[node, k])) * (Fraction(float(x[js])) - Fraction(float(pool.xbar[node]))))
            T += 1
            _term(z, o, cols, w, coef, phi, N)
    return phi, base, M, T


def restated(pool, fidx, X, N=float):
    """:func:`leafwise` over forests and rows: ``(phi (D, K, p, n), base (D, K), M (D, K, n), T (D, n))``."""
    X = np.asarray(X, np.float64)
    n, p = X.shape
    fidx = np.asarray(fidx)
    D, K = fidx.shape[0], int(pool.n_outputs)
    dt = np.float64 if N is float else object
    phi, base = np.empty((D, K, p, n), dt), np.empty((D, K), dt)
    M, T = np.empty((D, K, n), object), np.zeros((D, n), np.int64)
    for d in range(D):
        for i in range(n):
            ph, b, m_, t_ = leafwise(pool, fidx[d], X[i], N)
            for k in range(K):
                phi[d, k, :, i] = ph[k]
                M[d, k, i] = m_[k]
            base[d] = b
            T[d, i] = t_
    return phi, base, M, T


def magnitude(pool, fidx, X):
    """Per entry ``M`` (D, K, n) -- the sum of ``|coef|`` over the leaf terms of the forest, rounded up to a double --
    and their number ``T`` (D, n): a leaf's value, and its slope times ``x - xbar`` when it regresses on a column
    whose value is not NaN."""
    X = np.asarray(X, np.float64)
    n, p = X.shape
    fidx = np.asarray(fidx)
    D, K = fidx.shape[0], int(pool.n_outputs)
    value = np.asarray(pool.value, np.float64).reshape(-1, K)
    slope = np.asarray(pool.slope, np.float64).reshape(-1, K)
    M, T = np.zeros((D, K, n)), np.zeros((D, n), np.int64)
    for d in range(D):
        for i in range(n):
            acc = [Fraction(0)] * K
            for t in fidx[d].tolist():
                for g, _ in leaves(pool, int(t)):
                    js = int(pool.svar[g])
                    lin = 0 <= js < p and not math.isnan(float(X[i, js]))
                    T[d, i] += 1 + int(lin)
                    for k in range(K):
                        acc[k] += abs(Fraction(float(value[g, k])))
                        if lin:
                            acc[k] += abs(Fraction(float(slope[g, k])) * (Fraction(float(X[i, js])) - Fraction(float(pool.xbar[g]))))
            for k in range(K):
                M[d, k, i] = np.nextafter(float(acc[k]), np.inf)
    return M, T


# ------------------------------------------------------------------ pools
def _split_of(rules):
    def f(rng, j):
        rule = rules.get(j, ex.CONT)
        if rule == ex.ONEHOT:
            return float(rng.integers(0, 4))
        if rule == ex.SUBSET:
            return float(int(rng.integers(1, 64)))
        return float(ex.dyadic(rng, 2, 1.0))
    return f


def _zero_counts(pool, pairs):
    """Set the training counts of the children of the ``k``-th split nodes of the pool: ``pairs`` = [(k, cl, cr)]."""
    splits = np.flatnonzero(np.asarray(pool.var) >= 0)
    tree_of = np.searchsorted(np.asarray(pool.node_off), splits, side="right") - 1
    for k, cl, cr in pairs:
        g = int(splits[k % splits.size])
        base = int(pool.node_off[tree_of[k % splits.size]])
        pool.count[base + int(pool.left[g])] = cl
        pool.count[base + int(pool.right[g])] = cr


def _rows_for(rng, n, p, rules, nan_rate=0.15):
    X = ex.dyadic(rng, 2, 1.5, size=(n, p)).astype(np.float64)
    for j, rule in rules.items():
        X[:, j] = rng.integers(0, 6 if rule == ex.SUBSET else 4, size=n)
    X[rng.random((n, p)) < nan_rate] = np.nan
    return X


def pools():
    """``[(name, pool, forest table, X)]``: mixed rules with linear leaves on and off split columns (K = 3), the
    edges (K = 1: -0.0 against a split at 0.0, infinities, a stump, an unused column, repeated columns on a path),
    zero-count siblings in both, NaN entries in both."""
    out = []
    rng = np.random.default_rng(2718)
    rules = {1: ex.ONEHOT, 3: ex.SUBSET}
    roots = [ex.dyadic_tree(rng, 3, 5, [0, 1, 2, 3], _split_of(rules), grow=0.8, linear=(0, 4), counts="free", rules=rules)
             for _ in range(6)]
    pool = ex.build_pool(roots, 3)
    _zero_counts(pool, [(1, 0, 5), (4, 0, 0), (7, 3, 0)])
    X = _rows_for(rng, 10, 5, rules)
    X[0] = [0.25, 1.0, -0.0, 2.0, 0.5]          # a row without a missing value
    X[1, 4] = np.nan                            # a missing regressor off the split columns
    X[2, 0] = np.nan                            # ... and one on them
    out.append(("mixed-K3", pool, np.array([[0, 1, 2], [3, 4, 5], [5, 0, 0]], np.int32), X))

    rng = np.random.default_rng(3141)

    def leaf(v, svar=-1, slope=0.0, xbar=0.0, count=8):
        return Leaf([v], count=count, svar=svar, slope=[slope], xbar=xbar)

    roots = [
        Split(0, 0.0, leaf(1.5, count=3), leaf(-2.25, count=5)),                          # -0.0 <= 0.0 goes left
        Split(1, 0.5, Split(1, -math.inf, leaf(4.0, count=1), leaf(0.75, count=2), count=3),
              Split(0, 0.25, leaf(-1.0, count=4), Split(1, math.inf, leaf(2.0, count=6), leaf(8.0, count=0), count=6), count=10)),
        leaf(3.25),                                                                       # a stump: u = 0
        Split(2, 0.5, leaf(1.0, svar=2, slope=0.5, xbar=0.25, count=0), leaf(-1.0, svar=0, slope=-1.5, xbar=1.0, count=0)),
        Split(0, -0.5, Split(2, 0.0, leaf(0.5, count=0), leaf(2.5, count=7), count=7), leaf(-3.0, svar=2, slope=2.0, xbar=-1.0, count=9)),
    ]
    pool = ex.build_pool(roots, 1)
    X = np.array([[-0.0, 0.0, 1.0, 9.0], [0.0, -math.inf, 0.5, 9.0], [5e-324, math.inf, 0.25, -9.0], [-1.0, 0.5, -0.0, 0.0],
                  [math.nan, 1.0, 0.75, 1.0], [0.25, math.nan, math.nan, 1.0], [math.nan, math.nan, math.nan, math.nan],
                  [-0.5, 0.75, 0.0, math.nan]])
    out.append(("edges-K1", pool, np.array([[0, 1, 2, 3, 4], [2, 2, 2, 2, 2], [1, 1, 4, 4, 3]], np.int32), X))
    return out


def chain_pool(depth: int, K: int = 1, seed: int = 5, side: str = "left", linear=(), counts: str = "free"):
    """One chain tree of ``depth`` splits over the distinct columns ``0 .. depth - 1`` (``x <= v`` splits at dyadic
    values) and rows that follow the chain to different depths: ``(pool, forest table (1, 1), X (n, depth))``."""
    rng = np.random.default_rng(seed + depth)
    root = ex.chain_tree(rng, K, depth, list(range(depth)), lambda r, j: float(ex.dyadic(r, 2, 1.0)), side, linear=linear,
                         counts=counts)
    pool = ex.build_pool([root], K)
    return pool, np.zeros((1, 1), np.int32), rng


def chain_rows(pool, depth: int, p: int, rng, n: int = 3):
    """Rows for :func:`chain_pool`: row 0 follows the chain to its end, the others leave it at random depths; one
    NaN in the last row."""
    splits = {int(pool.var[g]): float(pool.split[g]) for g in range(pool.total_nodes) if pool.var[g] >= 0}
    left_is_on = pool.var[int(pool.left[0])] >= 0 if depth > 1 else True
    X = np.zeros((n, p))
    for i in range(n):
        stay = depth if i == 0 else int(rng.integers(0, depth))
        for j in range(depth):
            on = j < stay or rng.random() < 0.5
            go_left = on == bool(left_is_on)
            X[i, j] = splits[j] - 0.25 if go_left else splits[j] + 0.25
        X[i, depth:] = rng.normal(size=p - depth)
    if n > 1:
        X[n - 1, depth // 2] = np.nan
    return X
