"""Test helpers of the permutation importance tests (``test_permimp.py``, ``test_permimp_gpu.py``).

* :func:`perm` / :func:`use_lists` -- the host build of ``include/pgbart_permimp.h`` (the header the device kernel
  compiles) through a small C shim built with gcc: ``pgb_perm_index`` over a range of rows and the packer's CSR.
* :func:`recount` -- the use lists restated in NumPy from the definition (reachable nodes only).
* :func:`reference` -- the host reference of the value: ``f`` is the oracle backend's ``pgb_predict``; ``A`` and ``A'``
  are the oracle's ``pgb_predict`` called with the use list as a one-forest table of ``m = len(list)`` (the device's
  ``pgb_predict`` is bit-identical to it: ``test_predict_edges_gpu.py``); ``delta = A' - A`` and ``fperm = f + delta`` in
  NumPy -- one rounding each, as the header states.
* :func:`permuted_matrix` -- ``X`` with one column explicitly permuted.
* :func:`lengths_pool` -- a pool whose columns are used by 1, 3, 4, 8 and 9 trees of 12 (and one by none).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import _predict_exact as ex
from _host_build import build
from pymc_bart_amd import _abi
from pymc_bart_amd.trees import PosteriorSampler

PRED, DELTA = 0, 1

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_permimp.h"
unsigned permimp_rng(void) { return PGB_PERMIMP_RNG; }
int permimp_max_repeats(void) { return PGB_PERMIMP_MAX_REPEATS; }
void perm_range(uint64_t seed, uint32_t col, uint32_t rep, int64_t n, int64_t i0, int64_t cnt, int64_t* out) {
  for (int64_t i = 0; i < cnt; ++i) out[i] = pgb_perm_index(seed, col, rep, n, i0 + i);
}
/* the CSR: sizes first (off == NULL), then the copies */
int permimp_lists(const pgb_tree_arrays* trees, const int32_t* fidx, int m, int p, const int32_t* cols, int q,
                  const int32_t* picks, int n_picks, int64_t* n_list, int32_t* off, int32_t* list) {
  pgb_permimp_pack pk;
  const int rc = pgb_permimp_pack_build(trees, fidx, m, p, cols, q, picks, n_picks, &pk);
  if (rc) return rc;
  *n_list = pk.n_list;
  if (off) {
    memcpy(off, pgb_permimp_pack_off(&pk), sizeof(int32_t) * (size_t)(pk.n_lists + 1));
    memcpy(list, pgb_permimp_pack_list(&pk), sizeof(int32_t) * (size_t)pk.n_list);
  }
  pgb_permimp_pack_free(&pk);
  return 0;
}
"""

SIGNATURES = {"perm_range": (None, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
              "permimp_lists": (C.c_int, [C.POINTER(_abi.TreeArraysC), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]),
              "permimp_rng": (C.c_uint, []), "permimp_max_repeats": (C.c_int, [])}


def lib():
    return build("permimp_host", SHIM, SIGNATURES)


def perm(seed: int, col: int, rep: int, n: int, i0: int = 0, cnt: int | None = None) -> np.ndarray:
    """``pgb_perm_index(seed, col, rep, n, i)`` for ``i = i0 .. i0 + cnt`` (default: all of ``[0, n)``)."""
    cnt = n - i0 if cnt is None else cnt
    out = np.empty(cnt, np.int64)
    lib().perm_range(seed, col, rep, n, i0, cnt, out.ctypes.data)
    return out


def use_lists(pool, fidx, p: int, cols, picks=None):
    """``(off (n_picks * q + 1,), list)`` of the header's packer."""
    fidx = np.ascontiguousarray(fidx, np.int32)
    cols = np.ascontiguousarray(cols, np.int32)
    picks = np.ascontiguousarray(np.arange(fidx.shape[0]) if picks is None else picks, np.int32)
    carr = pool.as_c()
    nl = C.c_int64()
    args = (C.byref(carr), fidx.ctypes.data, fidx.shape[1], p, cols.ctypes.data, cols.size, picks.ctypes.data, picks.size)
    assert lib().permimp_lists(*args, C.byref(nl), None, None) == 0
    off, lst = np.zeros(picks.size * cols.size + 1, np.int32), np.zeros(max(nl.value, 1), np.int32)
    assert lib().permimp_lists(*args, C.byref(nl), off.ctypes.data, lst.ctypes.data) == 0
    return off, lst[:nl.value]


def tree_uses(pool, t: int, p: int) -> set:
    """The columns tree ``t`` uses: the splits of the nodes reachable from its root and the regressors of its
    reachable leaves."""
    base = int(pool.node_off[t])
    used, todo = set(), [0]
    while todo:
        g = base + todo.pop()
        if pool.var[g] >= 0:
            used.add(int(pool.var[g]))
            todo += [int(pool.left[g]), int(pool.right[g])]
        elif 0 <= int(pool.svar[g]) < p:
            used.add(int(pool.svar[g]))
    return used


def recount(pool, fidx, p: int, cols, picks=None):
    """The CSR of :func:`use_lists` from the definition."""
    fidx = np.asarray(fidx)
    picks = np.arange(fidx.shape[0]) if picks is None else np.asarray(picks)
    uses = [tree_uses(pool, t, p) for t in range(pool.n_trees)]
    off, lst = [0], []
    for d in picks:
        for c in cols:
            lst += [int(t) for t in fidx[d] if int(c) in uses[int(t)]]
            off.append(len(lst))
    return np.asarray(off, np.int32), np.asarray(lst, np.int32)


def predict(backend, pool, table, X) -> np.ndarray:
    """``pgb_predict`` of ``backend`` for every row of ``table``: ``(D, K, n)``."""
    table = np.ascontiguousarray(table, np.int32)
    s = PosteriorSampler(pool, table, table.shape[1], pool.n_outputs, backend=backend)
    return np.asarray(s.sample_posterior(np.ascontiguousarray(X, np.float64), list(range(table.shape[0])), None))


def permuted_matrix(X, col: int, seed: int, rep: int) -> np.ndarray:
    Xp = np.array(X, np.float64, copy=True)
    Xp[:, col] = Xp[perm(seed, col, rep, X.shape[0]), col]
    return Xp


def reference_block(oracle, pool, fidx, block, xcols, n_total: int, first_row: int, cols, R: int, seed: int, picks,
                    mode: int) -> np.ndarray:
    """``out[n_picks][q][R][K][nb]`` of ``pgb_predict_permuted`` from what the entry point is given: the block's rows
    and ``xcols`` ``(q, n_total)``, the chosen columns of the whole matrix."""
    block = np.ascontiguousarray(block, np.float64)
    nb, p = block.shape
    fidx = np.ascontiguousarray(fidx, np.int32)
    picks = np.asarray(picks)
    K = int(pool.n_outputs)
    f = predict(oracle, pool, fidx[picks], block)                       # (n_picks, K, nb)
    off, lst = use_lists(pool, fidx, p, cols, picks)
    out = np.empty((picks.size, len(cols), R, K, nb))
    for d in range(picks.size):
        for s, c in enumerate(cols):
            mine = lst[off[d * len(cols) + s]:off[d * len(cols) + s + 1]]
            A = predict(oracle, pool, mine[None, :], block)[0] if mine.size else np.zeros((K, nb))
            for r in range(R):
                Xp = block.copy()
                Xp[:, c] = xcols[s][perm(seed, int(c), r, n_total, first_row, nb)]
                Ap = predict(oracle, pool, mine[None, :], Xp)[0] if mine.size else np.zeros((K, nb))
                delta = Ap - A
                out[d, s, r] = delta if mode == DELTA else f[d] + delta
    return out


def reference(oracle, pool, fidx, X, first_row: int, nb: int, cols, R: int, seed: int, picks, mode: int) -> np.ndarray:
    """:func:`reference_block` on the rows ``first_row .. first_row + nb`` of the whole matrix ``X``."""
    X = np.ascontiguousarray(X, np.float64)
    xcols = np.ascontiguousarray(X[:, list(cols)].T)
    return reference_block(oracle, pool, fidx, X[first_row:first_row + nb], xcols, X.shape[0], first_row, cols, R, seed, picks,
                           mode)


# ------------------------------------------------------------------ a backend made of the host references
def _array(address, shape, dtype=np.float64):
    n = int(np.prod(shape))
    ct = {np.float64: C.c_double, np.int32: C.c_int32}[dtype]
    return np.ctypeslib.as_array((ct * n).from_address(int(address))).reshape(shape)


class HostBackend:
    """What ``permutation_importance`` asks of the HIP backend, answered on the host: ``pgb_predict`` is the oracle's,
    ``pgb_predict_permuted`` is :func:`reference_block`, the row reduce is the host build of its header
    (``_rowreduce_host``).  ``calls`` lists the ``(nb, q)`` of the ``pgb_predict_permuted`` calls."""

    def __init__(self, oracle, pool):
        from _oracle import NumpyMemory

        self.mem = NumpyMemory()
        self.lib = _HostLibrary(oracle, pool)
        self.calls = self.lib.calls


class _HostLibrary:
    backend_name = "hip-gfx950"
    path = "the host backend"

    def __init__(self, oracle, pool):
        import _rowreduce_host as rr

        self.calls = []
        self._oracle, self._pool, self._rr = oracle, pool, rr.lib()
        self.lib = oracle.lib.lib  # (pgb_predict: the oracle's)

    @staticmethod
    def check(rc, what):
        assert rc == 0, what

    def predict_permuted_entry_point(self):
        def call(carr, fidx, n_forests, m, xd, nb, p, ldx, xcols, n_total, first_row, cols, q, R, seed, picks, n_picks, f,
                 mode, out, stream):
            assert ldx == p and (f is None) == (mode == DELTA)
            table = _array(fidx, (n_forests, m), np.int32)
            cols_, picks_ = _array(cols, (q,), np.int32).copy(), _array(picks, (n_picks,), np.int32).copy()
            K = int(self._pool.n_outputs)
            got = reference_block(self._oracle, self._pool, table, _array(xd, (nb, p)), _array(xcols, (q, n_total)), n_total,
                                  first_row, cols_, R, seed, picks_, mode)
            if f is not None:  # (the caller's f is the one the reference computed)
                assert np.array_equal(_array(f, (n_picks, K, nb)), predict(self._oracle, self._pool, table[picks_], _array(xd, (nb, p))))
            _array(out, got.shape)[...] = got
            self.calls.append((int(nb), int(q)))
            return 0

        return call

    def rowreduce_entry_points(self):
        L = self._rr

        def reduce_(*a):
            L.rowred_block(*a[:-1])
            return 0

        def finish(*a):
            L.rowred_finish(*a[:-1])
            return 0

        return reduce_, finish, lambda D, K, G, has_y: 8 * L.rowred_ws_doubles(D, K, G, has_y)


LENGTHS = (1, 3, 4, 8, 9)  # both sides of PRED_WALKS = 4 and of its prefetch of the next four roots


def lengths_pool(rng, K: int, linear: bool = False):
    """Twelve trees over six columns: column ``j < 5`` is used by the first ``LENGTHS[j]`` trees, column 5 by none
    (``linear``: the leaves of tree 0 may regress on column 4 or 5 -- then 5 has a list of one).  Complete trees: every
    column of a tree is split on at every path."""
    roots = []
    for t in range(12):
        mine = [j for j in range(5) if t < LENGTHS[j]]
        if not mine:
            roots.append(ex.dyadic_leaf(rng, K, (), free=True))
        else:
            roots.append(ex.complete_tree(rng, K, len(mine), mine, lambda r, j: float(r.normal()),
                                          linear=(4, 5) if linear and t == 0 else (), counts="free"))
    return ex.build_pool(roots, K)
