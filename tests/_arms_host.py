"""Test helpers of the decision tests (``test_decision.py``, ``test_decision_gpu.py``).

* :func:`union_lists` / :func:`recount` -- the packer of ``include/pgbart_arms.h`` (the header the device kernels compile)
  through a small C shim built with gcc, and the same lists restated in NumPy from the definition.
* :func:`reference_block` -- the host reference of ``pgb_predict_arms``: the packer's lists, the oracle's ``pgb_predict``
  with each list as a one-forest table of ``m = len(list)`` at the row and at each ``x^a`` (the device's ``pgb_predict``
  is bit-identical to the oracle's: ``test_predict_edges_gpu.py``), ``delta = A_a - A_self`` and ``f_a = f + delta`` in
  NumPy -- one rounding each, as the header states.
* :func:`decide` -- ``pgb_arms_block`` (per chunk of rows) and ``pgb_arms_finish`` from the header.
* :func:`numpy_decision` -- the whole decision restated in NumPy from plain predictions, for pools whose sums are exact.
* :class:`HostBackend` -- a backend made of the host references, so that the Python layer runs without a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import _permimp_host as permimp
from _host_build import build
from pymc_bart_amd import _abi

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_arms.h"
int arms_max_cols(void) { return PGB_ARMS_MAX_COLS; }
int arms_max(void) { return PGB_ARMS_MAX; }
int64_t arms_ws_doubles(int D, int G, int A) { return pgb_arms_ws_doubles(D, G, A); }
int arms_better(double a, double b) { return pgb_arms_better(a, b); }
/* the CSR: sizes first (off == NULL), then the copies */
int arms_lists(const pgb_tree_arrays* trees, const int32_t* fidx, int m, int p, const int32_t* cols, int s,
               const int32_t* picks, int n_picks, int64_t* n_list, int32_t* off, int32_t* list) {
  pgb_arms_pack pk;
  const int rc = pgb_arms_pack_build(trees, fidx, m, p, cols, s, picks, n_picks, &pk);
  if (rc) return rc;
  *n_list = pk.n_list;
  if (off) {
    memcpy(off, pgb_arms_pack_off(&pk), sizeof(int32_t) * (size_t)(pk.n_lists + 1));
    memcpy(list, pgb_arms_pack_list(&pk), sizeof(int32_t) * (size_t)pk.n_list);
  }
  pgb_arms_pack_free(&pk);
  return 0;
}
void arms_block(const double* f, int64_t lda, int64_t ldd, int D, int A, int64_t nb, const double* w, const int32_t* g,
                const int32_t* policy, const double* off, const double* cost, double sign, int transform, int G,
                int64_t first_row, int init, double* ws, int32_t* nbest, double* mean, double* regret, int32_t* bayes) {
  const pgb_lltabs tb = pgb_lltabs_default();
  pgb_arms_block(f, lda, ldd, D, A, nb, w, g, policy, off, cost, sign, transform, G, first_row, init, &tb, ws, nbest, mean,
                 regret, bayes);
}
void arms_finish(const double* ws, int D, int G, int A, double* out, double* w_out, int64_t* counts) {
  pgb_arms_finish(ws, D, G, A, out, w_out, counts);
}
/* the whole call in one block, through the header's own pgb_arms_call */
void arms_call(const double* f, int64_t lda, int64_t ldd, int D, int A, int64_t n, const double* w, const int32_t* g,
               const int32_t* policy, const double* off, const double* cost, double sign, int transform, int G, double* ws,
               int32_t* nbest, double* mean, double* regret, int32_t* bayes, double* out, double* w_out, int64_t* counts) {
  const pgb_lltabs tb = pgb_lltabs_default();
  pgb_arms_call(f, lda, ldd, D, A, n, w, g, policy, off, cost, sign, transform, G, &tb, ws, nbest, mean, regret, bayes, out,
                w_out, counts);
}
"""

P = C.c_void_p
_BLOCK = [P, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64, P, P, P, P, P, C.c_double, C.c_int, C.c_int]
SIGNATURES = {"arms_max_cols": (C.c_int, []), "arms_max": (C.c_int, []),
              "arms_ws_doubles": (C.c_int64, [C.c_int] * 3), "arms_better": (C.c_int, [C.c_double, C.c_double]),
              "arms_lists": (C.c_int, [C.POINTER(_abi.TreeArraysC), P, C.c_int, C.c_int, P, C.c_int, P, C.c_int,
                                       C.POINTER(C.c_int64), P, P]),
              "arms_block": (None, _BLOCK + [C.c_int64, C.c_int, P, P, P, P, P]),
              "arms_finish": (None, [P, C.c_int, C.c_int, C.c_int, P, P, P]),
              "arms_call": (None, _BLOCK + [P, P, P, P, P, P, P, P])}
TRANSFORMS = {"identity": 0, "exp": 1, "logistic": 2, "probit": 3}


def lib():
    return build("arms_host", SHIM, SIGNATURES)


def ws_doubles(D: int, G: int, A: int) -> int:
    return int(lib().arms_ws_doubles(D, G, A))


def union_lists(pool, fidx, p: int, cols, picks=None):
    """``(off (n_picks + 1,), list)`` of the header's packer."""
    fidx = np.ascontiguousarray(fidx, np.int32)
    cols = np.ascontiguousarray(cols, np.int32)
    picks = np.ascontiguousarray(np.arange(fidx.shape[0]) if picks is None else picks, np.int32)
    carr = pool.as_c()
    nl = C.c_int64()
    args = (C.byref(carr), fidx.ctypes.data, fidx.shape[1], p, cols.ctypes.data, cols.size, picks.ctypes.data, picks.size)
    assert lib().arms_lists(*args, C.byref(nl), None, None) == 0
    off, lst = np.zeros(picks.size + 1, np.int32), np.zeros(max(nl.value, 1), np.int32)
    assert lib().arms_lists(*args, C.byref(nl), off.ctypes.data, lst.ctypes.data) == 0
    return off, lst[:nl.value]


def recount(pool, fidx, p: int, cols, picks=None):
    """The CSR of :func:`union_lists` from the definition: reachable nodes only (``_permimp_host.tree_uses``)."""
    fidx = np.asarray(fidx)
    picks = np.arange(fidx.shape[0]) if picks is None else np.asarray(picks)
    named = {int(c) for c in cols}
    uses = [bool(permimp.tree_uses(pool, t, p) & named) for t in range(pool.n_trees)]
    off, lst = [0], []
    for d in picks:
        lst += [int(t) for t in fidx[d] if uses[int(t)]]
        off.append(len(lst))
    return np.asarray(off, np.int32), np.asarray(lst, np.int32)


def arm_copy(X, cols, arm) -> np.ndarray:
    """``x^a`` for every row: ``X`` with ``cols`` overwritten by the arm's values."""
    Xa = np.array(X, np.float64, copy=True)
    Xa[:, list(cols)] = np.asarray(arm, np.float64)
    return Xa


def reference_block(oracle, pool, fidx, block, cols, arms, picks, f=None):
    """``(out (A, n_picks, K, nb), list lengths (n_picks,))`` of ``pgb_predict_arms`` from what the entry point is
    given; ``f``: what the caller hands in as ``f_dev`` (default: the oracle's ``pgb_predict``)."""
    block = np.ascontiguousarray(block, np.float64)
    nb, p = block.shape
    fidx = np.ascontiguousarray(fidx, np.int32)
    picks = np.asarray(picks)
    arms = np.asarray(arms, np.float64).reshape(-1, len(cols))
    K = int(pool.n_outputs)
    if f is None:
        f = permimp.predict(oracle, pool, fidx[picks], block)            # (n_picks, K, nb)
    off, lst = union_lists(pool, fidx, p, cols, picks)
    out = np.empty((arms.shape[0], picks.size, K, nb))
    for d in range(picks.size):
        mine = lst[off[d]:off[d + 1]]
        A_self = permimp.predict(oracle, pool, mine[None, :], block)[0] if mine.size else np.zeros((K, nb))
        for a in range(arms.shape[0]):
            A_a = permimp.predict(oracle, pool, mine[None, :], arm_copy(block, cols, arms[a]))[0] if mine.size else np.zeros((K, nb))
            delta = A_a - A_self
            out[a, d] = f[d] + delta
    return out, np.diff(off).astype(np.int32)


def _p(x):
    return None if x is None else x.ctypes.data


def _f(x):
    return None if x is None else np.ascontiguousarray(x, np.float64)


def _i(x):
    return None if x is None else np.ascontiguousarray(x, np.int32)


def decide(f, w, g, G, policy=None, off=None, cost=None, sign=1.0, transform="identity", chunk=None, whole_call=False) -> dict:
    """The header on the predictions ``f`` ``(A, D, n)`` (any strides along the first two axes that are multiples of the
    item size; the last axis contiguous).  ``chunk``: rows per block (a multiple of 64; ``None``: all at once), the
    partials carried from block to block; ``whole_call``: through ``pgb_arms_call``.  -> ``nbest``, ``mean``,
    ``regret`` ``(A, n)``, ``bayes`` ``(n,)``, ``out`` ``(4 + 2 A, D, G)``, ``W`` ``(G,)``, ``counts`` ``(3,)`` and the
    workspace ``ws``."""
    L = lib()
    A, D, n = f.shape
    assert f.dtype == np.float64 and f.strides[2] == 8
    w, off, cost, g, policy = _f(w), _f(off), _f(cost), _i(g), _i(policy)
    code = transform if isinstance(transform, int) else TRANSFORMS[transform]
    ws = np.full(ws_doubles(D, G, A), 7.5)                              # (init must clear it)
    nbest, mean, regret, bayes = np.empty((A, n), np.int32), np.empty((A, n)), np.empty((A, n)), np.empty(n, np.int32)
    out, W, counts = np.empty((4 + 2 * A, D, G)), np.empty(G), np.zeros(3, np.int64)
    if whole_call:
        L.arms_call(f.ctypes.data, f.strides[0] // 8, f.strides[1] // 8, D, A, n, _p(w), _p(g), _p(policy), _p(off), _p(cost),
                    sign, code, G, _p(ws), _p(nbest), _p(mean), _p(regret), _p(bayes), _p(out), _p(W), _p(counts))
    else:
        step = n if chunk is None else int(chunk)
        assert step == n or step % 64 == 0
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            nb = r1 - r0
            blk = lambda m: None if m is None else np.ascontiguousarray(m[..., r0:r1])  # noqa: E731
            fb = blk(f)
            nbb, mb, rb, bb = np.empty((A, nb), np.int32), np.empty((A, nb)), np.empty((A, nb)), np.empty(nb, np.int32)
            L.arms_block(_p(fb), D * nb, nb, D, A, nb, _p(blk(w)), _p(blk(g)), _p(blk(policy)), _p(blk(off)), _p(cost), sign,
                         code, G, r0, int(r0 == 0), _p(ws), _p(nbb), _p(mb), _p(rb), _p(bb))
            nbest[:, r0:r1], mean[:, r0:r1], regret[:, r0:r1], bayes[r0:r1] = nbb, mb, rb, bb
        L.arms_finish(_p(ws), D, G, A, _p(out), _p(W), _p(counts))
    return {"nbest": nbest, "mean": mean, "regret": regret, "bayes": bayes, "out": out, "W": W, "counts": counts, "ws": ws}


def numpy_decision(f, w, gid, G, policy=None, cost=None, sign=1.0) -> dict:
    """The decision from predictions ``f`` ``(A, D, n)`` in plain NumPy (identity transform, no offset), in the layout
    of ``optimal_arm``.  Its sums run in NumPy's order: it is the definition only where every sum is exact."""
    A, D, n = f.shape
    cost = np.zeros(A) if cost is None else np.asarray(cost, np.float64)
    u = sign * f - cost[:, None, None]
    best = np.argmax(u, axis=0)                                           # (D, n): the first of the largest
    umax = np.take_along_axis(u, best[None], axis=0)[0]
    res = {"p_best": np.stack([(best == a).sum(axis=0) for a in range(A)], axis=1) / float(D),
           "mean_utility": ((u.sum(axis=1) + 0.0) / float(D)).T,    # (+ 0.0: a sum that starts from +0.0 is never -0.0)
           "expected_regret": (((umax[None] - u).sum(axis=1) + 0.0) / float(D)).T}
    bayes = res["bayes_arm"] = np.argmax(u.sum(axis=1) + 0.0, axis=0).astype(np.int32)
    onehot = np.zeros((G, n))
    onehot[gid, np.arange(n)] = w
    W = res["group_weight"] = onehot.sum(axis=1)
    rows = np.arange(n)
    res["value_optimal"] = (umax @ onehot.T + 0.0) / W
    res["value_bayes"] = (u[bayes, :, rows].T @ onehot.T + 0.0) / W
    res["regret_bayes"] = res["value_optimal"] - res["value_bayes"]
    if policy is not None:
        res["value_policy"] = (u[np.asarray(policy), :, rows].T @ onehot.T + 0.0) / W
    res["value_arm"] = np.stack([(u[a] @ onehot.T + 0.0) / W for a in range(A)], axis=-1)
    res["share_best"] = np.stack([(best == a).astype(np.float64) @ onehot.T / W for a in range(A)], axis=-1)
    return res


# ------------------------------------------------------------------ a backend made of the host references
_array = permimp._array


class HostBackend:
    """What ``optimal_arm`` and ``arm_predictions`` ask of the HIP backend, answered on the host: ``pgb_predict`` is the
    oracle's, ``pgb_predict_arms`` is :func:`reference_block`, the decide step is the host build of the header.
    ``calls`` lists the ``nb`` of the ``pgb_predict_arms`` calls."""

    def __init__(self, oracle, pool):
        from _oracle import NumpyMemory

        self.mem = NumpyMemory()
        self.lib = _HostLibrary(oracle, pool)
        self.calls = self.lib.calls


class _HostLibrary(permimp._HostLibrary):
    def arms_entry_points(self):
        L = lib()

        def predict_arms(carr, fidx, n_forests, m, xd, nb, p, ldx, cols, s, arms, A, picks, n_picks, f, out, list_len, stream):
            assert ldx == p
            table = _array(fidx, (n_forests, m), np.int32)
            cols_, picks_ = _array(cols, (s,), np.int32).copy(), _array(picks, (n_picks,), np.int32).copy()
            K = int(self._pool.n_outputs)
            block = _array(xd, (nb, p))
            got, lens = reference_block(self._oracle, self._pool, table, block, cols_.tolist(), _array(arms, (A, s)).copy(), picks_)
            # (the caller's f is the one the reference computed)
            assert np.array_equal(_array(f, (n_picks, K, nb)), permimp.predict(self._oracle, self._pool, table[picks_], block))
            _array(out, got.shape)[...] = got
            if list_len is not None:
                _array(list_len, (n_picks,), np.int32)[...] = lens
            self.calls.append(int(nb))
            return 0

        def decide_(*a):
            L.arms_block(*a[:-1])
            return 0

        def finish(ws, D, G, A, has_policy, out, w_out, counts, stream):
            L.arms_finish(ws, D, G, A, out, w_out, counts)
            got = list(counts)
            return -1 if got[1] != 0 or (has_policy and got[2] != 0) else 0

        return predict_arms, decide_, finish, lambda D, G, A: 8 * int(L.arms_ws_doubles(D, G, A))
