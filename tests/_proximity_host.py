"""Host references of the posterior proximity (``include/pgbart_proximity.h``), two of them:

* a small C shim around the header -- the header the device kernels compile -- built with gcc like
  ``tests/_rowreduce_host.py``: ``pgb_prox_mismatch4``, ``pgb_prox_stop`` and the sequential references
  ``pgb_prox_codes_block``, ``pgb_prox_count_block`` and ``pgb_prox_topk_block``;
* an INDEPENDENT recount in Python / NumPy that uses nothing of the header: the stop-node walk over ``TreeArrays`` with
  ``_predict_exact._goes_left``, the distances as a count of unequal codes, the top-k by ``np.lexsort``.

Everything is an integer: every comparison against either is an exact equality."""
import ctypes as C
import math

import numpy as np

from _host_build import build
from _predict_exact import _goes_left

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_proximity.h"
int prox_pad(void) { return PGB_PROX_PAD; }
int prox_max_k(void) { return PGB_PROX_MAX_K; }
int prox_max_nodes(void) { return PGB_PROX_MAX_NODES; }
int64_t prox_max_slots(void) { return PGB_PROX_MAX_SLOTS; }
int64_t prox_words(int64_t T) { return pgb_prox_words(T); }
int64_t prox_topk_ws_words(int64_t q, int k) { return pgb_prox_topk_ws_words(q, k); }
uint32_t prox_mismatch4(uint32_t a, uint32_t b) { return pgb_prox_mismatch4(a, b); }
int prox_stop(const pgb_tree_arrays* tr, int t, const double* x, const uint8_t* excl) { return pgb_prox_stop(tr, t, x, excl); }
void prox_codes(const pgb_tree_arrays* tr, const int32_t* fidx, int D, int m, const double* X, int64_t nb, int64_t ldx,
                const uint8_t* excl, uint32_t* codes, int64_t ldc) {
  pgb_prox_codes_block(tr, fidx, D, m, X, nb, ldx, excl, codes, ldc);
}
void prox_count(const uint32_t* cq, int64_t ldq, int64_t q, const uint32_t* cr, int64_t ldr, int64_t nb, int64_t W,
                uint32_t* dist, int64_t ldo, int init) {
  pgb_prox_count_block(cq, ldq, q, cr, ldr, nb, W, dist, ldo, init);
}
void prox_topk(const uint32_t* dist, int64_t ldo, int64_t q, int64_t nb, int64_t first_row, int64_t self_row0, int k,
               uint64_t* ws, int init) {
  pgb_prox_topk_block(dist, ldo, q, nb, first_row, self_row0, k, ws, init);
}
"""

P, I64 = C.c_void_p, C.c_int64
SIGNATURES = {"prox_max_slots": (I64, []), "prox_words": (I64, [I64]), "prox_topk_ws_words": (I64, [I64, C.c_int]),
              "prox_mismatch4": (C.c_uint32, [C.c_uint32, C.c_uint32]),
              "prox_stop": (C.c_int, [P, C.c_int, P, P]),
              "prox_codes": (None, [P, P, C.c_int, C.c_int, P, I64, I64, P, P, I64]),
              "prox_count": (None, [P, I64, I64, P, I64, I64, I64, P, I64, C.c_int]),
              "prox_topk": (None, [P, I64, I64, I64, I64, I64, C.c_int, P, C.c_int])}
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def lib():
    return build("prox_host", SHIM, SIGNATURES)


def _p(x):
    return None if x is None else x.ctypes.data


def _flags(excluded, p: int):
    if excluded is None or len(excluded) == 0:
        return None
    f = np.zeros(p, np.uint8)
    f[[int(e) for e in excluded if 0 <= int(e) < p]] = 1
    return f


# ------------------------------------------------------------------ the header
def header_codes(pool, fidx, X, excluded=None, ldc=None, fill=0xDEADBEEF) -> np.ndarray:
    """``pgb_prox_codes_block`` -> the words ``uint32 (W, ldc)`` (the columns beyond the rows keep ``fill``)."""
    X = np.ascontiguousarray(X, np.float64)
    fidx = np.ascontiguousarray(fidx, np.int32)
    (D, m), (n, p) = fidx.shape, X.shape
    ldc = n if ldc is None else ldc
    out = np.full((int(lib().prox_words(D * m)), ldc), fill, np.uint32)
    carr, fl = pool.as_c(), _flags(excluded, p)
    lib().prox_codes(C.addressof(carr), _p(fidx), D, m, _p(X), n, p, _p(fl), _p(out), ldc)
    return out


def header_count(cq, cr, q=None, nb=None, dist=None) -> np.ndarray:
    """``pgb_prox_count_block`` of the words ``cq (W, ldq)`` and ``cr (W, ldr)``; ``dist``: the distances to continue
    from (``None``: init) -> ``uint32 (q, nb)``."""
    cq, cr = np.ascontiguousarray(cq, np.uint32), np.ascontiguousarray(cr, np.uint32)
    q, nb = cq.shape[1] if q is None else q, cr.shape[1] if nb is None else nb
    init = dist is None
    dist = np.full((q, nb), 0xABABABAB, np.uint32) if init else np.ascontiguousarray(dist, np.uint32).copy()
    lib().prox_count(_p(cq), cq.shape[1], q, _p(cr), cr.shape[1], nb, cq.shape[0], _p(dist), nb, int(init))
    return dist


def header_topk(dist, k, first_row=0, self_row0=-1, ws=None) -> np.ndarray:
    """``pgb_prox_topk_block`` of ``dist (q, nb)`` into the workspace ``ws`` (``None``: init) -> the workspace."""
    dist = np.ascontiguousarray(dist, np.uint32)
    q, nb = dist.shape
    init = ws is None
    ws = np.full(int(lib().prox_topk_ws_words(q, k)), 12345, np.uint64) if init else ws.copy()
    lib().prox_topk(_p(dist), nb, q, nb, first_row, self_row0, k, _p(ws), int(init))
    return ws


# ------------------------------------------------------------------ the independent recount
def stop_node(pool, t: int, x: np.ndarray, excl: set) -> int:
    """The tree-local index of the node where the row ``x`` stops in tree ``t``: at a leaf, or at a split whose column
    is excluded or whose value is NaN."""
    base = int(pool.node_off[t])
    k, steps = 0, 0
    while True:
        steps += 1
        assert steps <= 1 << 16, "the walk does not end"
        g = base + k
        j = int(pool.var[g])
        if j < 0:
            return k
        xv = float(x[j])
        if j in excl or math.isnan(xv):
            return k
        k = int(pool.left[g]) if _goes_left(int(pool.rule[g]), xv, float(pool.split[g])) else int(pool.right[g])


def stop_nodes(pool, fidx, X, excluded=()) -> np.ndarray:
    """-> ``(D, m, n)`` integers (not yet bytes: a tree of more than 255 nodes shows)."""
    X = np.asarray(X, np.float64)
    fidx = np.asarray(fidx)
    (D, m), (n, p) = fidx.shape, X.shape
    excl = {int(e) for e in excluded if 0 <= int(e) < p}
    per_tree = {}
    out = np.empty((D, m, n), np.int64)
    for d in range(D):
        for t in range(m):
            tree = int(fidx[d, t])
            if tree not in per_tree:
                per_tree[tree] = np.array([stop_node(pool, tree, X[i], excl) for i in range(n)], np.int64)
            out[d, t] = per_tree[tree]
    return out


def pack(codes) -> np.ndarray:
    """``(T, n)`` codes -> the words ``uint32 (ceil(T / 4), n)``: slot ``4 w + b`` in bits ``8 b .. 8 b + 7``, the slots
    beyond ``T`` hold 0xFF."""
    codes = np.asarray(codes, np.int64)
    T, n = codes.shape
    assert codes.min() >= 0 and codes.max() <= 254
    W = -(-T // 4)
    full = np.full((4 * W, n), 0xFF, np.int64)
    full[:T] = codes
    full = full.reshape(W, 4, n)
    return (full[:, 0] + full[:, 1] * 256 + full[:, 2] * 65536 + full[:, 3] * 16777216).astype(np.uint32)


def distances(codes_q, codes_r) -> np.ndarray:
    """``(T, q)`` and ``(T, n)`` codes -> ``(q, n)``: in how many slots the codes differ."""
    codes_q, codes_r = np.asarray(codes_q), np.asarray(codes_r)
    return (codes_q[:, :, None] != codes_r[:, None, :]).sum(0).astype(np.int64)


def topk(dist, k: int, exclude_self: bool = False):
    """-> (index ``(q, k)``, distance ``(q, k)``, the sum of the distances taken in ``(q,)``): nearest first, ties to the
    smaller row index."""
    dist = np.asarray(dist, np.int64)
    q, n = dist.shape
    idx, dk, total = np.empty((q, k), np.int64), np.empty((q, k), np.int64), np.empty(q, np.int64)
    for i in range(q):
        rows = np.array([j for j in range(n) if not (exclude_self and j == i)], np.int64)
        order = rows[np.lexsort((rows, dist[i, rows]))][:k]
        idx[i], dk[i], total[i] = order, dist[i, order], dist[i, rows].sum()
    return idx, dk, total


def split_ws(ws, q: int, k: int):
    """The workspace of a top-k -> (index, distance, sum) as :func:`topk` returns them."""
    ws = np.asarray(ws, np.uint64)
    keys, total = ws[:q * k].reshape(q, k), ws[q * k:q * k + q]
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), (keys >> np.uint64(32)).astype(np.int64), total.astype(np.int64)
