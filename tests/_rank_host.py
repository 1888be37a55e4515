"""Test helpers of the discrimination tests (``test_discrimination.py``, ``test_discrimination_gpu.py``).

* :func:`key`, :func:`value`, :func:`keys_block`, :func:`reference`, :func:`fault`, :func:`layout` -- the functions of
  ``include/pgbart_rank.h`` (the header the device kernels compile) through a small C shim built with gcc.
* :func:`numpy_counts` -- the definition restated with NumPy comparison matrices.
* :class:`HostBackend` -- ``_permimp_host.HostBackend`` (``pgb_predict`` is the oracle's) plus ``pgb_rank_keys`` and
  ``pgb_rank_metrics`` from the header, so that the Python layer runs without a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import _permimp_host as permimp
from _host_build import build

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_rank.h"
int rank_max_groups(void) { return PGB_RANK_MAX_GROUPS; }
int rank_max_thresholds(void) { return PGB_RANK_MAX_THRESHOLDS; }
uint64_t rank_key(double v) { return pgb_rank_key(v); }
double rank_value(double a, int has_off, double off, int transform) {
  const pgb_lltabs tb = pgb_lltabs_default();
  return pgb_rowsum_value(a, has_off, off, transform, &tb);
}
void rank_keys_block(const double* a, int64_t D, int64_t nb, int64_t ld, const double* off, int transform, const int64_t* dest,
                     int64_t n, uint64_t* keys, uint64_t* counters) {
  const pgb_lltabs tb = pgb_lltabs_default();
  pgb_rank_keys_block(a, D, nb, ld, off, transform, dest, n, &tb, keys, counters);
}
void rank_reference(const uint64_t* keys, int64_t D, int64_t n, const int64_t* seg_off, int G, const double* thr, int T,
                    int64_t* out) {
  pgb_rank_reference(keys, D, n, seg_off, G, thr, T, out);
}
int rank_fault(int64_t D, int64_t n, const int64_t* seg_off, int64_t G, const double* thr, int64_t T, int64_t* where) {
  return pgb_rank_fault(D, n, seg_off, G, thr, T, where);
}
int64_t rank_layout(const int32_t* c, const int32_t* g, int64_t n, int G, int64_t* seg_off, int64_t* dest) {
  return pgb_rank_layout(c, g, n, G, seg_off, dest);
}
"""

P, I64 = C.c_void_p, C.c_int64
SIGNATURES = {
    "rank_max_groups": (C.c_int, []), "rank_max_thresholds": (C.c_int, []),
    "rank_key": (C.c_uint64, [C.c_double]),
    "rank_value": (C.c_double, [C.c_double, C.c_int, C.c_double, C.c_int]),
    "rank_keys_block": (None, [P, I64, I64, I64, P, C.c_int, P, I64, P, P]),
    "rank_reference": (None, [P, I64, I64, P, C.c_int, P, C.c_int, P]),
    "rank_fault": (C.c_int, [I64, I64, P, I64, P, I64, P]),
    "rank_layout": (I64, [P, P, I64, C.c_int, P, P]),
}
TRANSFORMS = {"identity": 0, "exp": 1, "logistic": 2, "probit": 3}
NAN_KEY = (1 << 64) - 1


def lib():
    return build("rank_host", SHIM, SIGNATURES)


def key(v) -> np.ndarray:
    """``pgb_rank_key`` of every element of ``v`` -> uint64."""
    L = lib()
    return np.array([L.rank_key(float(x)) for x in np.ravel(v)], np.uint64).reshape(np.shape(v))


def value(a, transform, off=None) -> np.ndarray:
    """The header's value function of every element of ``a`` ``(..., n)``; ``off`` ``(n,)`` or ``None``."""
    L, code = lib(), TRANSFORMS[transform] if isinstance(transform, str) else transform
    a = np.asarray(a, np.float64)
    out = np.empty_like(a)
    flat, oflat = a.reshape(-1, a.shape[-1]), out.reshape(-1, a.shape[-1])
    for r in range(flat.shape[0]):
        for i in range(flat.shape[1]):
            oflat[r, i] = L.rank_value(flat[r, i], int(off is not None), 0.0 if off is None else float(off[i]), code)
    return out


def layout(cls, gid, G: int):
    """``pgb_rank_layout`` -> ``(seg_off (2 G + 1,), dest (n,))``."""
    cls, gid = np.ascontiguousarray(cls, np.int32), np.ascontiguousarray(gid, np.int32)
    seg_off, dest = np.empty(2 * G + 1, np.int64), np.empty(cls.size, np.int64)
    assert lib().rank_layout(cls.ctypes.data, gid.ctypes.data, cls.size, G, seg_off.ctypes.data, dest.ctypes.data) == 0
    return seg_off, dest


def keys_block(a, transform, dest, n: int, off=None, keys=None, counters=None):
    """``pgb_rank_keys_block`` on ``a`` ``(D, nb)`` (the last axis contiguous, any stride between the draws) ->
    ``(keys (D, n), counters (2,))``; given ``keys`` and ``counters`` are continued."""
    D, nb = a.shape
    assert a.dtype == np.float64 and a.strides[1] == 8 and a.strides[0] % 8 == 0
    dest = np.ascontiguousarray(dest, np.int64)
    off = None if off is None else np.ascontiguousarray(off, np.float64)
    keys = np.zeros((D, n), np.uint64) if keys is None else keys
    counters = np.zeros(2, np.uint64) if counters is None else counters
    code = TRANSFORMS[transform] if isinstance(transform, str) else transform
    lib().rank_keys_block(a.ctypes.data, D, nb, a.strides[0] // 8, None if off is None else off.ctypes.data, code,
                          dest.ctypes.data, n, keys.ctypes.data, counters.ctypes.data)
    return keys, counters


def reference(keys, seg_off, thr=()) -> np.ndarray:
    """``pgb_rank_reference`` on laid-out ``keys`` ``(D, n)`` -> ``out (D, G, 2 + 2 T)`` int64."""
    keys = np.ascontiguousarray(keys, np.uint64)
    D, n = keys.shape
    seg_off, thr = np.ascontiguousarray(seg_off, np.int64), np.ascontiguousarray(thr, np.float64)
    G, T = (seg_off.size - 1) // 2, thr.size
    out = np.full((D, G, 2 + 2 * T), -1, np.int64)
    lib().rank_reference(keys.ctypes.data, D, n, seg_off.ctypes.data, G, thr.ctypes.data if T else None, T, out.ctypes.data)
    return out


def fault(D, n, seg_off, G, thr, T):
    """``pgb_rank_fault`` -> ``(the number of the sentence, where)``."""
    where = C.c_int64(-1)
    seg_off = None if seg_off is None else np.ascontiguousarray(seg_off, np.int64)
    thr = None if thr is None else np.ascontiguousarray(thr, np.float64)
    code = lib().rank_fault(D, n, None if seg_off is None else seg_off.ctypes.data, G, None if thr is None else thr.ctypes.data,
                            T, C.byref(where))
    return int(code), int(where.value)


def reference_scores(scores, cls, gid, G: int, thr=()):
    """The header end to end on scores ``(D, n)`` (identity, no offset): layout, keys, pair counting ->
    ``(out (D, G, 2 + 2 T), n_nan)``."""
    scores = np.ascontiguousarray(scores, np.float64)
    seg_off, dest = layout(cls, gid, G)
    keys, counters = keys_block(scores, "identity", dest, scores.shape[1])
    return reference(keys, seg_off, thr), int(counters[0])


def numpy_counts(scores, cls, gid, G: int, thr=()) -> np.ndarray:
    """The definition in NumPy on the doubles themselves (``-0.0 == 0.0`` and the order of the infinities are IEEE's):
    the comparison matrix ``v_pos[:, None] > v_neg[None, :]``, ``==`` for the ties, ``>=`` for the thresholds and for
    ``tp(e)``, ``fp(e)``.  No NaN scores.  -> ``out (D, G, 2 + 2 T)`` int64."""
    scores, cls, gid = np.asarray(scores, np.float64), np.asarray(cls), np.asarray(gid)
    D, T = scores.shape[0], len(thr)
    out = np.zeros((D, G, 2 + 2 * T), np.int64)
    for d in range(D):
        for g in range(G):
            pos, neg = scores[d, (gid == g) & (cls == 1)], scores[d, (gid == g) & (cls == 0)]
            n1, n0 = pos.size, neg.size
            out[d, g, 0] = 2 * int((pos[:, None] > neg[None, :]).sum()) + int((pos[:, None] == neg[None, :]).sum())
            both = np.concatenate([pos, neg])
            tp = (pos[None, :] >= both[:, None]).sum(axis=1).astype(np.int64)
            fp = (neg[None, :] >= both[:, None]).sum(axis=1).astype(np.int64)
            out[d, g, 1] = int(np.abs(tp * n0 - fp * n1).max())
            for t, level in enumerate(thr):
                out[d, g, 2 + t] = int((pos >= level).sum())
                out[d, g, 2 + T + t] = int((neg >= level).sum())
    return out


# ------------------------------------------------------------------ a backend made of the host references
def _u64(address, count):
    return np.ctypeslib.as_array((C.c_uint64 * int(count)).from_address(int(address)))


def _i64(address, count):
    return np.ctypeslib.as_array((C.c_int64 * int(count)).from_address(int(address)))


class HostBackend(permimp.HostBackend):
    """What ``discrimination`` and ``discrimination_matrix`` ask of the HIP backend, answered on the host:
    ``pgb_predict`` is the oracle's, ``pgb_rank_keys`` and ``pgb_rank_metrics`` are the host build of their header.
    ``key_calls`` lists the ``(D, nb)`` of the ``pgb_rank_keys`` calls, ``metric_calls`` the ``D`` of the
    ``pgb_rank_metrics`` calls."""

    def __init__(self, oracle, pool):
        from _oracle import NumpyMemory

        self.mem = NumpyMemory()
        self.lib = _HostLibrary(oracle, pool)
        self.calls = self.lib.calls
        self.key_calls, self.metric_calls = self.lib.key_calls, self.lib.metric_calls


class _HostLibrary(permimp._HostLibrary):
    def __init__(self, oracle, pool):
        super().__init__(oracle, pool)
        self.key_calls, self.metric_calls = [], []

    def rank_entry_points(self):
        L = lib()

        def keys_(a, D, nb, ld, off, transform, dest, n, keys, cnt, stream):
            if not (a and dest and keys and cnt) or D < 1 or nb < 1 or n < 2 or nb > n or ld < nb or not 0 <= transform < 4:
                return -1
            L.rank_keys_block(a, D, nb, ld, off, transform, dest, n, keys, cnt)
            self.key_calls.append((int(D), int(nb)))
            return 0

        def ws_bytes(D, n, G):
            return 8 * D * n if D >= 1 and n >= 2 and 1 <= G <= 256 and D * n < 1 << 31 else 0

        def metrics(keys, ws, D, n, seg_off, G, thr, T, cnt, out, counts, stream):
            where = C.c_int64()
            if not (keys and ws and cnt and out and counts) or L.rank_fault(D, n, seg_off, G, thr, T, C.byref(where)):
                return -1
            got = _u64(cnt, 2)
            counts_ = counts if isinstance(counts, int) else C.addressof(counts)
            if got[1] != 0:
                _i64(counts_, 2)[:] = got.astype(np.int64)
                return -1
            L.rank_reference(keys, D, n, seg_off, G, thr, T, out)
            _i64(counts_, 2)[:] = got.astype(np.int64)
            self.metric_calls.append(int(D))
            return 0

        return keys_, ws_bytes, metrics
