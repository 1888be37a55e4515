"""Test helpers of the accumulated-local-effects tests (``test_ale.py``, ``test_ale_gpu.py``).

* :func:`bin_of` -- the host build of ``include/pgbart_ale.h`` (the header the device kernels compile) through a small C
  shim built with gcc: ``pgb_ale_bin`` over a vector of values.
* :func:`reference_block` -- the host reference of ``out`` and ``bins_out``: the bins are the header's; ``A_hi`` and
  ``A_lo`` are the oracle's ``pgb_predict`` called with the use list (``_permimp_host.use_lists``: the header's packer)
  as a one-forest table of ``m = len(list)``, at the block with the column overwritten per row by the upper and the lower
  edge of the row's bin (the device's ``pgb_predict`` is bit-identical to the oracle's: ``test_predict_edges_gpu.py``);
  ``delta = A_hi - A_lo`` in NumPy -- one rounding, as the header states -- and ``+0.0`` in the missing bin.
* :class:`HostBackend` -- a backend made of the host references, so that the Python layer runs without a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import _permimp_host as permimp
from _host_build import build

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_ale.h"
int ale_max_bins(void) { return PGB_ALE_MAX_BINS; }
void ale_bins(const double* e, int32_t B, const double* x, int64_t n, int32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = pgb_ale_bin(e, B, x[i]);
}
"""

SIGNATURES = {"ale_max_bins": (C.c_int, []),
              "ale_bins": (None, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p])}


def lib():
    return build("ale_host", SHIM, SIGNATURES)


def bin_of(edges, x) -> np.ndarray:
    """``pgb_ale_bin(edges, len(edges) - 1, x[i])`` for every ``i``."""
    e = np.ascontiguousarray(edges, np.float64)
    x = np.ascontiguousarray(x, np.float64).ravel()
    out = np.empty(x.size, np.int32)
    lib().ale_bins(e.ctypes.data, e.size - 1, x.ctypes.data, x.size, out.ctypes.data)
    return out


def reference_block(oracle, pool, fidx, block, cols, edges, picks):
    """``(out (q, n_picks, K, nb), bins_out (q, nb))`` of ``pgb_predict_ale`` from what the entry point is given: the
    block's rows, the columns, ``edges`` (a list of one vector per column) and the picks."""
    block = np.ascontiguousarray(block, np.float64)
    nb, p = block.shape
    fidx = np.ascontiguousarray(fidx, np.int32)
    picks = np.asarray(picks)
    K = int(pool.n_outputs)
    q = len(cols)
    off, lst = permimp.use_lists(pool, fidx, p, cols, picks)
    out = np.empty((q, picks.size, K, nb))
    bins = np.empty((q, nb), np.int32)
    for s, c in enumerate(cols):
        e = np.asarray(edges[s], np.float64)
        B = e.size - 1
        b = bins[s] = bin_of(e, block[:, c])
        missing = b == B
        at = np.where(missing, 0, b)                                    # (any finite stand-in: the result is dropped)
        X_hi, X_lo = block.copy(), block.copy()
        X_hi[:, c], X_lo[:, c] = e[at + 1], e[at]
        for d in range(picks.size):
            mine = lst[off[d * q + s]:off[d * q + s + 1]]
            A_hi = permimp.predict(oracle, pool, mine[None, :], X_hi)[0] if mine.size else np.zeros((K, nb))
            A_lo = permimp.predict(oracle, pool, mine[None, :], X_lo)[0] if mine.size else np.zeros((K, nb))
            delta = A_hi - A_lo
            delta[:, missing] = 0.0
            out[s, d] = delta
    return out, bins


def flat_edges(edges) -> tuple:
    """-> (all edges in one vector, ``edge_off (q + 1,)`` int32): what the entry point takes."""
    off = np.concatenate([[0], np.cumsum([len(e) for e in edges])]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate([np.asarray(e, np.float64) for e in edges])), off


# ------------------------------------------------------------------ a backend made of the host references
_array = permimp._array


class HostBackend:
    """What ``accumulated_local_effects`` asks of the HIP backend, answered on the host: ``pgb_predict_ale`` is
    :func:`reference_block`, the row reduce is the host build of its header (``_rowreduce_host``).  ``calls`` lists the
    ``(nb, q)`` of the ``pgb_predict_ale`` calls."""

    def __init__(self, oracle, pool):
        from _oracle import NumpyMemory

        self.mem = NumpyMemory()
        self.lib = _HostLibrary(oracle, pool)
        self.calls = self.lib.calls


class _HostLibrary(permimp._HostLibrary):
    def predict_ale_entry_point(self):
        def call(carr, fidx, n_forests, m, xd, nb, p, ldx, cols, q, edges, edge_off, picks, n_picks, out, bins_out, stream):
            assert ldx == p
            table = _array(fidx, (n_forests, m), np.int32)
            cols_, picks_ = _array(cols, (q,), np.int32).copy(), _array(picks, (n_picks,), np.int32).copy()
            off = _array(edge_off, (q + 1,), np.int32).copy()
            assert off[0] == 0 and np.all(np.diff(off) >= 2)
            flat = _array(edges, (int(off[-1]),)).copy()
            got, bins = reference_block(self._oracle, self._pool, table, _array(xd, (nb, p)), cols_.tolist(),
                                        [flat[off[s]:off[s + 1]] for s in range(q)], picks_)
            _array(out, got.shape)[...] = got
            _array(bins_out, bins.shape, np.int32)[...] = bins
            self.calls.append((int(nb), int(q)))
            return 0

        return call
