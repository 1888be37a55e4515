"""Test helpers of the survival tests (``test_survival.py``, ``test_survival_gpu.py``).

* :func:`block` -- ``pgb_surv_block`` of ``include/pgbart_surv.h`` (the header the device kernel compiles) through a small
  C shim built with gcc; :func:`link_q` -- the header's ``1 - p`` of single values.
* :func:`numpy_curves` -- the definition restated with NumPy's sequential ``accumulate`` on the header's ``q``.
* :class:`HostBackend` -- ``_arms_host.HostBackend`` plus the host ``pgb_surv_block`` and the host row summary, so that
  the Python layer runs without a GPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import _arms_host as arms_host
from _host_build import build

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_surv.h"
int surv_max_levels(void) { return PGB_SURV_MAX_LEVELS; }
int surv_max_times(void) { return PGB_ARMS_MAX; }
double surv_q(double f, int has_off, double off, int transform) {
  const pgb_lltabs tb = pgb_lltabs_default();
  return pgb_surv_q(f, has_off, off, transform, &tb);
}
void surv_block(double* f, int64_t lda, int64_t ldd, int D, int A, int64_t nb, const double* off, int transform,
                const double* t, const double* dt, const double* u, int Q, double beyond, int init, double* state,
                uint64_t* n_nonfinite) {
  const pgb_lltabs tb = pgb_lltabs_default();
  pgb_surv_block(f, lda, ldd, D, A, nb, off, transform, t, dt, u, Q, beyond, init, &tb, state, n_nonfinite);
}
"""

P = C.c_void_p
_BLOCK = [P, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int64, P, C.c_int, P, P, P, C.c_int, C.c_double, C.c_int, P, P]
SIGNATURES = {"surv_max_levels": (C.c_int, []), "surv_max_times": (C.c_int, []),
              "surv_q": (C.c_double, [C.c_double, C.c_int, C.c_double, C.c_int]), "surv_block": (None, _BLOCK)}
LINKS = {"logistic": 2, "probit": 3}


def lib():
    return build("surv_host", SHIM, SIGNATURES)


def link_q(f, link, off=None) -> np.ndarray:
    """The header's ``q = 1 - p`` of every element of ``f`` (``off``: a scalar offset)."""
    L, code = lib(), LINKS[link]
    has, o = (0, 0.0) if off is None else (1, float(off))
    return np.array([L.surv_q(float(v), has, o, code) for v in np.ravel(f)]).reshape(np.shape(f))


def grid(J: int, origin: float = 0.0, rng=None):
    """``(t, dt, beyond)`` of a grid of ``J`` times as ``survival_curves`` derives them."""
    t = np.arange(1, J + 1, dtype=np.float64) if rng is None else np.cumsum(rng.uniform(0.25, 2.0, J)) + origin
    dt = np.diff(np.concatenate([[origin], t]))
    return np.ascontiguousarray(t), np.ascontiguousarray(dt), float(t[-1] + dt[-1])


def block(f, t, dt, u, beyond, link, off=None, state=None, count=None):
    """``pgb_surv_block`` on ``f`` ``(A, D, nb)``, IN PLACE -- any strides along the first two axes that are multiples
    of the item size, the last axis contiguous.  ``state``: ``None`` starts it (``init = 1``), otherwise the call
    continues from it.  -> ``(state (2 + Q, D, nb), the counter)``."""
    A, D, nb = f.shape
    assert f.dtype == np.float64 and f.strides[2] == 8 and f.strides[0] % 8 == 0 and f.strides[1] % 8 == 0
    t, dt, u = (np.ascontiguousarray(v, np.float64) for v in (t, dt, u))
    assert t.shape == dt.shape == (A,)
    off = None if off is None else np.ascontiguousarray(off, np.float64)
    init = state is None
    if init:
        state = np.full((2 + u.size, D, nb), 7.5)                        # (init must overwrite it)
    assert state.shape == (2 + u.size, D, nb) and state.flags.c_contiguous
    cnt = np.array([0 if count is None else int(count)], np.uint64)
    lib().surv_block(f.ctypes.data, f.strides[0] // 8, f.strides[1] // 8, D, A, nb, None if off is None else off.ctypes.data,
                     LINKS[link], t.ctypes.data, dt.ctypes.data, u.ctypes.data if u.size else None, u.size, float(beyond),
                     int(init), state.ctypes.data, cnt.ctypes.data)
    return state, int(cnt[0])


def numpy_curves(f, t, dt, u, beyond, link, off=None):
    """``(S (A, D, nb), R (D, nb), T (Q, D, nb))`` from predictions ``f`` ``(A, D, nb)`` by the definition: ``q`` is the
    header's (``pgb_rowsum_value`` at the negated predictor, pinned by the row-summary tests), ``S`` is
    ``np.multiply.accumulate`` and ``R`` ``np.add.accumulate`` of ``S_prev * dt`` -- NumPy's accumulate is sequential
    with one rounding per step."""
    f = np.asarray(f, np.float64)
    A, D, nb = f.shape
    q = np.empty_like(f)
    for i in range(nb):
        q[:, :, i] = link_q(f[:, :, i], link, None if off is None else off[i])
    S = np.multiply.accumulate(np.concatenate([np.ones((1, D, nb)), q]), axis=0)[1:]
    S_prev = np.concatenate([np.ones((1, D, nb)), S[:-1]])
    terms = S_prev * np.asarray(dt)[:, None, None]
    R = np.add.accumulate(np.concatenate([np.zeros((1, D, nb)), terms]), axis=0)[-1]
    T = np.full((len(u), D, nb), float(beyond))
    for l, level in enumerate(u):
        with np.errstate(invalid="ignore"):
            hit = S <= level
        first = np.argmax(hit, axis=0)
        T[l] = np.where(hit.any(axis=0), np.asarray(t)[first], float(beyond))
    return S, R, T


# ------------------------------------------------------------------ a backend made of the host references
class HostBackend(arms_host.HostBackend):
    """What ``survival_curves`` and ``survival_matrix`` ask of the HIP backend, answered on the host: ``pgb_predict`` is
    the oracle's, ``pgb_predict_arms`` is ``_arms_host.reference_block``, ``pgb_surv_curves`` the host build of its
    header, the row summary and the row reduce the host builds of theirs.  ``calls`` lists the ``nb`` of the
    ``pgb_predict_arms`` calls, ``surv_calls`` the ``(nb, A, init)`` of the ``pgb_surv_curves`` calls."""

    def __init__(self, oracle, pool):
        from _oracle import NumpyMemory

        self.mem = NumpyMemory()
        self.lib = _HostLibrary(oracle, pool)
        self.calls = self.lib.calls
        self.surv_calls = self.lib.surv_calls


class _HostLibrary(arms_host._HostLibrary):
    def __init__(self, oracle, pool):
        super().__init__(oracle, pool)
        self.surv_calls = []

    def surv_entry_points(self):
        L = lib()

        def curves(f, lda, ldd, D, A, nb, off, transform, t, dt, u, Q, beyond, init, state, cnt, stream):
            L.surv_block(f, lda, ldd, D, A, nb, off, transform, t, dt, u, Q, beyond, init, state, cnt)
            self.surv_calls.append((int(nb), int(A), int(init)))
            return 0

        return curves

    def rowsummary_entry_point(self):
        import _rowsummary_host as rs

        return lambda *a: rs.lib().rowsum_columns(*a[:-1])
