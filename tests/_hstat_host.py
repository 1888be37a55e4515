"""Test helpers of the H-statistic tests (``test_hstat.py``, ``test_hstat_gpu.py``).

* :func:`lib` -- the host build of ``include/pgbart_hstat.h`` (the header the device kernels compile) through a small C
  shim built with gcc: the plan of a call, the block evaluators and the finish, each entry mirroring the device entry
  point of the same name.
* :func:`walk_sums` -- ``g``, the walk's sums of the column jobs: the oracle's ``pgb_predict`` called with the use list
  (``_permimp_host.use_lists``) as a one-forest table, as ``_permimp_host.reference_block`` does for its ``A``.
* :class:`Reference` -- one whole call on the host, block by block: what ``pgb_hstat_*`` must return bit for bit.
* :func:`brute_force` -- J, T and I from the DEFINITION alone: the ``n_e x n_b`` hybrid rows are built and predicted,
  with the exact rational walk of ``_predict_exact`` (``exact=True``: ``Fraction`` throughout) or with the oracle's
  ``pgb_predict`` and NumPy means.
* :class:`HostBackend` -- a backend made of the host references, so that the Python layer runs without a GPU.
"""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np

import _permimp_host as permimp
import _predict_exact as ex
from _host_build import build
from pymc_bart_amd import _abi

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_hstat.h"

int hstat_max_pairs(void) { return PGB_HSTAT_MAX_PAIRS; }
int hstat_max_u(void) { return PGB_HSTAT_MAX_U; }

typedef struct {
  pgb_shap_pack sp;
  pgb_hstat_plan pl;
  pgb_shap_view v;
  pgb_hstat_plan_view pv;
} job_t;

static int job_open(job_t* j, const pgb_tree_arrays* trees, const int32_t* fidx, int m, int p, const int32_t* cols, int q,
                    const int32_t* pairs, int n_pairs, const int32_t* picks, int n_picks, int32_t* n_common) {
  if (pgb_shap_pack_build(trees, p, &j->sp)) return -10;
  const int rc = pgb_hstat_plan_build(trees, fidx, m, p, cols, q, pairs, n_pairs, picks, n_picks,
                                      (const int32_t*)(j->sp.buf + j->sp.o_off), n_common, &j->pl);
  if (rc) {
    pgb_shap_pack_free(&j->sp);
    return rc;
  }
  const int lin = trees->slope && trees->xbar && trees->svar;
  j->v = pgb_shap_pack_view(&j->sp, j->sp.buf, trees->value, lin ? trees->slope : 0, trees->n_outputs);
  j->pv = pgb_hstat_plan_at(&j->pl, j->pl.buf);
  return 0;
}
static void job_close(job_t* j) {
  pgb_shap_pack_free(&j->sp);
  pgb_hstat_plan_free(&j->pl);
}

#define JOB_ARGS const pgb_tree_arrays* trees, const int32_t* fidx, int m, int p, const int32_t* cols, int q, \
                 const int32_t* pairs, int n_pairs, const int32_t* picks, int n_picks
#define JOB_PASS trees, fidx, m, p, cols, q, pairs, n_pairs, picks, n_picks

/* sizes[0 .. 10): n_jobs, n_tree, n_slots, then the layout's seven words; plan_out: NULL or the plan's buffer */
int hstat_sizes(JOB_ARGS, int64_t* sizes, int32_t* n_common, int32_t* plan_out) {
  job_t j;
  const int rc = job_open(&j, JOB_PASS, n_common);
  if (rc) return rc;
  const pgb_hstat_layout L = pgb_hstat_ws_layout(j.pl.n_jobs, trees->n_outputs, j.pl.n_slots);
  sizes[0] = j.pl.n_jobs; sizes[1] = j.pl.n_tree; sizes[2] = j.pl.n_slots;
  sizes[3] = L.o_rpart; sizes[4] = L.o_wpart; sizes[5] = L.o_vpart; sizes[6] = L.o_V; sizes[7] = L.o_mpart; sizes[8] = L.o_B;
  sizes[9] = L.words;
  if (plan_out) memcpy(plan_out, j.pl.buf, sizeof(int32_t) * (size_t)pgb_hstat_plan_words(&j.pl));
  job_close(&j);
  return 0;
}

int hstat_background(JOB_ARGS, const double* X, int64_t nb, int64_t ldx, const double* vw, int64_t first_row, int init,
                     double* ws) {
  job_t j;
  const int rc = job_open(&j, JOB_PASS, 0);
  if (rc) return rc;
  pgb_hstat_bg_block(&j.v, &j.pv, j.pl.n_jobs, j.pl.n_slots, X, nb, ldx, vw, 0, first_row, init, ws);
  job_close(&j);
  return 0;
}

int hstat_rows(JOB_ARGS, const double* X, int64_t nb, int64_t ldx, const double* w, const double* g, int64_t first_row,
               int init, double* ws, double* jscr, double* t_rows, double* i_rows) {
  job_t j;
  const int rc = job_open(&j, JOB_PASS, 0);
  if (rc) return rc;
  if (init) pgb_hstat_moments(j.pl.n_jobs, trees->n_outputs, j.pl.n_slots, ws);
  pgb_hstat_rows_block(&j.v, &j.pv, n_picks, q, n_pairs, pairs, j.pl.n_slots, X, nb, ldx, w, g, 0, first_row, init, ws, jscr,
                       t_rows, i_rows);
  job_close(&j);
  return 0;
}

void hstat_finish(const double* ws, int n_picks, int q, int n_pairs, int K, const double* var_fit, double* main_var,
                  double* total_var, double* h2_total, double* inter_var, double* h2, int64_t* n_nonfinite) {
  pgb_hstat_finish_host(ws, n_picks, q, n_pairs, K, var_fit, main_var, total_var, h2_total, inter_var, h2, n_nonfinite);
}
"""

P = C.c_void_p
_JOB = [C.POINTER(_abi.TreeArraysC), P, C.c_int, C.c_int, P, C.c_int, P, C.c_int, P, C.c_int]
SIGNATURES = {"hstat_max_pairs": (C.c_int, []), "hstat_max_u": (C.c_int, []),
              "hstat_sizes": (C.c_int, _JOB + [P, P, P]),
              "hstat_background": (C.c_int, _JOB + [P, C.c_int64, C.c_int64, P, C.c_int64, C.c_int, P]),
              "hstat_rows": (C.c_int, _JOB + [P, C.c_int64, C.c_int64, P, P, C.c_int64, C.c_int, P, P, P, P]),
              "hstat_finish": (None, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, P])}
SIZE_NAMES = ("n_jobs", "n_tree", "n_slots", "o_rpart", "o_wpart", "o_vpart", "o_V", "o_mpart", "o_B", "words")


def lib():
    return build("hstat_host", SHIM, SIGNATURES)


def _i32(a, shape=None):
    a = np.ascontiguousarray(a, np.int32)
    return a if shape is None else a.reshape(shape)


def _ptr(a):
    return None if a is None else a.ctypes.data


class Jobs:
    """The description of the jobs every entry takes: the history, the columns, the pairs (SLOTS of ``cols``), the picks."""

    def __init__(self, pool, fidx, p, cols, pairs, picks):
        self.pool, self.fidx, self.p = pool, _i32(fidx), int(p)
        self.cols, self.picks = _i32(cols), _i32(picks)
        self.pairs = _i32(pairs, (-1, 2)) if len(pairs) else np.zeros((0, 2), np.int32)
        self.q, self.n_pairs, self.n_picks, self.K = self.cols.size, self.pairs.shape[0], self.picks.size, int(pool.n_outputs)
        self.carr = pool.as_c()

    def args(self):
        return (C.byref(self.carr), self.fidx.ctypes.data, self.fidx.shape[1], self.p, self.cols.ctypes.data, self.q,
                _ptr(self.pairs) if self.n_pairs else None, self.n_pairs, self.picks.ctypes.data, self.n_picks)

    def sizes(self, plan=False):
        """-> (dict of ``SIZE_NAMES``, ``n_common (n_picks, n_pairs)`` [, the plan's dict of arrays])."""
        out, common = np.zeros(10, np.int64), np.full((self.n_picks, self.n_pairs), -1, np.int32)
        assert lib().hstat_sizes(*self.args(), out.ctypes.data, _ptr(common), None) == 0
        sizes = dict(zip(SIZE_NAMES, (int(v) for v in out)))
        if not plan:
            return sizes, common
        nj = sizes["n_jobs"]
        buf = np.zeros(4 * nj + 2 + sizes["n_tree"], np.int32)
        assert lib().hstat_sizes(*self.args(), out.ctypes.data, None, buf.ctypes.data) == 0
        parts = {"tree_off": buf[:nj + 1], "slot_off": buf[nj + 1:2 * nj + 2], "a": buf[2 * nj + 2:3 * nj + 2],
                 "b": buf[3 * nj + 2:4 * nj + 2], "tree": buf[4 * nj + 2:]}
        return sizes, common, parts


def walk_sums(oracle, jobs: Jobs, block) -> np.ndarray:
    """``g (n_picks, q, K, nb)``: ``pgb_predict`` of every (pick, column)'s use list at the block's rows."""
    block = np.ascontiguousarray(block, np.float64)
    off, lst = permimp.use_lists(jobs.pool, jobs.fidx, jobs.p, jobs.cols, jobs.picks)
    g = np.zeros((jobs.n_picks, jobs.q, jobs.K, block.shape[0]))
    for d in range(jobs.n_picks):
        for s in range(jobs.q):
            mine = lst[off[d * jobs.q + s]:off[d * jobs.q + s + 1]]
            if mine.size:
                g[d, s] = permimp.predict(oracle, jobs.pool, mine[None, :], block)[0]
    return g


class Reference:
    """One whole call on the host.  ``background(X, v, r0, init)`` and ``rows(X, w, r0, init)`` take one block each, as
    the device entry points do; ``finish(var_fit)`` -> the dict of outputs.  ``J``, ``T`` ``(n_picks, q, K, n)`` and
    ``I`` ``(n_picks, n_pairs, K, n)`` collect the per-row values of every block."""

    def __init__(self, oracle, jobs: Jobs):
        self.oracle, self.jobs = oracle, jobs
        self.sizes, self.n_common = jobs.sizes()
        self.ws = np.full(self.sizes["words"], np.nan)  # (whatever was there before: init must not read it)
        self._J, self._T, self._I = [], [], []

    def background(self, X, v, r0=0, init=True):
        X, v = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(v, np.float64)
        assert lib().hstat_background(*self.jobs.args(), X.ctypes.data, X.shape[0], X.shape[1], v.ctypes.data, r0, int(init),
                                      self.ws.ctypes.data) == 0

    def rows(self, X, w, r0=0, init=True, g=None):
        j = self.jobs
        X, w = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(w, np.float64)
        nb = X.shape[0]
        g = np.ascontiguousarray(walk_sums(self.oracle, j, X) if g is None else g)
        J, T = np.empty((j.n_picks, j.q, j.K, nb)), np.empty((j.n_picks, j.q, j.K, nb))
        I = np.empty((j.n_picks, j.n_pairs, j.K, nb))  # noqa: E741
        assert lib().hstat_rows(*j.args(), X.ctypes.data, nb, X.shape[1], w.ctypes.data, g.ctypes.data, r0, int(init),
                                self.ws.ctypes.data, J.ctypes.data, T.ctypes.data, I.ctypes.data) == 0
        self._J.append(J), self._T.append(T), self._I.append(I)
        return J, T, I

    @property
    def J(self):
        return np.concatenate(self._J, axis=-1)

    @property
    def T(self):
        return np.concatenate(self._T, axis=-1)

    @property
    def I(self):  # noqa: E743
        return np.concatenate(self._I, axis=-1)

    def B(self):
        """The finished moments ``(n_slots, 8)`` and ``V``."""
        s = self.sizes
        return self.ws[s["o_B"]:s["o_B"] + 8 * s["n_slots"]].reshape(-1, 8).copy(), float(self.ws[s["o_V"]])

    def finish(self, var_fit):
        return finish(self.ws, self.jobs.n_picks, self.jobs.q, self.jobs.n_pairs, self.jobs.K, var_fit)


def finish(ws, n_picks, q, n_pairs, K, var_fit) -> dict:
    var_fit = np.ascontiguousarray(var_fit, np.float64).reshape(n_picks, K)
    out = {k: np.full((n_picks, q, K), np.nan) for k in ("main_var", "total_var", "h2_total")}
    out.update({k: np.full((n_picks, n_pairs, K), np.nan) for k in ("inter_var", "h2")})
    bad = C.c_int64(-1)
    lib().hstat_finish(ws.ctypes.data, n_picks, q, n_pairs, K, var_fit.ctypes.data, *(out[k].ctypes.data for k in
                       ("main_var", "total_var", "h2_total", "inter_var", "h2")), C.addressof(bad))
    out["n_nonfinite"] = int(bad.value)
    return out


def whole_call(oracle, pool, fidx, cols, pairs, picks, Xb, v, Xe, w, var_fit=None, block=None) -> tuple:
    """:class:`Reference` run over ``Xb`` and ``Xe`` in blocks of ``block`` rows (``None``: one block each) ->
    ``(the reference, finish(var_fit))``; ``var_fit`` defaults to ones."""
    jobs = Jobs(pool, fidx, np.asarray(Xe).shape[1], cols, pairs, picks)
    ref = Reference(oracle, jobs)
    for X, wt, fn in ((Xb, v, ref.background), (Xe, w, ref.rows)):
        step = X.shape[0] if block is None else block
        for r0 in range(0, X.shape[0], step):
            fn(X[r0:r0 + step], wt[r0:r0 + step], r0, r0 == 0)
    return ref, ref.finish(np.ones((jobs.n_picks, jobs.K)) if var_fit is None else var_fit)


# ------------------------------------------------------------------ the definition, by brute force
def _hybrid(Xe, Xb, S) -> np.ndarray:
    """The ``n_e * n_b`` hybrid rows "row i on the columns S, row r elsewhere", i-major."""
    H = np.repeat(Xb[None, :, :], Xe.shape[0], axis=0)
    for c in S:
        H[:, :, c] = Xe[:, None, c]
    return H.reshape(-1, Xb.shape[1])


def brute_force(pool, trees, a, b, Xe, Xb, v, oracle=None, exact=True) -> dict:
    """The partial dependences of the forest ``trees`` (pool indices) from the definition: ``PD_S(i)[k]`` = the ``v``-
    weighted mean over the background rows of the prediction of the hybrid row, for S = {}, {a}, {b}, {a, b} (``b``
    given) and everything but a.  -> ``{"0", "a", "b", "ab", "-a"}`` of arrays ``(K, n_e)`` -- of ``Fraction`` when
    ``exact`` -- and ``"f"``, the prediction at the rows themselves; ``"abs"``: with ``exact``, the largest sum of the
    absolute terms of any of the hybrid predictions (the S of the error bounds)."""
    Xe, Xb = np.asarray(Xe, np.float64), np.asarray(Xb, np.float64)
    ne, nbk, p = Xe.shape[0], Xb.shape[0], Xe.shape[1]
    K = int(pool.n_outputs)
    table = np.asarray(trees, np.int32)[None, :]
    others = [c for c in range(p) if c != a]
    subsets = {"0": [], "a": [a], "-a": others}
    if b is not None:
        subsets.update({"b": [b], "ab": [a, b]})
    out, worst = {}, Fraction(0)
    if exact:
        vq = [Fraction(float(x)) for x in v]
        V = sum(vq)

    def predict(X):
        nonlocal worst
        if table.shape[1] == 0:
            return np.full((K, X.shape[0]), Fraction(0) if exact else 0.0, dtype=object if exact else np.float64)
        if exact:
            w = ex.walk(pool, table, X)
            worst = max(worst, max(w.S.ravel()))
            return w.R[0]
        return permimp.predict(oracle, pool, table, X)[0]

    for name, S in subsets.items():
        f = predict(_hybrid(Xe, Xb, S)).reshape(K, ne, nbk)
        if exact:
            pd = np.empty((K, ne), dtype=object)
            for k in range(K):
                for i in range(ne):
                    pd[k, i] = sum((vq[r] * f[k, i, r] for r in range(nbk)), Fraction(0)) / V
            out[name] = pd
        else:
            out[name] = (f * v[None, None, :]).sum(axis=2) / v.sum()
    out["f"] = predict(Xe)
    out["abs"] = worst
    return out


# ------------------------------------------------------------------ a backend made of the host references
_array = permimp._array


class HostBackend:
    """What ``friedman_h`` asks of the HIP backend, answered on the host: ``pgb_predict`` is the oracle's, the four
    ``pgb_hstat_*`` entry points are the shim's (the walk's sums by :func:`walk_sums`), the row reduce and the row
    summary are the host builds of their headers.  ``calls`` lists ``(name, nb, q, n_pairs)`` of every hstat call."""

    def __init__(self, oracle, pool):
        from _oracle import NumpyMemory

        self.mem = NumpyMemory()
        self.lib = _HostLibrary(oracle, pool)
        self.calls = self.lib.calls


class _HostLibrary(permimp._HostLibrary):
    def _jobs(self, fidx, n_forests, m, p, cols, q, pairs, n_pairs, picks, n_picks):
        return Jobs(self._pool, _array(fidx, (n_forests, m), np.int32).copy(), p, _array(cols, (q,), np.int32).copy(),
                    _array(pairs, (n_pairs, 2), np.int32).copy() if n_pairs else [], _array(picks, (n_picks,), np.int32).copy())

    def hstat_entry_points(self):
        L = lib()

        def ws_bytes(carr, fidx, n_forests, m, p, cols, q, pairs, n_pairs, picks, n_picks, bytes_out, n_common):
            sizes, common = self._jobs(fidx, n_forests, m, p, cols, q, pairs, n_pairs, picks, n_picks).sizes()
            bytes_out._obj.value = 8 * sizes["words"]
            if n_common is not None and n_pairs:
                _array(n_common, common.shape, np.int32)[...] = common
            self.calls.append(("workspace_bytes", 0, int(q), int(n_pairs)))
            return 0

        def background(carr, fidx, n_forests, m, xd, nb, p, ldx, vd, first_row, init, cols, q, pairs, n_pairs, picks, n_picks,
                       ws, stream):
            j = self._jobs(fidx, n_forests, m, p, cols, q, pairs, n_pairs, picks, n_picks)
            self.calls.append(("background", int(nb), int(q), int(n_pairs)))
            return L.hstat_background(*j.args(), xd, nb, ldx, vd, first_row, init, ws)

        def rows(carr, fidx, n_forests, m, xd, nb, p, ldx, wd, first_row, init, cols, q, pairs, n_pairs, picks, n_picks, ws,
                 jscr, t_rows, i_rows, stream):
            assert ldx == p
            j = self._jobs(fidx, n_forests, m, p, cols, q, pairs, n_pairs, picks, n_picks)
            g = np.ascontiguousarray(walk_sums(self._oracle, j, _array(xd, (nb, p))))
            self.calls.append(("rows", int(nb), int(q), int(n_pairs)))
            return L.hstat_rows(*j.args(), xd, nb, ldx, wd, g.ctypes.data, first_row, init, ws, jscr, t_rows, i_rows)

        def finish_(ws, n_picks, q, n_pairs, K, var_fit, main_var, total_var, h2_total, inter_var, h2, bad, stream):
            self.calls.append(("finish", 0, int(q), int(n_pairs)))
            L.hstat_finish(ws, n_picks, q, n_pairs, K, var_fit, main_var, total_var, h2_total, inter_var, h2, C.addressof(bad._obj))
            return 0

        return ws_bytes, background, rows, finish_

    def rowsummary_entry_point(self):
        import _rowsummary_host as rs

        return lambda *a: rs.lib().rowsum_columns(*a[:-1])
