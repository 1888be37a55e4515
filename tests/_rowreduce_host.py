"""Host reference of the per-draw averages over rows: a small C shim around ``include/pgbart_rowreduce.h`` -- the header
the device kernels compile -- built with gcc like ``tests/_rowsummary_host.py``.  It exports the header's
``pgb_rowred_block`` and ``pgb_rowred_finish``."""
import ctypes as C

import numpy as np

from _host_build import build

SHIM = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_rowreduce.h"
int rowred_max_groups(void) { return PGB_ROWRED_MAX_GROUPS; }
int rowred_lanes(void) { return PGB_ROWRED_LANES; }
int64_t rowred_ws_doubles(int D, int K, int G, int has_y) { return pgb_rowred_ws_doubles(D, K, G, has_y); }
void rowred_block(const double* a, const double* b, int D, int K, int64_t nb, int64_t ld, const double* w, const int32_t* g,
                  const double* y, const double* off_a, const double* off_b, const double* centre, int G, int transform,
                  int64_t first_row, int init, double* ws, double* v_out) {
  const pgb_lltabs tb = pgb_lltabs_default();
  pgb_rowred_block(a, b, D, K, nb, ld, w, g, y, off_a, off_b, centre, G, transform, first_row, init, &tb, ws, v_out);
}
void rowred_finish(const double* ws, int D, int K, int G, int has_y, const double* centre, double* out, double* w_out,
                   int64_t* counts) {
  pgb_rowred_finish(ws, D, K, G, has_y, centre, out, w_out, counts);
}
/* the whole call in one block, through the header's own pgb_rowred_call */
void rowred_call(const double* a, const double* b, int D, int K, int64_t n, int64_t ld, const double* w, const int32_t* g,
                 const double* y, const double* off_a, const double* off_b, const double* centre, int G, int transform,
                 double* ws, double* v_out, double* out, double* w_out, int64_t* counts) {
  const pgb_lltabs tb = pgb_lltabs_default();
  pgb_rowred_call(a, b, D, K, n, ld, w, g, y, off_a, off_b, centre, G, transform, &tb, ws, v_out, out, w_out, counts);
}
"""

TRANSFORMS = {"identity": 0, "exp": 1, "logistic": 2, "probit": 3}
P = C.c_void_p
SIGNATURES = {"rowred_ws_doubles": (C.c_int64, [C.c_int] * 4),
              "rowred_block": (None, [P, P, C.c_int, C.c_int, C.c_int64, C.c_int64, P, P, P, P, P, P, C.c_int, C.c_int, C.c_int64,
                                      C.c_int, P, P]),
              "rowred_finish": (None, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P]),
              "rowred_call": (None, [P, P, C.c_int, C.c_int, C.c_int64, C.c_int64, P, P, P, P, P, P, C.c_int, C.c_int, P, P, P, P,
                                     P])}


def lib():
    return build("rowred_host", SHIM, SIGNATURES)


def max_groups() -> int:
    return int(lib().rowred_max_groups())


def ws_doubles(D: int, K: int, G: int, has_y: bool) -> int:
    return int(lib().rowred_ws_doubles(D, K, G, int(has_y)))


def _p(x):
    return None if x is None else x.ctypes.data


def _f(x):
    return None if x is None else np.ascontiguousarray(x, np.float64)


def reduce(a, w, g, G, b=None, y=None, off_a=None, off_b=None, centre=None, transform="identity", chunk=None,
           whole_call=False) -> dict:
    """The header on the predictions ``a`` (and ``b``) ``(D, K, n)`` -- the last axis may be a view of a wider array:
    its stride is the leading dimension.  ``w``, ``y`` ``(n,)``, ``g`` ``(n,)`` integers, offsets ``(K, n)``, ``centre``
    ``(K, G)``.  ``chunk``: rows per block (a multiple of 64; ``None``: all at once), the partials carried from block
    to block; ``whole_call``: through ``pgb_rowred_call``.  -> ``out`` ``(2 | 6, D, K, G)``, ``W`` ``(G,)``,
    ``n_nonfinite``, ``n_bad_group``, ``v`` ``(D, K, n)`` and the workspace ``ws``."""
    L = lib()
    a = np.asarray(a, np.float64)
    D, K, n = a.shape
    a, b = np.ascontiguousarray(a), _f(b)
    w, y, off_a, off_b, centre = _f(w), _f(y), _f(off_a), _f(off_b), _f(centre)
    g = np.ascontiguousarray(g, np.int32)
    code = transform if isinstance(transform, int) else TRANSFORMS[transform]
    has_y = y is not None
    ws = np.full(ws_doubles(D, K, G, has_y), 7.5)              # (init must clear it)
    v = np.empty((D, K, n))
    n_out = 6 if has_y else 2
    out, W, counts = np.empty((n_out, D, K, G)), np.empty(G), np.zeros(2, np.int64)
    if whole_call:
        L.rowred_call(_p(a), _p(b), D, K, n, n, _p(w), _p(g), _p(y), _p(off_a), _p(off_b), _p(centre), G, code, _p(ws), _p(v),
                      _p(out), _p(W), _p(counts))
    else:
        step = n if chunk is None else int(chunk)
        assert step == n or step % 64 == 0
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            nb = r1 - r0
            blk = lambda m: None if m is None else np.ascontiguousarray(m[..., r0:r1])  # noqa: E731
            ab, bb, vb = blk(a), blk(b), np.empty((D, K, nb))
            L.rowred_block(_p(ab), _p(bb), D, K, nb, nb, _p(blk(w)), _p(blk(g)), _p(blk(y)), _p(blk(off_a)), _p(blk(off_b)),
                           _p(centre), G, code, r0, int(r0 == 0), _p(ws), _p(vb))
            v[:, :, r0:r1] = vb
        L.rowred_finish(_p(ws), D, K, G, int(has_y), _p(centre), _p(out), _p(W), _p(counts))
    return {"out": out, "W": W, "n_nonfinite": int(counts[0]), "n_bad_group": int(counts[1]), "v": v, "ws": ws}


def public(pred, weights=None, groups=None, pred_b=None, y=None, offset=None, offset_b=None, transform="identity") -> dict:
    """The header's numbers in the layout of ``pymc_bart_amd.average``: ``pred`` ``(D, K, n)`` as ``sample_posterior``
    returns it."""
    D, K, n = pred.shape
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    labels, gid = (np.zeros(1, np.int64), np.zeros(n, np.int64)) if groups is None else np.unique(groups, return_inverse=True)
    G = labels.size
    centre = None
    if y is not None:
        y = np.asarray(y, np.float64)
        centre = (np.bincount(gid, weights=w * y, minlength=G) / np.bincount(gid, weights=w, minlength=G))[None, :]
    r = reduce(pred, w, gid, G, pred_b, y, offset, offset_b, centre, transform)
    out = np.moveaxis(r["out"], 2, 3)                             # (n_out, D, G, K)
    res = {"group_labels": labels, "weight": r["W"], "n_rows": np.bincount(gid, minlength=G), "n_draws": D,
           "n_nonfinite": r["n_nonfinite"], "v": r["v"]}
    if y is None:
        res["mean"] = out[0]
    else:
        for j, name in enumerate(("mean", "var_fit", "bias", "mse", "var_res", "r2")):
            if name != "mean":
                res[name] = out[j, :, :, 0]
        res["rmse"] = np.sqrt(res["mse"])
    return res
