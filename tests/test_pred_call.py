"""The argument checker the ``pgb_predict_*`` entry points share (``PredCall``, ``csrc/pgb_pred_host.h``), through both
builds of the library and without a GPU: the same bad value given to every entry point that takes ``cols_host`` or
``picks_host`` is refused with the same sentence, prefixed with that entry point's name."""
import ctypes as C

import numpy as np
import pytest

import _pdp_host as host
from pymc_bart_amd import _abi

E_INVALID = -1  # PGB_E_INVALID (include/pgbart.h)
N_FORESTS, M, P, N_ROWS, N_INST, N_COLS, N_PICKS = 4, 3, 3, 8, 2, 2, 3

# entry point -> (its accessor on the library, the index vectors it takes: name -> number of entries)
ENTRY_POINTS = {
    "pgb_predict_ice": ("ice_entry_point", {"cols_host": N_COLS, "picks_host": N_COLS * N_INST * N_PICKS}),
    "pgb_predict_pdp": ("pdp_entry_point", {"cols_host": N_COLS, "picks_host": N_COLS * N_PICKS}),
    "pgb_predict_shap": ("shap_entry_point", {"picks_host": N_PICKS}),
    "pgb_predict_shap_interactions": ("shap_interactions_entry_point", {"cols_host": N_COLS, "picks_host": N_PICKS}),
}
BOUND = {"cols_host": ("p", P), "picks_host": ("n_forests", N_FORESTS)}
CASES = [(fn, vec) for fn, (_, vecs) in ENTRY_POINTS.items() for vec in vecs] + [(fn, "ldx") for fn in ENTRY_POINTS]


def _call(lib, fn, cols, picks, ldx):
    """One call of ``fn`` on the hand-built pool; device pointers are host buffers that are never dereferenced."""
    pool = host.hand_pool()
    carr = pool.as_c()
    fidx = np.array([[0, 1, 2], [3, 4, 5], [6, 0, 2], [4, 5, 5]], np.int32)
    buf = np.zeros(64)
    base = np.zeros(N_PICKS)
    head = (C.byref(carr), fidx.ctypes.data, N_FORESTS, M, buf.ctypes.data, N_ROWS, P, ldx)
    call = getattr(lib, ENTRY_POINTS[fn][0])()
    if fn == "pgb_predict_ice":
        rc = call(*head, buf.ctypes.data, N_INST, P, cols.ctypes.data, N_COLS, picks.ctypes.data, N_PICKS, buf.ctypes.data, None)
    elif fn == "pgb_predict_pdp":
        rc = call(*head, cols.ctypes.data, N_COLS, picks.ctypes.data, N_PICKS, 0, buf.ctypes.data, None, None)
    elif fn == "pgb_predict_shap":
        rc = call(*head, picks.ctypes.data, N_PICKS, buf.ctypes.data, base.ctypes.data, None)
    else:
        rc = call(*head, cols.ctypes.data, N_COLS, picks.ctypes.data, N_PICKS, buf.ctypes.data, base.ctypes.data, None)
    return rc, lib.lib.pgb_last_error().decode()


@pytest.mark.parametrize("max_particles", [64, 128], ids=["libpgbart_hip.so", "libpgbart_hip_p128.so"])
@pytest.mark.parametrize("fn,bad", CASES, ids=[f"{fn}-{bad}" for fn, bad in CASES])
def test_every_entry_point_refuses_the_same_bad_value_with_the_shared_sentence(max_particles, fn, bad):
    lib = _abi.load_hip_library(max_particles)
    vecs = ENTRY_POINTS[fn][1]
    cols = np.arange(N_COLS, dtype=np.int32)
    picks = np.zeros(vecs["picks_host"], np.int32)
    if bad == "ldx":
        rc, msg = _call(lib, fn, cols, picks, P - 1)
        assert rc == E_INVALID and msg == f"{fn}: ldx must be >= p"
        return
    hi_name, hi = BOUND[bad]
    last = vecs[bad] - 1
    (cols if bad == "cols_host" else picks)[last] = hi            # one past the end, at the last position
    rc, msg = _call(lib, fn, cols, picks, P)
    assert rc == E_INVALID and msg == f"{fn}: {bad}[{last}] = {hi} is outside [0, {hi_name} = {hi})"
