"""Test helper: a backend that claims to be the HIP library and only writes down what it is asked to do.

:class:`Recorder` is what a sampler's ``_get_backend`` hook returns in ``test_stored_layer.py``: ``lib.backend_name`` is
``"hip-gfx950"``, every ``*_entry_point()`` and ``lib.lib.pgb_predict`` is a function that appends one line to
``trace`` and returns 0, and ``mem`` is :class:`tests._oracle.NumpyMemory` with every allocation and every copy back
logged to the same list.  Buffers stay zero-filled: what the callers compute from them means nothing, the trace does.

A line of the trace is a string.  ``from_host 64x20 float64`` / ``empty 3840 float64`` / ``to_host 3840``: the memory
traffic.  ``pgb_predict trees:6 host 60 3 dev:1280+0 64 ...``: a library call and its arguments in order --

* an integer or a float: a scalar, as it is;
* ``-``: a null pointer;
* ``dev:<elements>+<offset>``: an address inside a LIVE buffer of ``mem`` (its element count, the offset in elements);
  an address inside a buffer that has already been dropped reads ``host`` and so changes the trace;
* ``host``: any other address (an ndarray of the host);
* ``trees:<n>``, ``i64``, ``flags``, ``pwlik(...)`` / ``ppclik(...)``: what was passed by reference -- the structs with
  their scalars and their device pointers spelled as above.
"""

from __future__ import annotations

import ctypes as C
import types
import weakref

import numpy as np

from _oracle import NumpyMemory
from pymc_bart_amd import _abi

ENTRY_POINTS = {"pointwise": "pgb_pointwise_loglik", "psis": "pgb_psis_rows", "psis_expect": "pgb_psis_expect",
                "add_offset": "pgb_add_offset", "ice": "pgb_predict_ice", "pdp": "pgb_predict_pdp",
                "shap": "pgb_predict_shap", "shap_interactions": "pgb_predict_shap_interactions",
                "rowsummary": "pgb_row_summary", "chain_diag": "pgb_chain_diag", "ppc": "pgb_ppc_draw"}
FAMILY_NAMES = {v: k for k, v in _abi.FAMILIES.items()}


class LoggedMemory(NumpyMemory):
    """``NumpyMemory`` that logs into ``trace`` and remembers its live buffers by address."""

    def __init__(self, trace: list):
        self.trace = trace
        self._live = []  # (address, bytes, itemsize, weakref)

    def _keep(self, kind: str, buf):
        self.trace.append(f"{kind} {'x'.join(str(v) for v in buf.shape)} {buf.dtype}")
        self._live.append((buf.ctypes.data, buf.nbytes, buf.itemsize, weakref.ref(buf)))
        return buf

    def from_host(self, arr):
        return self._keep("from_host", NumpyMemory.from_host(arr))

    def empty(self, shape, dtype=np.float64):
        return self._keep("empty", NumpyMemory.empty(shape, dtype))

    def to_host(self, buf):
        self.trace.append(f"to_host {buf.size}")
        return NumpyMemory.to_host(buf)

    @staticmethod
    def is_resident(obj) -> bool:
        return False

    def where(self, address: int) -> str:
        self._live = [e for e in self._live if e[3]() is not None]
        for start, nbytes, itemsize, _ in reversed(self._live):
            if start <= address < start + nbytes:
                return f"dev:{nbytes // itemsize}+{(address - start) // itemsize}"
        return "host"


class Recorder:
    """``be.lib`` / ``be.mem`` of a backend that records (see the module docstring)."""

    def __init__(self):
        self.trace = []
        self.mem = LoggedMemory(self.trace)
        self.lib = _Library(self)

    def spell(self, a) -> str:
        if a is None:
            return "-"
        if isinstance(a, (bool, float)):
            return repr(a)
        if isinstance(a, (int, np.integer)):
            return str(int(a)) if abs(int(a)) < 1 << 40 else self.mem.where(int(a))
        if isinstance(a, C.Array):
            return "flags"
        obj = getattr(a, "_obj", None)  # (ctypes.byref)
        if isinstance(obj, _abi.TreeArraysC):
            return f"trees:{obj.n_trees}"
        if isinstance(obj, C.c_int64):
            return "i64"
        if isinstance(obj, (_abi.PointwiseLik, _abi.PpcLik)):
            name = "pwlik" if isinstance(obj, _abi.PointwiseLik) else "ppclik"
            fields = [FAMILY_NAMES[obj.family], str(obj.n_params)]
            fields += [f"{f[:-4] if f.endswith('_dev') else f}={self.spell(getattr(obj, f))}"
                       for f, _ in obj._fields_[2:] if f != "code_bytes"]
            return f"{name}({','.join(fields)})"
        raise TypeError(f"the recorder cannot spell the argument {a!r}")

    def function(self, name: str):
        def call(*args):
            self.trace.append(" ".join([name] + [self.spell(a) for a in args]))
            return 0

        return call


class _Library:
    backend_name = "hip-gfx950"
    path = "the recording backend"

    def __init__(self, rec: Recorder):
        self.lib = types.SimpleNamespace(**{name: rec.function(name)
                                            for name in ("pgb_predict", "pgb_predict_pdp", "pgb_predict_ice")})
        for stem, name in ENTRY_POINTS.items():
            setattr(self, stem + "_entry_point", (lambda fn: lambda: fn)(rec.function(name)))

    @staticmethod
    def check(rc, what):
        assert rc == 0, what
