"""The one recipe of the host shims ``tests/_*_host.py``: a C source around a header of ``include/`` -- the header the
device kernel compiles -- built with gcc under the flags of the compiled family's host build (``compiled.HOST_FLAGS``:
``-ffp-contract=off``, the numeric contract of every host reference) and opened with ctypes."""
import ctypes as C
import os
import subprocess
import tempfile

from pymc_bart_amd import compiled

_LIBS = {}


def build(name, shim_source, signatures, extra_flags=()) -> C.CDLL:
    """The library of ``shim_source``, built once per ``(name, extra_flags)``.  ``signatures``: function name ->
    ``(restype, argtypes)``; ``argtypes`` None leaves them unset, functions not named keep ctypes' defaults."""
    key = (name, tuple(extra_flags))
    if key not in _LIBS:
        d = tempfile.mkdtemp(prefix=f"pgb_{name}_")
        src, so = os.path.join(d, name + ".c"), os.path.join(d, name + ".so")
        with open(src, "w") as fh:
            fh.write(shim_source)
        subprocess.check_call(["gcc", *compiled.HOST_FLAGS, *extra_flags, f"-I{compiled.INCLUDE}", src, "-o", so, "-lm"])
        L = C.CDLL(so)
        for fn, (restype, argtypes) in signatures.items():
            f = getattr(L, fn)
            f.restype = restype
            if argtypes is not None:
                f.argtypes = argtypes
        _LIBS[key] = L
    return _LIBS[key]
