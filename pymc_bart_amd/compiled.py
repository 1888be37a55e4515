"""Custom per-row likelihoods compiled at run time: family ``"compiled"`` (``include/pgbart_compiled.h``).

The user writes the log-density of ONE observation as a short C function body -- and, optionally, a SAMPLER body: how
to draw one observation.  One build path (:func:`_build`) turns a body into a gfx950 code object and a host library,
both from committed units that read the same two generated files; how a body becomes a function is stated once, in
``include/pgbart_compiled_body.h``.  The kinds of build (``_KINDS``):

* ``pass`` (:func:`compile_loglik`): ``csrc/k_loglik_compiled.hip`` -- the library's log-likelihood pass with the body
  at every evaluation site, for one particle build, ``n_outputs = K`` predictors (``mu[0] .. mu[K-1]``) and constant
  or, with ``linear=True``, linear leaves (``response="linear"`` / ``"mix"``).  The HIP library loads it
  (``pgb_set_loglik_code``) and the chain stays device-resident: no host round trip per SMC round;
* ``pointwise`` (``compile_loglik(..., pointwise=True)``): ``csrc/k_pointwise_compiled.hip`` -- the body inside the
  posterior tree walk, for scoring a fit (:mod:`pymc_bart_amd.pointwise`);
* ``sampler`` (:func:`compile_sampler`): ``csrc/k_ppc_compiled.hip`` -- the sampler body inside the replicating kernel
  (:mod:`pymc_bart_amd.predictive`).

The host build (gcc, the oracle's flags) of a density is ``csrc/h_loglik_compiled.c``: for one output a function with
the ``pgb_loglik_fn`` signature, which any CPU backend runs as family ``"callback"`` -- natively, no Python in the
per-row loop; for K outputs (no CPU backend runs those: the callback family has one output and constant leaves) an
evaluator of rows that the device's probe kernel is held to.  That of a sampler body is ``csrc/h_ppc_compiled.c``, the
reference of the device's draws.  Both sides evaluate a body with the same vocabulary (table-driven ``exp`` / ``log`` /
``log_ndtr`` / ``softplus`` / ``lgamma`` on the tables of ``include/pgbart_spec.h``, explicit comparisons), so that the
CPU checks the GPU bit for bit.  Builds are cached on disk (``$PGB_JIT_CACHE``, default
``~/.cache/pymc_bart_amd/jit``) under a key over everything that goes into them.
"""

from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import tempfile
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")
#: the kinds of build (the layout record's marks 0, 1, 2): the device unit, the host unit, the kernel whose resources
#: are reported, the device build's extra defines.  The kind is part of the cache key (``cache_key``) and decides the
#: meta record (``_build``); only a pass object depends on the particle build and on the kind of leaves
_PARTICLES = "-DPGB_MAX_PARTICLES={mp}"
_KINDS = {
    "pass": ("k_loglik_compiled.hip", "h_loglik_compiled.c", "k_loglik_compiled", [_PARTICLES]),
    "pointwise": ("k_pointwise_compiled.hip", "h_loglik_compiled.c", "k_pointwise_compiled", [_PARTICLES]),
    "sampler": ("k_ppc_compiled.hip", "h_ppc_compiled.c", "k_ppc_compiled", []),
}
LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")

#: the library's device flags (``__graft_entry__.HIPCC_FLAGS`` without ``-fPIC`` / ``-shared``; a test holds them equal)
DEVICE_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17",
    "-ffp-contract=off",
    f"-I{INCLUDE}",
    "-mllvm", "-amdgpu-kernarg-preload-count=16",
]
#: what turns the unit into one raw gfx950 code object (an ELF the runtime loads with hipModuleLoadData)
GENCO_FLAGS = ["--genco", "--no-gpu-bundle-output"]
#: the host build: the oracle's flags
HOST_FLAGS = ["-O2", "-std=gnu11", "-ffp-contract=off", "-fPIC", "-shared"]

MAX_PARAMS = 8
MAX_OUTPUTS = 16  # PGB_MAX_OUTPUTS
#: what a body may call (include/pgbart_compiled.h, section "vocabulary")
VOCABULARY = {
    "exp": "exp(x): pgb_exp_t, the spec's table-driven exponential",
    "log": "log(x): pgb_log_t (x <= 0 -> -1e300, NaN stays NaN)",
    "log_ndtr": "log_ndtr(x): log Phi(x), pgb_lphi_t",
    "softplus": "softplus(x): log(1 + e^x), pgb_softplus_t",
    "fabs": "fabs(x): x < 0 ? -x : x + 0.0",
    "fmin": "fmin(a, b): a < b ? a : b",
    "fmax": "fmax(a, b): a > b ? a : b",
    "lgamma": "lgamma(x): log Gamma(x) for x > 0 (NaN otherwise), on the log table",
}
#: what a SAMPLER body may call on top of it (include/pgbart_ppc.h, "SAMPLER BODIES"); never a density body
RANDOM_VOCABULARY = {
    "uniform": "uniform(): a uniform in [0, 1)",
    "uniform_open": "uniform_open(): a uniform in (0, 1), for a logarithm",
    "normal": "normal(): a standard normal",
    "gamma": "gamma(a): Gamma(a, 1), Marsaglia-Tsang (pgb_ppc_gamma)",
    "poisson": "poisson(lam): Poisson(lam), inversion below 10 and PTRS from there (pgb_ppc_poisson)",
    "sqrt": "sqrt(x): pgb_psis_sqrt",
    "floor": "floor(x): pgb_ppc_floor",
}
_EXPLOG = ("exp", "log", "softplus", "lgamma")
_C_KEYWORDS = {
    "auto", "break", "case", "char", "const", "continue", "default", "do", "double", "else", "enum", "extern",
    "float", "for", "goto", "if", "inline", "int", "long", "register", "restrict", "return", "short", "signed",
    "sizeof", "static", "struct", "switch", "typedef", "union", "unsigned", "void", "volatile", "while", "asm",
    "_Bool", "_Thread_local", "bool", "true", "false", "class", "template", "this", "new", "delete", "namespace",
    "using", "operator", "typename", "virtual", "constexpr", "thread_local", "static_assert", "alignas", "alignof",
}
#: keywords a body may not use: storage that would outlive the call, declarations outside the function
_REFUSED_KEYWORDS = {"static", "extern", "register", "volatile", "_Thread_local", "thread_local", "typedef", "goto",
                     "struct", "union", "enum", "class", "template", "namespace", "using", "operator", "new", "delete",
                     "asm", "inline"}
_CALLABLE_KEYWORDS = {"if", "while", "for", "switch", "return", "sizeof", "int", "double", "float", "long", "unsigned",
                      "signed", "char", "short", "const"}
_IDENT = re.compile(r"[A-Za-z_][A-Za-z0-9_]*")


class CompileError(RuntimeError):
    """A body the compilers refuse (or one that calls a function outside the vocabulary)."""


def vocabulary_text(sampler: bool = False) -> str:
    words = list(VOCABULARY.values()) + (list(RANDOM_VOCABULARY.values()) if sampler else [])
    return "; ".join(words) + "; plus + - * /, comparisons, ?:, if, local double / int variables"


# ---------------------------------------------------------------------------------------------------- validation
def _strip_comments(body: str) -> str:
    body = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), body, flags=re.S)
    return re.sub(r"//[^\n]*", "", body)


def check_outputs(n_outputs) -> int:
    if isinstance(n_outputs, bool) or int(n_outputs) != n_outputs or not 1 <= int(n_outputs) <= MAX_OUTPUTS:
        raise ValueError(f"n_outputs must be an integer in [1, {MAX_OUTPUTS}], got {n_outputs!r}")
    return int(n_outputs)


def validate(body: str, param_names, n_outputs: int = 1, sampler: bool = False) -> tuple[str, ...]:
    """Refuse, before any compiler runs, what the body may not contain.  Returns the param names as a tuple.
    ``sampler``: the body is a SAMPLER body -- it may call the random vocabulary too, has no ``y``, and no param may
    carry a name of the random vocabulary."""
    what = "sampler" if sampler else "likelihood"
    vocabulary = {**VOCABULARY, **RANDOM_VOCABULARY} if sampler else VOCABULARY
    if not isinstance(body, str) or not body.strip():
        raise ValueError(f"the {'sampler ' if sampler else ''}body must be a non-empty string of C statements")
    K = check_outputs(n_outputs)
    names = tuple(param_names)
    if len(names) > MAX_PARAMS:
        raise ValueError(f"at most {MAX_PARAMS} params, {len(names)} given")
    seen = set()
    for nm in names:
        if not isinstance(nm, str) or not re.fullmatch(r"[A-Za-z_][A-Za-z0-9_]*", nm):
            raise ValueError(f"param name {nm!r} is not a C identifier")
        if nm in ("y", "mu", "aux"):
            raise ValueError(f"param name {nm!r} clashes with the body's arguments y, mu, aux")
        if K > 1 and nm == "K":
            raise ValueError("param name 'K' is reserved: a body of n_outputs >= 2 reads its number of outputs as K")
        if nm in vocabulary:
            raise ValueError(f"param name {nm!r} clashes with the vocabulary ({', '.join(vocabulary)})"
                             + (": a likelihood with a sampler body reserves the random vocabulary's names"
                                if nm in RANDOM_VOCABULARY else ""))
        if nm in _C_KEYWORDS:
            raise ValueError(f"param name {nm!r} is a C keyword")
        if nm.startswith("__") or nm.lower().startswith("pgb_"):
            raise ValueError(f"param name {nm!r}: names starting with '__' or 'pgb_' are reserved")
        if nm in seen:
            raise ValueError(f"duplicate param name {nm!r}")
        seen.add(nm)
    for lineno, line in enumerate(body.splitlines(), 1):
        if line.lstrip().startswith("#") or line.lstrip().startswith("%:"):
            raise ValueError(f"line {lineno}: preprocessor lines are not allowed in a {what} body: {line.strip()!r}")
    # (on the raw text: no line splice can move code into or out of a comment)
    for bad, thing in (("#", "'#' (preprocessor)"), ("%:", "'%:' (preprocessor digraph)"), ("??", "'??' (trigraph)"),
                      ("\\", "a backslash")):
        if bad in body:
            raise ValueError(f"the body contains {thing}: not allowed in a {what} body")
    code = _strip_comments(body)
    for bad, thing in (('"', "a string literal"), ("'", "a character literal")):
        if bad in code:
            raise ValueError(f"the body contains {thing}: not allowed in a {what} body")
    for m in _IDENT.finditer(code):
        tok = m.group(0)
        if tok in ("asm", "__asm__", "__asm") or tok.startswith("__asm"):
            raise ValueError(f"inline assembly ({tok!r}) is not allowed in a {what} body")
        if tok.startswith("__builtin"):
            raise ValueError(f"compiler builtins ({tok!r}) are not allowed in a {what} body; the vocabulary: "
                             + ", ".join(vocabulary))
        if tok.startswith("__"):
            raise ValueError(f"identifiers starting with '__' ({tok!r}) are reserved")
        if tok.lower().startswith("pgb_"):
            raise ValueError(f"identifiers starting with 'pgb_' ({tok!r}) are reserved for the prelude")
        if tok in _REFUSED_KEYWORDS:
            raise ValueError(f"{tok!r} is not allowed in a {what} body (local double / int variables only)")
        if sampler and tok == "y":
            lineno = code.count("\n", 0, m.start()) + 1
            raise ValueError(f"line {lineno}: a sampler body has no y -- it returns one replicated observation from "
                             f"mu, aux and the params:\n    {body.splitlines()[lineno - 1].strip()}")
    depth = 0
    for ch in code:  # the body stays inside its function
        depth += ch == "{"
        depth -= ch == "}"
        if depth < 0:
            raise ValueError("unbalanced '}' in the body")
    if depth != 0:
        raise ValueError("unbalanced '{' in the body")
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_]*)\s*\(", code):
        fn = m.group(1)
        if fn in vocabulary or fn in _CALLABLE_KEYWORDS:
            continue
        lineno = code.count("\n", 0, m.start()) + 1
        raise CompileError(f"line {lineno}: {fn!r} is not in the {what} vocabulary"
                           + (" (the random vocabulary belongs to sampler bodies)" if fn in RANDOM_VOCABULARY else "")
                           + f":\n    {body.splitlines()[lineno - 1].strip()}\nthe vocabulary: {vocabulary_text(sampler)}")
    if K > 1:
        for m in re.finditer(r"\bmu\b(\s*\[\s*([0-9]+)\s*\])?", code):
            lineno = code.count("\n", 0, m.start()) + 1
            src = body.splitlines()[lineno - 1].strip()
            if m.group(1) is None and not re.match(r"\s*\[", code[m.end():]):
                raise CompileError(f"line {lineno}: mu holds K = {K} predictors, it is not a scalar: write mu[0] .. "
                                   f"mu[{K - 1}]\n    {src}")
            if m.group(2) is not None and int(m.group(2)) >= K:
                raise ValueError(f"line {lineno}: mu[{m.group(2)}] is out of range: mu holds K = {K} predictors "
                                 f"(mu[0] .. mu[{K - 1}])\n    {src}")
        for m in re.finditer(r"\b(?:int|double|float|long|short|char|unsigned|signed)\s+K\b", code):
            raise ValueError("'K' is reserved: a body of n_outputs >= 2 reads its number of outputs as K")
    return names


def uses_tables(body: str) -> bool:
    """Whether the body calls exp / log / softplus / lgamma (the kernel then stages their tables in LDS)."""
    code = _strip_comments(body)
    return any(re.search(rf"\b{f}\s*\(", code) for f in _EXPLOG)


# ---------------------------------------------------------------------------------------------------- keys, cache
def _header_files() -> list[str]:
    """What ``PGB_HEADERS_HASH`` covers, by rule: the headers of ``include/`` and ``csrc/`` and the units compiled at
    run time, ``csrc/*_compiled.hip`` (device) and ``csrc/*_compiled.c`` (host).  ``__graft_entry__.build`` rebuilds
    the library when one of them is newer."""
    files = [os.path.join(INCLUDE, f) for f in sorted(os.listdir(INCLUDE)) if f.endswith(".h")]
    return files + [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC))
                    if f.endswith((".h", "_compiled.hip", "_compiled.c"))]


def headers_hash() -> int:
    """64-bit hash of every file a code object, a host build and the library are built from (:func:`_header_files`):
    the library is compiled with it (``-DPGB_HEADERS_HASH``) and refuses a code object that carries another."""
    h = hashlib.sha256()
    for f in _header_files():
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    v = int.from_bytes(h.digest()[:8], "little")
    return v or 1


def hipcc_path() -> str:
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


_HIPCC_VERSION: dict = {}


def _hipcc_version(hipcc: str) -> str:
    if hipcc not in _HIPCC_VERSION:
        _HIPCC_VERSION[hipcc] = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout
    return _HIPCC_VERSION[hipcc]


def cache_dir() -> str:
    return os.environ.get("PGB_JIT_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "pymc_bart_amd", "jit")


def cache_key(body: str, param_names, max_particles: int = 64, n_outputs: int = 1, linear: bool = False,
              pointwise: bool = False, sampler: bool = False) -> str:
    kind = "sampler" if sampler else "pointwise" if pointwise else "pass"
    h = hashlib.sha256()
    h.update(json.dumps({"kind": kind, "body": body, "params": list(param_names), "max_particles": int(max_particles),
                         "n_outputs": int(n_outputs), "linear": bool(linear),
                         "device_flags": DEVICE_FLAGS + GENCO_FLAGS, "host_flags": HOST_FLAGS,
                         "headers_hash": headers_hash(), "hipcc": _hipcc_version(hipcc_path())},
                        sort_keys=True).encode())
    return h.hexdigest()[:32]


def _write_atomic(path: str, data: bytes) -> None:
    d = os.path.dirname(path)
    fd, tmp = tempfile.mkstemp(dir=d, prefix=".tmp_", suffix=os.path.basename(path))
    try:
        with os.fdopen(fd, "wb") as fh:
            fh.write(data)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


# ---------------------------------------------------------------------------------------------------- the builds
def _body_defs(names, explog: bool, n_outputs: int = 1, linear: bool = False) -> str:
    """``pgb_compiled_body.inc``: what both compilers know about a body besides its text."""
    return "\n".join([
        f"#define PGB_COMPILED_NPARAMS {len(names)}",
        f"#define PGB_COMPILED_NOUT {int(n_outputs)}",
        f"#define PGB_COMPILED_LINEAR {1 if linear else 0}",
        f"#define PGB_COMPILED_EXPLOG {1 if explog else 0}",
        f"#define PGB_HEADERS_HASH {headers_hash()}ull",
        "#define PGB_COMPILED_PARAMS " + "".join(f", const double {nm}" for nm in names),
        "#define PGB_COMPILED_ARGV(V) " + "".join(f", (V)[{i}]" for i in range(len(names))),
        "#define PGB_COMPILED_ARGS(P) PGB_COMPILED_ARGV((P).v)",
        "",
    ])


def _body_text(body: str, sampler: bool = False) -> str:
    """``pgb_compiled_body_text.inc``: compiler messages count the user's lines."""
    return f'#line 1 "{"sampler" if sampler else "loglik"} body"\n' + body + "\n"


def _compile_error(stderr: str, body: str, side: str, sampler: bool = False) -> CompileError:
    lines = body.splitlines()
    msgs = []
    for m in re.finditer(r"(?:loglik|sampler) body:(\d+):(?:\d+:)?\s*(?:fatal )?error:\s*(.*)", stderr):
        ln = int(m.group(1))
        src = lines[ln - 1].strip() if 1 <= ln <= len(lines) else ""
        msgs.append(f"line {ln}: {m.group(2).strip()}\n    {src}")
    if not msgs:
        tail = [ln for ln in stderr.splitlines() if "error" in ln][:5]
        msgs = tail or [stderr.strip()[-2000:]]
    return CompileError(f"the {'sampler' if sampler else 'likelihood'} body does not compile ({side}):\n"
                        + "\n".join(msgs[:5]) + f"\nthe vocabulary: {vocabulary_text(sampler)}")


def kernel_resources(code_object_path: str, kernel: str = "k_loglik_compiled") -> dict:
    """VGPR / SGPR / scratch / LDS / spills / workgroups per CU of ``kernel``, from the code object's
    metadata note -- the way tools/occupancy_guard.py reads the library's."""
    import yaml

    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", code_object_path], text=True)
    start = notes.index("---\n") + 4
    end = notes.index("\n...", start) if "\n..." in notes[start:] else len(notes)
    meta = yaml.safe_load(notes[start:end])
    for k in meta["amdhsa.kernels"]:
        if k[".name"] == kernel:  # (not the probe: its resources do not matter)
            vg, ag = int(k[".vgpr_count"]), int(k.get(".agpr_count", 0))
            lds = int(k[".group_segment_fixed_size"])
            unified = ((vg + 3) // 4) * 4 + ag
            alloc = -(-unified // 8) * 8
            waves = max(1, min(8, 512 // max(alloc, 8)))
            wgs = min(waves * 4 // 4, (160 * 1024) // lds if lds else 1 << 30, 8)
            return {"vgpr": vg, "agpr": ag, "sgpr": int(k[".sgpr_count"]), "lds_bytes": lds,
                    "scratch_bytes": int(k[".private_segment_fixed_size"]),
                    "vgpr_spills": int(k.get(".vgpr_spill_count", 0)), "sgpr_spills": int(k.get(".sgpr_spill_count", 0)),
                    "wgs_per_cu": wgs}
    raise CompileError(f"the code object has no kernel {kernel}")


class _Build:
    """One build of a body: the code object (``code``), the host library (``host_lib``), the kernel's resource usage
    (``resources``), the cache ``key``; ``compile_seconds`` is 0.0 on a cache hit."""

    def __init__(self, key, body, param_names, code, host_lib, resources, compile_seconds, cached, n_outputs=1):
        self.key, self.body, self.param_names = key, body, tuple(param_names)
        self.n_outputs = int(n_outputs)
        self.code, self.host_lib, self.resources = code, host_lib, resources
        self.compile_seconds, self.cached = compile_seconds, cached
        self._host = None

    @property
    def n_params(self) -> int:
        return len(self.param_names)

    def _host_fn(self, name: str, argtypes):
        """The host build's entry point ``name`` as a ctypes function, loaded at its first use."""
        if self._host is None:
            self._host = getattr(C.CDLL(self.host_lib), name)
            self._host.restype, self._host.argtypes = C.c_int, argtypes
        return self._host


class CompiledLoglik(_Build):
    """The build of a density body.  ``linear``: the code object's pass kernel is the linear-leaf pass (a sampler with
    ``response="linear"`` / ``"mix"`` takes it, one with constant leaves refuses it, and the other way round).
    ``pointwise``: the code object holds ``k_pointwise_compiled`` instead of a pass kernel."""

    def __init__(self, *args, max_particles=64, linear=False, pointwise=False):
        super().__init__(*args)
        self.max_particles, self.linear, self.pointwise = int(max_particles), bool(linear), bool(pointwise)

    def host_function(self):
        """The host build's ``pgb_compiled_loglik`` as a ctypes function (``pgb_loglik_fn``)."""
        from . import _abi

        if self.n_outputs > 1:
            raise CompileError(f"a body of {self.n_outputs} outputs has no callback: no CPU backend runs a K-vector "
                               "compiled likelihood (see host_eval)")
        if self._host is None:
            self._host = _abi.LOGLIK_FN(("pgb_compiled_loglik", C.CDLL(self.host_lib)))
        return self._host

    def host_eval(self, y, mu, aux=None, params=()):
        """The host build of a K-vector body on given rows: ``mu`` is [K][n]; the values are clamped like the
        sampler takes them ([-2047, 2047], NaN -> -2047)."""
        if self.n_outputs < 2:
            raise CompileError("host_eval is the evaluator of a K-vector body (n_outputs >= 2)")
        y = np.ascontiguousarray(y, np.float64).ravel()
        n = y.size
        mu = np.ascontiguousarray(mu, np.float64)
        if mu.shape != (self.n_outputs, n):
            raise ValueError(f"mu must be [K][n] = ({self.n_outputs}, {n}), got {mu.shape}")
        ctx = CompiledContext()
        keep = None
        if aux is not None:
            keep = np.ascontiguousarray(aux, np.float64).ravel()
            if keep.size != n:
                raise ValueError(f"aux must hold n = {n} values")
            ctx.aux = keep.ctypes.data
        for i, v in enumerate(params):
            ctx.params[i] = float(v)
        f = self._host_fn("pgb_compiled_eval_rows", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])
        out = np.empty(n)
        rc = f(C.cast(C.pointer(ctx), C.c_void_p), y.ctypes.data, mu.ctypes.data, n, out.ctypes.data)
        if rc != 0:
            raise CompileError(f"pgb_compiled_eval_rows returned {rc}")
        return out


class CompiledContext(C.Structure):
    """``ctx`` of the host build: the aux column (or NULL) and the params."""

    _fields_ = [("aux", C.c_void_p), ("params", C.c_double * MAX_PARAMS)]


class CompiledSampler(_Build):
    """The build of a SAMPLER body: the code object holds ``k_ppc_compiled`` (mark 2)."""

    def host_draw(self, mu, params=None, aux=None, seed=0, row0=0, y=None):
        """The host build of the body over ``mu`` ``(D, K, n)`` (the offset already added), ``params``
        ``(D, n_params)``, ``aux`` ``(n,)`` or ``None``, at global rows ``row0 ..`` -> (values ``(D, n)``, PIT counts
        ``(2, n)`` int32 against ``y`` or ``None``, ``(n_capped, n_exhausted)``): what ``pgb_ppc_draw_compiled`` gives
        for the same arguments, bit for bit."""
        mu = np.ascontiguousarray(mu, np.float64)
        if mu.ndim != 3 or mu.shape[1] != self.n_outputs:
            raise ValueError(f"mu must be (D, K, n) with K = {self.n_outputs}, got {mu.shape}")
        D, _, n = mu.shape
        par = np.zeros((D, 0)) if params is None else np.ascontiguousarray(params, np.float64).reshape(D, -1)
        if par.shape[1] != self.n_params:
            raise ValueError(f"params must be (D, {self.n_params}), got {par.shape}")
        ax = None if aux is None else np.ascontiguousarray(aux, np.float64).ravel()
        if ax is not None and ax.size != n:
            raise ValueError(f"aux must hold n = {n} values")
        yy = None if y is None else np.ascontiguousarray(y, np.float64).ravel()
        if yy is not None and yy.size != n:
            raise ValueError(f"y must hold n = {n} values")
        f = self._host_fn("pgb_compiled_draw", [C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
        out = np.empty((D, n))
        pit = None if yy is None else np.zeros((2, n), np.int32)
        flags = np.zeros(2, np.int64)
        rc = f(mu.ctypes.data, D, n, int(row0), par.ctypes.data if par.size else None, self.n_params,
               None if ax is None else ax.ctypes.data, int(seed), out.ctypes.data,
               None if yy is None else yy.ctypes.data, None if pit is None else pit.ctypes.data, flags.ctypes.data)
        if rc != 0:
            raise CompileError(f"pgb_compiled_draw returned {rc}")
        return out, pit, (int(flags[0]), int(flags[1]))


def _build(kind: str, body: str, names, mp: int = 64, K: int = 1, linear: bool = False):
    """The one build path of every kind of ``_KINDS``: the cache entry of the key, or -- in a temporary directory --
    the two generated files, the host build (first: quick, and the compiler's messages about the body are the same on
    either side), the device build and its kernel's resources; then the entry's three files, written atomically."""
    (device, host_unit, kernel, defines), sampler, pointwise = _KINDS[kind], kind == "sampler", kind == "pointwise"
    key = cache_key(body, names, mp, K, linear, pointwise, sampler)
    root = cache_dir()
    os.makedirs(root, exist_ok=True)
    co_path, so_path, meta_path = (os.path.join(root, key + ext) for ext in (".co", ".so", ".json"))

    def result(code, resources, seconds, cached):
        if sampler:
            return CompiledSampler(key, body, names, code, so_path, resources, seconds, cached, K)
        return CompiledLoglik(key, body, names, code, so_path, resources, seconds, cached, K,
                              max_particles=mp, linear=linear, pointwise=pointwise)

    if os.path.exists(meta_path) and os.path.exists(co_path) and os.path.exists(so_path):
        with open(meta_path) as fh:
            meta = json.load(fh)
        with open(co_path, "rb") as fh:
            return result(fh.read(), meta["resources"], 0.0, True)
    t0 = time.perf_counter()
    with tempfile.TemporaryDirectory(prefix="pgb_jit_") as tmp:
        with open(os.path.join(tmp, "pgb_compiled_body.inc"), "w") as fh:
            fh.write(_body_defs(names, not sampler and uses_tables(body), K, linear))
        with open(os.path.join(tmp, "pgb_compiled_body_text.inc"), "w") as fh:
            fh.write(_body_text(body, sampler))
        so_tmp, co_tmp = os.path.join(tmp, "host.so"), os.path.join(tmp, "k.co")
        for side, cmd in (
                ("host", ["gcc", *HOST_FLAGS, "-Werror=implicit-function-declaration", f"-I{INCLUDE}", f"-I{tmp}",
                          os.path.join(CSRC, host_unit), "-o", so_tmp, "-lm"]),
                ("device", [hipcc_path(), *DEVICE_FLAGS, *GENCO_FLAGS, *(d.format(mp=mp) for d in defines),
                            f"-I{CSRC}", f"-I{tmp}", "-w", os.path.join(CSRC, device), "-o", co_tmp])):
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise _compile_error(r.stderr, body, side, sampler)
        resources = kernel_resources(co_tmp, kernel)
        seconds = time.perf_counter() - t0
        with open(co_tmp, "rb") as fh:
            code = fh.read()
        with open(so_tmp, "rb") as fh:
            host = fh.read()
    _write_atomic(co_path, code)
    _write_atomic(so_path, host)
    meta = {"sampler": body} if sampler else {"body": body, "max_particles": mp, "linear": linear, "pointwise": pointwise}
    meta.update(params=list(names), n_outputs=K, resources=resources, compile_seconds=seconds)
    _write_atomic(meta_path, json.dumps(meta, indent=1).encode())  # (last: an entry is complete once it exists)
    return result(code, resources, seconds, False)


def _warn_scratch(b: CompiledLoglik) -> None:
    if b.pointwise:  # (the walk's own stack of the marginalising path lives in scratch: nothing about the body)
        return
    if (b.n_outputs > 1 or b.linear) and b.resources.get("scratch_bytes", 0) > 0:
        warnings.warn(f"the likelihood body of {b.n_outputs} outputs{' (linear leaves)' if b.linear else ''} puts "
                      f"{b.resources['scratch_bytes']} B per thread "
                      "in scratch memory: mu lives in registers, and a run-time index such as mu[(int)y] moves it "
                      "out.  Pick by comparison instead -- for (int k = 0; k < K; ++k) if (k == c) m = mu[k]; -- "
                      "which is what the built-in softmax does", RuntimeWarning, stacklevel=3)


def compile_loglik(body: str, param_names=(), max_particles: int = 64, n_outputs: int = 1,
                   linear: bool = False, pointwise: bool = False) -> CompiledLoglik:
    """Compile ``body`` (see :class:`pymc_bart_amd.CompiledLikelihood`) for the particle build ``max_particles``
    (64 or 128) and ``n_outputs`` predictors -- or take it from the cache.  ``linear``: the code object's pass is
    the linear-leaf one (``response="linear"`` / ``"mix"``) instead of the constant-leaf one.  ``pointwise``: a code
    object of its own kind -- no pass kernel but ``k_pointwise_compiled``, the body inside the posterior tree walk
    (:mod:`pymc_bart_amd.pointwise`); it serves every kind of leaves and either particle build."""
    K = check_outputs(n_outputs)
    names = validate(body, param_names, K)
    if pointwise and linear:
        raise ValueError("pointwise=True takes no linear=True: the walk applies the leaves' slopes itself")
    # (the pointwise kernel reads no particle record: one object for both builds)
    mp = 128 if int(max_particles) > 64 and not pointwise else 64
    b = _build("pointwise" if pointwise else "pass", body, names, mp, K, bool(linear))
    _warn_scratch(b)
    return b


def compile_sampler(body: str, param_names=(), n_outputs: int = 1) -> CompiledSampler:
    """Compile the SAMPLER body ``body`` (see :class:`pymc_bart_amd.CompiledLikelihood`) of ``n_outputs`` predictors
    into ``k_ppc_compiled`` (``csrc/k_ppc_compiled.hip``) and its host evaluator -- or take them from the cache.  The
    kernel reads no particle record: one object serves both particle builds."""
    K = check_outputs(n_outputs)
    return _build("sampler", body, validate(body, param_names, K, sampler=True), K=K)


class CompiledLikelihood:
    """A per-row log-likelihood written as a C function body, compiled for the GPU at run time.

    ``body`` is the inside of ``double f(double y, double mu, double aux, const double <param>...)``:

    * ``y``   the observed value of the row, ``mu`` its linear predictor (sum of trees plus offset) -- with
      ``n_outputs = K >= 2`` the K predictors ``mu[0] .. mu[K-1]`` (``K`` is a constant the body can read; the
      variable then has shape ``(K, n)``),
    * ``aux`` the row's entry of the optional per-row column ``aux`` (0.0 without one),
    * one ``const double`` per entry of ``params`` (at most 8), in the order given.

    ``params`` maps each name to a number or to the name of a point variable (read like the built-in families'
    parameters: a number, a shared variable, a callable, or a key of the point).

    The vocabulary: IEEE ``+ - * /``, comparisons, ``?:``, ``if``, local ``double`` and ``int`` variables, and
    ``exp``, ``log`` (the spec's table functions), ``log_ndtr`` (log Phi), ``softplus`` (log(1 + e^x)), ``lgamma``
    (log Gamma on the log table), ``fabs``, ``fmin``, ``fmax`` (explicit comparisons).  Nothing from libm (no ``sqrt``, ``pow``): the same body must give the
    same bits on the GPU and on the CPU.  No preprocessor lines, no ``asm``, no ``__``-names.

    The value is clamped to [-2047, 2047] (NaN -> -2047) and summed in fixed point exactly like family
    ``"callback"``; on the GPU the evaluation runs inside the sampler's own likelihood kernel.

    Leaves: any ``response`` of the ``BARTOp`` -- ``"constant"``, ``"linear"``, ``"mix"`` -- with one output or K, like
    the built-in families.  ``mu`` then includes the leaf's slope term; the body does not know about leaves.  The
    linear-leaf pass is a code object of its own (``compiled(max_particles, linear=True)``), built when a sampler
    with such a response first asks for it.  Linear / mix leaves of a compiled likelihood run on the HIP backend
    only (a CPU backend runs the body as its callback family, which has constant leaves).

    >>> CompiledLikelihood("double u = (y - mu) / b;  return -(u * (u < 0.0 ? q - 1.0 : q));",
    ...                    params={"b": 0.25, "q": "q_var"})            # doctest: +SKIP

    ``sampler`` (optional) says how to DRAW one observation: the inside of ``double r(double mu, double aux, const
    double <param>...)`` -- the same ``mu`` (or ``mu[0] .. mu[K-1]``), ``aux`` and params, and no ``y`` (a sampler body
    that names ``y`` is refused) -- which returns one replicated observation.  With it the posterior predictive calls
    (``posterior_predictive``, ``predictive_summary``, ``predictive_pit``, ``loo_pit``, ``loo_predictive(kind="y")``)
    take the likelihood; without it they refuse it, and nothing else changes.  A sampler body calls the vocabulary
    above plus, in sampler bodies only, ``uniform()`` ([0, 1)), ``uniform_open()`` ((0, 1)), ``normal()``,
    ``gamma(a)``, ``poisson(lam)`` and the helpers ``sqrt(x)``, ``floor(x)`` -- the exact samplers of the built-in
    families (``include/pgbart_ppc.h``).  A value is a function of the seed, the position of the draw, the global row
    and the inputs; a body may call a random function repeatedly (every call is a fresh, independent value; at most
    1024 calls of one kind per evaluation; calls of one kind are numbered in execution order, so two of them in ONE
    expression -- ``normal() - normal()`` -- may be numbered differently by the host and the device compiler: give
    them statements of their own where the bits matter).  A non-finite result is capped and counted (``n_capped``).  The body owns
    its domain: the params are only checked to be finite.  No param may carry a name of the random vocabulary when
    there is a sampler body.

    >>> CompiledLikelihood(zip_density, params={"pi": "pi"},
    ...                    sampler="return uniform() < pi ? 0.0 : poisson(exp(mu));")   # doctest: +SKIP
    """

    family = "compiled"

    def __init__(self, body: str, params=None, aux=None, n_outputs: int = 1, sampler=None):
        self.body = body
        self.sampler = sampler
        self.n_outputs = check_outputs(n_outputs)
        self.param_spec = dict(params or {})
        self.param_names = validate(body, list(self.param_spec), self.n_outputs)
        if sampler is not None:  # (before any compiler runs)
            validate(sampler, self.param_names, self.n_outputs, sampler=True)
        self.aux = None if aux is None else np.ascontiguousarray(aux, dtype=np.float64).ravel()
        if self.aux is not None and not np.all(np.isfinite(self.aux)):
            raise ValueError("aux must be finite")
        self._builds = {}
        self.compiled(64)  # (errors surface here, not at the first step)
        if sampler is not None:
            self.compiled_sampler()

    def compiled(self, max_particles: int = 64, linear: bool = False, pointwise: bool = False) -> CompiledLoglik:
        mp = 128 if int(max_particles) > 64 and not pointwise else 64
        k = (mp, False, True) if pointwise else (mp, bool(linear))
        if k not in self._builds:
            self._builds[k] = compile_loglik(self.body, self.param_names, mp, self.n_outputs, bool(linear),
                                             bool(pointwise))
        return self._builds[k]

    @property
    def has_sampler(self) -> bool:
        return self.sampler is not None

    def compiled_sampler(self) -> CompiledSampler:
        """The build of the sampler body: the code object of ``k_ppc_compiled``, the host library (``host_draw``) and
        the kernel's resources."""
        if self.sampler is None:
            raise CompileError("the likelihood has no sampler body (CompiledLikelihood(..., sampler=...))")
        if "sampler" not in self._builds:
            self._builds["sampler"] = compile_sampler(self.sampler, self.param_names, self.n_outputs)
        return self._builds["sampler"]

    def params(self, point=None):
        from .pgbart import _from_point

        return [_from_point(v, point) for v in self.param_spec.values()]

    def __getstate__(self):
        return {"body": self.body, "params": self.param_spec, "aux": self.aux, "n_outputs": self.n_outputs,
                "sampler": self.sampler}

    def __setstate__(self, d):
        self.__init__(d["body"], d["params"], d["aux"], d.get("n_outputs", 1), d.get("sampler"))
