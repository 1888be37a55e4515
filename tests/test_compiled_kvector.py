"""Family "compiled" with K-vector leaves, on the build box: the code objects of bodies of K = 2 .. 16 outputs (their
kernels, layout record and resources), the host builds of bodies that restate the built-in K-vector families against
the spec's own routines, the vocabulary's lgamma, and the refusals -- all before any launch."""
import ctypes as C
import importlib.util
import json
import os
import struct
import subprocess
import warnings

import numpy as np
import pytest

from _host_build import build
from pymc_bart_amd import CompiledLikelihood, _abi, compiled
from pymc_bart_amd.compiled import CompileError, compile_loglik
from pymc_bart_amd.pgbart import PGBART, BARTOp
from pymc_bart_amd.sampler import PyBartSettings, PySampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]

# pgb_loglik_meanscale_t, operation for operation (log(sd) = pgb_log_pos_t(sd) + 0.0 for sd in [1e-8, 1e300])
MEANSCALE = """double sd = mu[1] < 0.0 ? -mu[1] : mu[1];
if (!(sd >= 1e-8)) sd = 1e-8;
if (sd > 1.0e300) sd = 1.0e300;
double z = (y - mu[0]) / sd;
return -log(sd) - 0.5 * (z * z);"""
# pgb_loglik_cat_t, operation for operation; mu[c] picked by comparison (a run-time index would move mu to scratch);
# the upper bound 0 written so that a NaN stays a NaN for the sampler's clamp (fmin(NaN, 0) would give 0)
SOFTMAX = """double mx = mu[0];
for (int k = 1; k < K; ++k) if (mu[k] > mx) mx = mu[k];
double sum = 0.0;
for (int k = 0; k < K; ++k) sum += exp(mu[k] - mx);
int c = (int)y;
if (c < 0) c = 0;
if (c > K - 1) c = K - 1;
double muc = mu[0];
for (int k = 1; k < K; ++k) if (k == c) muc = mu[k];
double ll = (muc - mx) - log(sum);
if (!(sum >= 1.0)) ll = -2047.0;
return ll > 0.0 ? 0.0 : ll;"""


@pytest.fixture(autouse=True)
def _jit_cache(tmp_path_factory, monkeypatch):
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit"))


def _elf_symbol_bytes(code: bytes, name: str) -> bytes:
    """The bytes of a defined symbol of a 64-bit little-endian ELF (the code object's layout record)."""
    shoff, = struct.unpack_from("<Q", code, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", code, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", code, shoff + i * shentsize) for i in range(shnum)]
    for sh in secs:
        if sh[1] != 2:  # SHT_SYMTAB
            continue
        strtab = secs[sh[6]]
        for k in range(sh[5] // 24):
            st_name, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", code, sh[4] + k * 24)
            end = code.index(b"\0", strtab[4] + st_name)
            if code[strtab[4] + st_name:end].decode() == name:
                sec = secs[shndx]
                off = value - sec[3] + sec[4]
                return code[off:off + size]
    raise KeyError(name)


@pytest.mark.parametrize("K", [2, 3])
def test_a_kvector_code_object_exports_both_kernels_and_says_its_k(K, tmp_path):
    b = compile_loglik(SOFTMAX, [], n_outputs=K)
    p = tmp_path / "k.co"
    p.write_bytes(b.code)
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--symbols", str(p)], text=True)
    assert " k_loglik_compiled\n" in syms and " k_loglik_compiled_probe\n" in syms
    rec = _elf_symbol_bytes(b.code, "pgb_compiled_layout_record")
    magic, max_particles, n_params, n_outputs = struct.unpack_from("<iiii", rec, 0)
    assert (magic, max_particles, n_params, n_outputs) == (0x43424750, 64, 0, K)
    assert struct.unpack_from("<Q", rec, 56)[0] == compiled.headers_hash()
    one = compile_loglik("return -(y - mu) * (y - mu);", [])          # a one-output object says 1
    assert struct.unpack_from("<iiii", _elf_symbol_bytes(one.code, "pgb_compiled_layout_record"), 0)[3] == 1


def _guard_table_p128():
    spec = importlib.util.spec_from_file_location("occupancy_guard_here", os.path.join(ROOT, "tools", "occupancy_guard.py"))
    og = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(og)
    rows = og.table(os.path.join(ROOT, "pymc_bart_amd", "csrc", "libpgbart_hip_p128.so"))
    return {r["kernel"]: r for r in rows}


@pytest.mark.parametrize("body, K", [(MEANSCALE, 2), (SOFTMAX, 3), (SOFTMAX, 4), (SOFTMAX, 6), (SOFTMAX, 12),
                                     (SOFTMAX, 16)])
def test_restated_bodies_keep_the_builtin_instances_resources(body, K):
    inst = f"k_loglik<{K if K <= 4 else 0}, 3, false>"  # (the budget file's instance of that K)
    r = compile_loglik(body, [], n_outputs=K).resources
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["wgs_per_cu"] >= BUDGET[inst]["min_wgs_per_cu"], (r, BUDGET[inst])
    # the 128-particle build: against the same built-in instance of libpgbart_hip_p128.so (which misses some of the
    # budget file's 64-particle targets on its own)
    r128 = compile_loglik(body, [], max_particles=128, n_outputs=K).resources
    assert r128["scratch_bytes"] == 0 and r128["vgpr_spills"] == 0, r128
    assert r128["wgs_per_cu"] >= _guard_table_p128()[inst]["wgs_per_cu"], r128


_SPEC_HARNESS = r"""
#include <stdint.h>
#include <stddef.h>
#include "pgbart_spec.h"
void spec_rows(int which, int K, const double* y, const double* mu, int64_t n, double* out) {
  const pgb_lltabs tb = pgb_lltabs_default();
  double m[PGB_MAX_OUTPUTS];
  for (int64_t i = 0; i < n; ++i) {
    for (int k = 0; k < K; ++k) m[k] = mu[(size_t)k * (size_t)n + (size_t)i];
    out[i] = which == 0 ? pgb_loglik_meanscale_t(y[i], m, &tb) : pgb_loglik_cat_t(K, y[i], m, &tb);
  }
}
"""


def _spec_lib():
    return build("spec_rows", _SPEC_HARNESS,
                 {"spec_rows": (None, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p])}).spec_rows


def _edge_grid(K, n, seed, classes=False):
    rng = np.random.default_rng(seed)
    # (extremes within pgb_exp_t's domain, |x| < 4.6e7: the spec's table exponential has no clamp beyond it)
    edges = np.array([0.0, -0.0, 1e-300, -1e-300, 1e-9, -1e-9, 1.0, -1.0, 36.5, -36.5, 700.0, -700.0, 745.0, -745.0,
                      1e5, -1e5, 2e7, -2e7, np.inf, -np.inf, np.nan])
    mu = np.where(rng.random((K, n)) < 0.3, rng.choice(edges, (K, n)), rng.normal(0, 3, (K, n)) * 10.0 ** rng.integers(-3, 3, (K, n)))
    if classes:
        y = rng.integers(-1, K + 1, n).astype(float)                  # (out-of-range classes are clamped)
        odd = rng.random(n) < 0.05
        y[odd] = rng.choice([-3.0, -0.5, 0.5, K - 0.5, K + 2.0], int(odd.sum()))
    else:
        y = np.where(rng.random(n) < 0.2, rng.choice(edges, n), rng.normal(0, 5, n))
    return np.ascontiguousarray(y), np.ascontiguousarray(mu)


@pytest.mark.parametrize("which, K", [(0, 2), (1, 2), (1, 3), (1, 4), (1, 6), (1, 12), (1, 16)])
def test_host_builds_of_the_restated_bodies_equal_the_spec_bit_for_bit(which, K):
    spec = _spec_lib()
    y, mu = _edge_grid(K, 40_000, seed=10 * which + K, classes=which == 1)
    want = np.empty(y.size)
    spec(which, K, y.ctypes.data, mu.ctypes.data, y.size, want.ctypes.data)
    got = compile_loglik(MEANSCALE if which == 0 else SOFTMAX, [], n_outputs=K).host_eval(y, mu)
    assert np.all(np.isfinite(want))
    bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


def _host1(body):
    """A one-output body's host build, unclamped, on y (mu = 0)."""
    b = compile_loglik(body, [])
    fn = b.host_function()
    ctx = compiled.CompiledContext()

    def run(x):
        x = np.ascontiguousarray(x, np.float64)
        rows = np.arange(x.size, dtype=np.int64)
        mu = np.zeros_like(x)
        out = np.empty_like(x)
        assert fn(C.cast(C.pointer(ctx), C.c_void_p), rows.ctypes.data_as(C.POINTER(C.c_int64)),
                  x.ctypes.data_as(C.POINTER(C.c_double)), mu.ctypes.data_as(C.POINTER(C.c_double)), x.size,
                  out.ctypes.data_as(C.POINTER(C.c_double))) == 0
        return out

    return run


def test_lgamma_meets_its_accuracy_bound_and_domain():
    from scipy.special import gammaln

    lg = _host1("return lgamma(y);")
    rng = np.random.default_rng(3)
    x = np.concatenate([np.logspace(-6, 12, 200_001), rng.uniform(1e-6, 30.0, 100_000),
                        np.arange(1.0, 200.0), np.arange(0.5, 200.0), 1.0 + np.linspace(-1e-3, 1e-3, 2001),
                        2.0 + np.linspace(-1e-3, 1e-3, 2001), np.nextafter(10.0, [0.0, 20.0]), [1e-6, 1e12]])
    got, want = lg(x), gammaln(x)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 1e-13, (x[err.argmax()], got[err.argmax()], want[err.argmax()], err.max())
    odd = lg(np.array([0.0, -0.0, -1.0, -2.5, -np.inf, np.nan, np.inf]))
    assert np.all(np.isnan(odd[:6])) and odd[6] == np.inf
    assert compiled.uses_tables("return lgamma(y);")                  # (the log table is staged in LDS)
    for f in ("sqrt", "pow"):
        with pytest.raises(CompileError, match=f"'{f}' is not in the likelihood vocabulary"):
            compile_loglik(f"return {f}(y, 2.0);", [])


@pytest.mark.parametrize("kw, exc, msg", [
    (dict(body="return -mu[0] * mu[1] * K0;", params={"K": 1.0}, n_outputs=2), ValueError, "'K' is reserved"),
    (dict(body="int K = 3; return mu[0];", n_outputs=2), ValueError, "'K' is reserved"),
    (dict(body="return -(y - mu[0]) * (y - mu[2]);", n_outputs=2), ValueError, r"mu\[2\] is out of range"),
    (dict(body="double s = exp(mu[1]);\nreturn -(y - mu) / s;", n_outputs=2), CompileError,
     r"line 2: mu holds K = 2 predictors, it is not a scalar(.|\n)*return -\(y - mu\) / s;"),
    (dict(body="if (mu) return 0.0;\nreturn mu[1];", n_outputs=3), CompileError, "line 1: mu holds K = 3"),
    (dict(body="return mu;", n_outputs=0), ValueError, r"n_outputs must be an integer in \[1, 16\]"),
    (dict(body="return mu[0];", n_outputs=17), ValueError, r"n_outputs must be an integer in \[1, 16\]"),
])
def test_refusals_come_before_any_compiler_and_name_the_problem(kw, exc, msg, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("refused before any compiler runs")

    monkeypatch.setattr(subprocess, "run", boom)
    body = kw.pop("body")
    with pytest.raises(exc, match=msg):
        CompiledLikelihood(body, **kw)


def test_a_kvector_compiled_sampler_is_refused_on_a_cpu_backend(oracle):
    rng = np.random.default_rng(0)
    X, Y = rng.normal(size=(200, 3)), rng.gamma(2.0, 1.0, 200)
    st = PyBartSettings.from_data(X, Y, m=5, num_particles=6, n_outputs=2, family="compiled")
    with pytest.raises(_abi.PGBError, match="HIP backend only.*single output"):
        PySampler(st, X, Y, np.zeros(3, np.int32), np.ones(3), backend=oracle)
    lik = CompiledLikelihood(MEANSCALE, n_outputs=2)
    with pytest.raises(_abi.PGBError, match="HIP backend only"):
        PGBART([BARTOp(X, Y, m=5)], num_particles=6, likelihood=lik, random_seed=1, backend=oracle)
    with pytest.raises(CompileError, match="no callback"):
        lik.compiled(64).host_function()


def test_the_cache_key_covers_k_and_a_runtime_index_warns_exactly_with_scratch():
    k2, k3 = (compiled.cache_key(SOFTMAX, [], 64, K) for K in (2, 3))
    assert k2 != k3 and compiled.cache_key(SOFTMAX, []) == compiled.cache_key(SOFTMAX, [], 64, 1) != k2
    assert compile_loglik(SOFTMAX, [], n_outputs=2).key != compile_loglik(SOFTMAX, [], n_outputs=3).key
    for K in (2, 4, 16):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            b = compile_loglik("int c = (int)y;\nif (c < 0) c = 0;\nif (c > K - 1) c = K - 1;\nreturn mu[c] - mu[0];",
                               [], n_outputs=K)
        warned = [x for x in w if "scratch memory" in str(x.message)]
        assert bool(warned) == (b.resources["scratch_bytes"] > 0), (K, b.resources)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        compile_loglik(SOFTMAX, [], n_outputs=4)                       # (the compare-and-pick form: no warning)


def test_a_kvector_likelihood_pickles_with_its_k():
    import pickle

    lik = CompiledLikelihood(MEANSCALE, n_outputs=2)
    twin = pickle.loads(pickle.dumps(lik))
    assert twin.n_outputs == 2 and twin.body == MEANSCALE
    assert CompiledLikelihood("return -(y - mu) * (y - mu);").n_outputs == 1
