"""Family "compiled" on the build box: the body's two builds (a gfx950 code object, a host function), the vocabulary
and its refusals, the cache, and the CPU path -- the oracle running the host build as family "callback" -- which
must reproduce the built-in family the body spells out, bit for bit."""
import ctypes as C
import json
import os
import pickle
import subprocess

import numpy as np
import pytest

from _cases import digest, make_case, run_case
from pymc_bart_amd import CompiledLikelihood, compiled
from pymc_bart_amd.compiled import CompileError, compile_loglik
from pymc_bart_amd.pgbart import PGBART, BARTOp
from pymc_bart_amd.sampler import PySampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_runs.json")))
BUDGET = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
CHECK_LOSS = "double u = (y - mu) / b;  return -(u * (u < 0.0 ? q - 1.0 : q));"
# pgb_loglik1q's POISSON_LOG, spelled out with the vocabulary
POISSON = ("double yy = y > 0.0 ? y : 0.0;\n"
           "double em = exp(mu);\n"
           "double sat = yy > 0.0 ? yy * log(yy) - yy : 0.0;\n"
           "return (yy * mu - em) - sat;")


@pytest.fixture(autouse=True)
def _jit_cache(tmp_path_factory, monkeypatch):
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit"))


def _kernel_symbols(code: bytes, tmp_path) -> str:
    p = tmp_path / "k.co"
    p.write_bytes(code)
    return subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--symbols", str(p)], text=True)


def test_device_flags_are_the_library_flags():
    import importlib.util

    # (by path: another test may have imported a copy of __graft_entry__ from a temporary tree)
    spec = importlib.util.spec_from_file_location("graft_entry_here", os.path.join(ROOT, "__graft_entry__.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)

    assert compiled.DEVICE_FLAGS == [f for f in g.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    assert "-ffp-contract=off" in compiled.HOST_FLAGS and "-ffp-contract=off" in compiled.DEVICE_FLAGS


def test_check_loss_code_object_exports_the_kernel_and_the_record_and_keeps_its_occupancy(tmp_path):
    b = compile_loglik(CHECK_LOSS, ["b", "q"])
    assert b.code[:4] == b"\x7fELF"
    syms = _kernel_symbols(b.code, tmp_path)
    assert " k_loglik_compiled" in syms and "pgb_compiled_layout_record" in syms
    r = b.resources
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0
    assert r["wgs_per_cu"] >= BUDGET["k_loglik<1, 7, false>"]["min_wgs_per_cu"]
    p = compile_loglik(POISSON, [])
    assert p.resources["scratch_bytes"] == 0 and p.resources["vgpr_spills"] == 0
    assert p.resources["wgs_per_cu"] >= BUDGET["k_loglik<1, 5, false>"]["min_wgs_per_cu"]


def _host_eval(build, y, mu, aux=None, params=()):
    fn = build.host_function()
    ctx = compiled.CompiledContext()
    keep = None
    if aux is not None:
        keep = np.ascontiguousarray(aux, np.float64)
        ctx.aux = keep.ctypes.data
    for i, v in enumerate(params):
        ctx.params[i] = v
    n = y.size
    rows = np.arange(n, dtype=np.int64)
    out = np.empty(n)
    rc = fn(C.cast(C.pointer(ctx), C.c_void_p), rows.ctypes.data_as(C.POINTER(C.c_int64)),
            y.ctypes.data_as(C.POINTER(C.c_double)), mu.ctypes.data_as(C.POINTER(C.c_double)), n,
            out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    return out


def test_host_build_of_an_ieee_body_equals_numpy_bit_for_bit():
    rng = np.random.default_rng(0)
    n = 100_000
    y, mu, aux = rng.normal(0, 3, n), rng.normal(0, 3, n), rng.uniform(0, 2, n)
    body = ("double u = (y - mu) / b;\n"
            "double w = aux > 1.0 ? q : 1.0 - q;\n"
            "if (u < 0.0) { u = -u * w; } else { u = u * (w + 0.5); }\n"
            "return -(u * u) / (2.0 + fabs(mu)) + fmin(aux, 1.5) - fmax(y, -1.0);")
    out = _host_eval(compile_loglik(body, ["b", "q"]), y, mu, aux, (0.7, 0.3))
    u = (y - mu) / 0.7
    w = np.where(aux > 1.0, 0.3, 1.0 - 0.3)
    u = np.where(u < 0.0, -u * w, u * (w + 0.5))
    want = -(u * u) / (2.0 + np.abs(mu)) + np.where(aux < 1.5, aux, 1.5) - np.where(y > -1.0, y, -1.0)
    assert np.array_equal(out.view(np.int64), want.view(np.int64))


def test_host_exp_and_log_are_the_spec_tables_not_libm(oracle):
    """The Poisson-log arithmetic of pgb_loglik1q spelled out with the vocabulary equals the oracle's own
    pgbo_loglikq wherever that value is <= 0 (its clamp): exp / log are the spec's table functions."""
    rng = np.random.default_rng(1)
    n = 100_000
    y = rng.poisson(3.0, n).astype(float)
    mu = rng.normal(1.0, 1.5, n)
    got = _host_eval(compile_loglik(POISSON, []), y, mu)
    lib = oracle.lib.lib
    f = lib.pgbo_loglikq
    f.restype, f.argtypes = None, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p]
    want = np.empty(n)
    f(5, y.ctypes.data, mu.ctypes.data, n, 0.0, 1.0, want.ctypes.data)
    keep = (got <= 0.0) & (got > -2047.0)
    assert keep.mean() > 0.99
    assert np.array_equal(got[keep].view(np.int64), want[keep].view(np.int64))
    libm = y * mu - np.exp(mu) - np.where(y > 0, y * np.log(np.where(y > 0, y, 1.0)) - y, 0.0)
    assert not np.array_equal(got[keep], libm[keep])                 # (libm would differ somewhere)


def _compiled_case(lik):
    c = dict(make_case("quantile_asymlaplace"))
    c["family"] = "compiled"
    orig = PySampler.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        if self.settings.family == "compiled":
            self.set_compiled_likelihood(lik)

    return c, orig, init


def test_oracle_chain_with_the_compiled_check_loss_reproduces_the_builtin_fingerprint(oracle):
    lik = CompiledLikelihood(CHECK_LOSS, params={"b": 0.25, "q": 0.9})
    c, orig, init = _compiled_case(lik)
    PySampler.__init__ = init
    try:
        res = run_case(c, oracle)
    finally:
        PySampler.__init__ = orig
    assert res["sampler"].backend.lib.backend_name != "hip-gfx950"
    assert digest(res) == GOLD["quantile_asymlaplace"]


@pytest.mark.parametrize("body, params, msg, exc", [
    ("#include <math.h>\nreturn 0.0;", [], "preprocessor", ValueError),
    ("  #define X 1\nreturn X;", [], "preprocessor", ValueError),
    ("%:define X 1\nreturn 0.0;", [], "preprocessor", ValueError),
    ('asm("s_nop 0"); return 0.0;', [], "string literal", ValueError),
    ("asm volatile (0); return 0.0;", [], "assembly", ValueError),
    ("__asm__ (0); return 0.0;", [], "assembly", ValueError),
    ("return __builtin_sqrt(y);", [], "builtins", ValueError),
    ("return __x;", [], "'__'", ValueError),
    ("return y;", ["mu"], "clashes", ValueError),
    ("return y;", ["log"], "vocabulary", ValueError),
    ("return y;", ["b", "b"], "duplicate", ValueError),
    ("return y;", [f"p{i}" for i in range(9)], "at most 8", ValueError),
    ("return y; } double g(double x) { return x;", [], "unbalanced", ValueError),
    ("static double s = 0.0; return s;", [], "'static'", ValueError),
    ("return pow(y, 2.0);", [], "'pow' is not in the likelihood vocabulary", CompileError),
])
def test_refusals_name_the_problem(body, params, msg, exc):
    with pytest.raises(exc, match=msg):
        compile_loglik(body, params)


def test_a_call_outside_the_vocabulary_lists_the_vocabulary():
    with pytest.raises(CompileError) as e:
        CompiledLikelihood("double z = y - mu;\nreturn -sqrt(z * z);")
    text = str(e.value)
    assert "return -sqrt(z * z);" in text and "log_ndtr" in text and "softplus" in text


def test_a_syntax_error_is_a_compile_error_quoting_the_users_line():
    with pytest.raises(CompileError) as e:
        compile_loglik("double z = (y - mu) / s;\nreturn -0.5 * z * z +;", ["s"])
    assert "return -0.5 * z * z +;" in str(e.value) and "line 2" in str(e.value)


def test_the_cache_serves_a_second_compile_without_a_subprocess(monkeypatch, tmp_path):
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path / "cache"))
    a = compile_loglik(CHECK_LOSS, ["b", "q"])
    assert not a.cached and a.compile_seconds > 0
    files = sorted(os.listdir(tmp_path / "cache"))
    assert files == sorted(a.key + ext for ext in (".co", ".json", ".so"))  # (no temporary left behind)

    def boom(*a, **k):
        raise AssertionError("a cache hit runs no subprocess")

    monkeypatch.setattr(subprocess, "run", boom)
    monkeypatch.setattr(subprocess, "check_output", boom)
    monkeypatch.setattr(subprocess, "Popen", boom)
    b = compile_loglik(CHECK_LOSS, ["b", "q"])
    assert b.cached and b.key == a.key and b.code == a.code and b.resources == a.resources
    monkeypatch.undo()
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path / "cache"))
    keys = {a.key, compiled.cache_key(CHECK_LOSS + " ", ["b", "q"]), compiled.cache_key(CHECK_LOSS, ["bb", "q"]),
            compiled.cache_key(CHECK_LOSS, ["b", "q"], 128)}
    assert len(keys) == 4


def test_cache_entries_are_written_atomically(monkeypatch, tmp_path):
    """Every file goes to a temporary name in the cache directory and is renamed into place."""
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path))
    seen = []
    real = os.replace

    def spy(src, dst):
        seen.append((os.path.basename(src), os.path.basename(dst)))
        assert os.path.dirname(src) == os.path.dirname(dst) == str(tmp_path)
        return real(src, dst)

    monkeypatch.setattr(os, "replace", spy)
    b = compile_loglik(CHECK_LOSS, ["b", "q"])
    assert [d for _, d in seen] == [b.key + ".co", b.key + ".so", b.key + ".json"]  # (the record last)
    assert all(s.startswith(".tmp_") for s, _ in seen)


def test_step_method_with_a_compiled_likelihood_pickles_and_continues_bit_for_bit(oracle, monkeypatch):
    import pymc_bart_amd.sampler as sm

    monkeypatch.setattr(sm, "_DEFAULT_BACKEND", oracle)
    rng = np.random.default_rng(2)
    X = rng.uniform(-1, 1, size=(300, 2))
    f = np.sin(3 * X[:, 0])
    Y = f + rng.normal(0, 0.5, 300)
    w = rng.uniform(0.5, 2.0, 300)
    lik = CompiledLikelihood("double z = (y - mu) / s;  return -0.5 * aux * z * z;", params={"s": "sigma"}, aux=w)
    step = PGBART([BARTOp(X, Y, m=10)], num_particles=8, likelihood=lik, random_seed=4, backend=oracle)
    draws = []
    for it in range(80):
        if it == 40:
            step.stop_tuning()
        mu, _ = step.astep(None, {"sigma": 0.5})
        if it >= 40:
            draws.append(mu)
    assert np.corrcoef(np.mean(draws, axis=0), f)[0, 1] > 0.8
    twin = pickle.loads(pickle.dumps(step))
    assert twin.likelihood.body == lik.body and np.array_equal(twin.likelihood.aux, w)
    for _ in range(3):
        a, _ = step.astep(None, {"sigma": 0.5})
        b, _ = twin.astep(None, {"sigma": 0.5})
        assert np.array_equal(a, b)


def _elf_symbol_bytes(code: bytes, name: str) -> bytes:
    """The bytes of a defined symbol of a 64-bit little-endian ELF (the code object's layout record)."""
    import struct

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


def test_a_code_object_for_128_particles_says_so_in_its_layout_record():
    import struct

    for mp in (64, 128):
        b = compile_loglik(CHECK_LOSS, ["b", "q"], max_particles=mp)
        rec = _elf_symbol_bytes(b.code, "pgb_compiled_layout_record")
        magic, max_particles, n_params, _ = struct.unpack_from("<iiii", rec, 0)
        assert magic == 0x43424750 and max_particles == mp and n_params == 2
        assert struct.unpack_from("<Q", rec, 56)[0] == compiled.headers_hash()
