"""Sampler bodies of compiled likelihoods, on the CPU: the validation, the host builds against the host build of the
built-in families (``tests/_ppc_host.py``) bit for bit, the addressing of repeated calls, the caps, and the Python layer
of the five public calls on the recording backend."""
import ctypes as C
import math
import pickle

import numpy as np
import pytest

import _ppc_compiled_cases as cases
import _ppc_host as host
import pymc_bart_amd as pb
from _recording_backend import Recorder
from pymc_bart_amd import CompiledLikelihood, _abi
from pymc_bart_amd.compiled import CompileError, compile_sampler
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays
from test_ppc_gpu import CASES, ROW0, inputs

DENSITY = "double z = (y - mu) / s; return -0.5 * z * z - log(s);"
CAPPED, EXHAUSTED = 0, 1


# ------------------------------------------------------------------ 1. validation
def test_a_sampler_body_has_no_y():
    with pytest.raises(ValueError, match="line 2: a sampler body has no y"):
        CompiledLikelihood(DENSITY, {"s": 1.0}, sampler="double t = mu;\nreturn y + t;")
    CompiledLikelihood(DENSITY, {"s": 1.0}, sampler="double my = mu; /* y */ return my + s * normal();  // y")


@pytest.mark.parametrize("sampler, exc, msg", [
    ("return mu + pow(s, 2.0);", CompileError, "'pow' is not in the sampler vocabulary"),
    ("return mu + rand();", CompileError, "'rand' is not in the sampler vocabulary"),
    ("#define A 1\nreturn mu;", ValueError, "preprocessor lines are not allowed in a sampler body"),
    ("asm(\"\"); return mu;", ValueError, "string literal|inline assembly"),
    ("__asm__ volatile(); return mu;", ValueError, "inline assembly"),
    ("return __builtin_sqrt(mu);", ValueError, "compiler builtins"),
    ("double __x = mu; return __x;", ValueError, "starting with '__'"),
    ("return pgb_u01(1, 2);", ValueError, "reserved for the prelude"),
    ("", ValueError, "non-empty string"),
])
def test_what_a_sampler_body_may_not_contain(sampler, exc, msg):
    with pytest.raises(exc, match=msg):
        CompiledLikelihood(DENSITY, {"s": 1.0}, sampler=sampler)


def test_a_density_body_has_no_random_vocabulary():
    for fn in ("normal()", "uniform()", "gamma(2.0)", "poisson(2.0)", "sqrt(2.0)"):
        with pytest.raises(CompileError, match="not in the likelihood vocabulary"):
            CompiledLikelihood(f"return {fn} - y + mu;")
        with pytest.raises(CompileError, match="not in the likelihood vocabulary"):
            CompiledLikelihood(f"return {fn} - y + mu;", sampler="return mu;")


def test_random_names_are_reserved_only_with_a_sampler_body():
    body = "double z = (y - mu) / normal; return -0.5 * z * z - gamma;"
    lik = CompiledLikelihood(body, {"normal": 2.0, "gamma": 0.5})           # density only: as before
    assert lik.param_names == ("normal", "gamma") and not lik.has_sampler
    with pytest.raises(CompileError, match="no sampler body"):
        lik.compiled_sampler()
    for name in ("normal", "gamma", "uniform", "uniform_open", "poisson", "sqrt", "floor"):
        with pytest.raises(ValueError, match=f"param name '{name}' clashes with the vocabulary"):
            CompiledLikelihood(f"return -(y - mu) * (y - mu) * {name};", {name: 1.0}, sampler="return mu;")


def test_a_compiler_error_names_the_line_of_the_sampler_body():
    with pytest.raises(CompileError, match=r"the sampler body does not compile \(host\):\nline 3:.*\n    return mu \+ t \+ nope;"):
        CompiledLikelihood(DENSITY, {"s": 1.0}, sampler="double t = s * normal();\n\nreturn mu + t + nope;")


# ------------------------------------------------------------------ 2. restated families
@pytest.mark.parametrize("case", list(cases.RESTATED))
def test_a_restated_family_gives_the_bits_of_the_built_in_one(case):
    build = cases.restated(case)
    for j, (D, n) in enumerate([(33, 65), (7, 257)]):
        family, mu, params, off = inputs(case, D, n, seed=100 * D + n)
        for row0 in ROW0:
            y = np.round(mu[0, 0])
            want, wpit, wflags = host.fill(family, mu, params, row0=row0, seed=5 + j, y=y)
            got, pit, flags = build.host_draw(mu, params, seed=5 + j, row0=row0, y=y)
            assert np.array_equal(cases.bits(got), cases.bits(want)), (case, D, n, row0)
            assert np.array_equal(pit, wpit) and flags == wflags, (case, D, n, row0)
    if case in ("poisson_log", "negbin_log"):   # both Poisson samplers were reached
        rate = np.exp(mu[:, 0])
        assert (rate < host.poisson_switch()).any() and (rate > 2 * host.poisson_switch()).any()


# ------------------------------------------------------------------ 3. repeated calls
def test_repeated_calls_are_independent():
    build = cases.build(cases.DIFFERENCE)
    mu = np.zeros((64, 1, 1000))
    v, _, flags = build.host_draw(mu, seed=11)
    assert flags == (0, 0) and not np.any(v == 0.0)
    N = v.size
    se = 2.0 * math.sqrt(2.0 / (N - 1))                       # of the sample variance of N normals of variance 2
    assert abs(v.var(ddof=1) - 2.0) < 5 * se, (v.var(ddof=1), se)
    again, _, _ = build.host_draw(mu, seed=11)
    assert np.array_equal(cases.bits(again), cases.bits(v))
    other, _, _ = build.host_draw(mu, seed=12)
    assert not np.array_equal(cases.bits(other), cases.bits(v))


def test_the_call_cap():
    build = cases.build(cases.LOOP1025)
    D, n = 3, 9
    v, _, flags = build.host_draw(np.zeros((D, 1, n)), seed=1)
    assert flags == (0, D * n) and np.all(np.isfinite(v))
    # 1024 calls: the last one still draws
    ok = compile_sampler(cases.LOOP1025[0].replace("1025", "1024"), ())
    w, _, flags = ok.host_draw(np.zeros((D, 1, n)), seed=1)
    assert flags == (0, 0) and np.array_equal(cases.bits(w), cases.bits(v))   # (the 1025th call adds its fixed 0.0)


# ------------------------------------------------------------------ 4. a body no family has
def test_the_zero_inflated_poisson_has_its_pmf():
    build = cases.build(cases.ZIP)
    D, n, mu, pi = 64, 1000, 0.9, 0.3
    v, _, flags = build.host_draw(np.full((D, 1, n), mu), np.full((D, 1), pi), seed=2024)
    assert flags == (0, 0)
    lam = float(np.exp(mu))
    N = D * n
    for k in range(9):
        p = (1.0 - pi) * math.exp(-lam) * lam ** k / math.factorial(k) + (pi if k == 0 else 0.0)
        freq = float((v == k).sum()) / N
        assert abs(freq - p) < 5 * math.sqrt(p * (1 - p) / N), (k, freq, p)
    assert np.all(v == np.floor(v)) and v.min() == 0.0


# ------------------------------------------------------------------ 5. caps
def test_an_overflowing_result_is_capped_and_counted():
    build = cases.build(cases.OVERFLOW)
    D, n = 4, 11
    aux = (np.arange(n) % 2).astype(np.float64)
    v, _, flags = build.host_draw(np.ones((D, 1, n)), aux=aux, seed=1)
    assert flags == (D * n, 0)
    assert np.all(v[:, aux < 0.5] == 1.7976931348623157e308) and np.all(v[:, aux > 0.5] == -1.7976931348623157e308)


# ------------------------------------------------------------------ 6. the Python layer
N_ROWS, P, M_TREES, DRAWS = 200, 3, 2, 60


class Rec(Recorder):
    """The recording backend with ``pgb_ppc_draw_compiled``: each call is kept with what its struct points to."""

    def __init__(self):
        super().__init__()
        self.compiled_calls = []
        self.lib.ppc_compiled_entry_point = lambda: self._draw_compiled

    def _draw_compiled(self, md, D, K, nb, ld, row0, lik, seed, *rest):
        code = lik._obj
        assert isinstance(code, _abi.PpcCode) and code.code_bytes > 64
        aux = None if not code.aux_dev else np.array((C.c_double * nb).from_address(code.aux_dev))
        par = np.array((C.c_double * (D * code.n_params)).from_address(code.params_host)).reshape(D, code.n_params)
        elf = bytes((C.c_char * 4).from_address(code.code_object))
        self.compiled_calls.append({"D": D, "K": K, "nb": nb, "ld": ld, "row0": row0, "seed": seed, "aux": aux, "params": par,
                                    "elf": elf, "offset": code.offset_dev})
        self.trace.append("pgb_ppc_draw_compiled")
        return 0


def _fit(rec):
    pool = TreeArrays.empty(M_TREES, M_TREES, 1)
    pool.tree_id[:] = np.arange(M_TREES)
    pool.node_off[:] = np.arange(M_TREES + 1)
    pool.var[:] = -1
    pool.count[:] = 10
    return PosteriorSampler(pool, np.tile(np.arange(M_TREES, dtype=np.int32), (DRAWS, 1)), M_TREES, 1, backend=rec)


def _calls(lik, points=None):
    """name -> call(sampler, X, y) of the five public calls."""
    kw = {"points": points, "random_seed": 9}
    return {"posterior_predictive": lambda s, X, y: pb.posterior_predictive(s, X, lik, **kw),
            "predictive_summary": lambda s, X, y: pb.predictive_summary(s, X, lik, **kw),
            "predictive_pit": lambda s, X, y: pb.predictive_pit(s, X, y, lik, **kw),
            "loo_pit": lambda s, X, y: pb.loo_pit(s, X, y, lik, **kw),
            "loo_predictive_y": lambda s, X, y: pb.loo_predictive(s, X, y, lik, kind="y", **kw)}


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(5)
    return rng.normal(size=(N_ROWS, P)), rng.normal(size=N_ROWS)


def test_without_a_sampler_body_the_five_calls_refuse_in_todays_words(data):
    X, y = data
    lik = CompiledLikelihood(cases.CENSORED_DENSITY, {"s": "sigma"}, aux=np.zeros(N_ROWS))
    rec = Rec()
    for name, call in _calls(lik, {"sigma": 1.0}).items():
        with pytest.raises(ValueError, match="the compiled family has a log density only, no sampler"):
            call(_fit(rec), X, y)
    assert rec.trace == []


def test_argument_errors_come_before_a_backend_is_touched(data):
    X, y = data
    rec = Rec()
    short = CompiledLikelihood(cases.CENSORED_DENSITY, {"s": "sigma"}, aux=np.zeros(N_ROWS - 1), sampler=cases.LATENT)
    for name, call in _calls(short, {"sigma": 1.0}).items():
        with pytest.raises(ValueError, match=f"aux must hold one value per row \\({N_ROWS}\\), got {N_ROWS - 1}"):
            call(_fit(rec), X, y)
    lik = CompiledLikelihood(cases.CENSORED_DENSITY, {"s": "sigma"}, aux=np.zeros(N_ROWS), sampler=cases.LATENT)
    sigma = np.ones(DRAWS)
    sigma[2] = np.nan
    for name, call in _calls(lik, {"sigma": sigma}).items():
        with pytest.raises(ValueError, match="likelihood params must be finite"):
            call(_fit(rec), X, y)
    two = CompiledLikelihood("return -(y - mu[0]) * (y - mu[0]) - mu[1];", n_outputs=2, sampler="return mu[0] + normal();")
    with pytest.raises(ValueError, match="the likelihood has n_outputs = 2, the sampler's trees n_outputs = 1"):
        pb.posterior_predictive(_fit(rec), X, two)
    assert rec.trace == []
    # a negative or zero param is the body's business: no domain check
    pb.posterior_predictive(_fit(rec), X, lik, points={"sigma": -np.ones(DRAWS)})
    assert len(rec.compiled_calls) == 1


@pytest.mark.parametrize("name", ["posterior_predictive", "predictive_summary", "predictive_pit", "loo_pit", "loo_predictive_y"])
def test_each_block_carries_its_slice_of_aux_its_row0_and_the_params(name, data, monkeypatch):
    X, y = data
    aux = np.arange(N_ROWS, dtype=np.float64)
    sigma = 0.5 + np.arange(DRAWS)
    lik = CompiledLikelihood(cases.CENSORED_DENSITY, {"s": "sigma"}, aux=aux, sampler=cases.LATENT)
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(1 << 16))
    rec = Rec()
    _calls(lik, {"sigma": sigma})[name](_fit(rec), X, y)
    calls = rec.compiled_calls
    assert len(calls) >= 2 and not any(line.startswith("pgb_ppc_draw ") for line in rec.trace)
    r0 = 0
    for c in calls:
        assert c["row0"] == r0 and c["ld"] == c["nb"] and (c["D"], c["K"], c["seed"]) == (DRAWS, 1, 9)
        assert np.array_equal(c["aux"], aux[r0:r0 + c["nb"]])
        assert np.array_equal(c["params"], sigma[:, None]) and c["elf"] == b"\x7fELF" and not c["offset"]
        r0 += c["nb"]
    assert r0 == N_ROWS
    # per_row counts the aux column: with it the blocks are no longer than without
    none = CompiledLikelihood(cases.CENSORED_DENSITY, {"s": "sigma"}, sampler=cases.LATENT)
    rec2 = Rec()
    _calls(none, {"sigma": sigma})[name](_fit(rec2), X, y)
    assert all(c["aux"] is None for c in rec2.compiled_calls) and len(rec2.compiled_calls) <= len(calls)


def test_the_pickle_round_trip_carries_the_sampler():
    lik = CompiledLikelihood(cases.CENSORED_DENSITY, {"s": "sigma"}, aux=np.arange(4.0), sampler=cases.LATENT)
    back = pickle.loads(pickle.dumps(lik))
    assert back.sampler == cases.LATENT and back.has_sampler and back.body == lik.body
    assert back.compiled_sampler().key == lik.compiled_sampler().key and np.array_equal(back.aux, lik.aux)
    assert lik.compiled_sampler().key != lik.compiled(pointwise=True).key != lik.compiled().key
    state = lik.__getstate__()
    del state["sampler"]                                       # a pickle from before sampler bodies
    old = CompiledLikelihood.__new__(CompiledLikelihood)
    old.__setstate__(state)
    assert old.sampler is None and not old.has_sampler and old.compiled().key == lik.compiled().key


def test_the_abi_names_the_missing_symbol():
    from _oracle import oracle_backend

    with pytest.raises(NotImplementedError, match="pgb_ppc_draw_compiled"):
        oracle_backend().lib.ppc_compiled_entry_point()


def test_the_timing_tool_imports_and_answers_help_without_a_device(capsys, monkeypatch):
    import importlib
    import os
    import sys

    monkeypatch.setattr(sys, "path", [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")]
                        + list(sys.path))
    with pytest.raises(SystemExit) as e:
        importlib.import_module("ppc_timing_compiled").main(["--help"])
    assert e.value.code == 0 and capsys.readouterr().out.startswith("usage:")
