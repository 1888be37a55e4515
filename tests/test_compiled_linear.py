"""Family "compiled" with linear / mix leaves, on the build box: the linear-leaf code objects of one-output and
K-output bodies (their kernels, layout record, cache keys and resources), the refusal of a CPU backend, pickling --
all before any launch."""
import importlib.util
import json
import os
import pickle
import struct
import subprocess

import numpy as np
import pytest

from _restated_bodies import CHECK_LOSS, MEANSCALE, POISSON, PROBIT, SOFTMAX
from pymc_bart_amd import CompiledLikelihood, _abi, compiled
from pymc_bart_amd.compiled import compile_loglik
from pymc_bart_amd.pgbart import PGBART, BARTOp
from pymc_bart_amd.sampler import PyBartSettings, PySampler
from test_compiled_kvector import _elf_symbol_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]


@pytest.fixture(autouse=True)
def _jit_cache(tmp_path_factory, monkeypatch):
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit"))


def _record(code):
    rec = _elf_symbol_bytes(code, "pgb_compiled_layout_record")
    assert len(rec) == 72
    return rec


@pytest.mark.parametrize("body, names, K", [(CHECK_LOSS, ["b", "q"], 1), (MEANSCALE, [], 2), (SOFTMAX, [], 3),
                                            (SOFTMAX, [], 6), (SOFTMAX, [], 16)],
                         ids=["check_loss", "meanscale_k2", "softmax_k3", "softmax_k6", "softmax_k16"])
@pytest.mark.parametrize("mp", [64, 128])
def test_a_linear_code_object_exports_both_kernels_and_says_linear_leaves(body, names, K, mp, tmp_path):
    lin = compile_loglik(body, names, mp, K, linear=True)
    con = compile_loglik(body, names, mp, K)
    assert lin.linear is True and con.linear is False and (lin.n_outputs, lin.max_particles) == (K, mp)
    p = tmp_path / "k.co"
    p.write_bytes(lin.code)
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--symbols", str(p)], text=True)
    assert " k_loglik_compiled\n" in syms and " k_loglik_compiled_probe\n" in syms
    rl, rc = _record(lin.code), _record(con.code)
    assert struct.unpack_from("<iiii", rl, 0) == (0x43424750, mp, len(names), K) == struct.unpack_from("<iiii", rc, 0)
    assert struct.unpack_from("<Q", rl, 56)[0] == compiled.headers_hash() == struct.unpack_from("<Q", rc, 56)[0]
    assert struct.unpack_from("<ii", rl, 64) == (1, 0)               # linear_leaves, padding
    assert struct.unpack_from("<ii", rc, 64) == (0, 0)
    # two entries of the cache, side by side
    assert lin.key != con.key
    assert lin.key == compiled.cache_key(body, names, mp, K, True) and con.key == compiled.cache_key(body, names, mp, K)
    for b in (lin, con):
        for ext in (".co", ".so", ".json"):
            assert os.path.exists(os.path.join(compiled.cache_dir(), b.key + ext))
    meta = json.load(open(os.path.join(compiled.cache_dir(), lin.key + ".json")))
    assert meta["linear"] is True and meta["n_outputs"] == K
    again = compile_loglik(body, names, mp, K, linear=True)
    assert again.cached and again.linear and again.code == lin.code


def _guard_table_p128():
    spec = importlib.util.spec_from_file_location("occupancy_guard_here", os.path.join(ROOT, "tools", "occupancy_guard.py"))
    og = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(og)
    rows = og.table(os.path.join(ROOT, "pymc_bart_amd", "csrc", "libpgbart_hip_p128.so"))
    return {r["kernel"]: r for r in rows}


@pytest.mark.parametrize("body, names, K", [(CHECK_LOSS, ["b", "q"], 1), (PROBIT, [], 1), (POISSON, [], 1),
                                            (MEANSCALE, [], 2), (SOFTMAX, [], 3), (SOFTMAX, [], 6), (SOFTMAX, [], 16)],
                         ids=["check_loss", "probit", "poisson", "meanscale_k2", "softmax_k3", "softmax_k6", "softmax_k16"])
def test_linear_code_objects_keep_the_builtin_linear_instances_resources(body, names, K):
    inst = "k_loglik<1, -1, true>" if K == 1 else "k_loglik<0, -1, true>"  # (the built-in linear instance of that shape)
    assert BUDGET[inst]["min_wgs_per_cu"] == (4 if K == 1 else 3)
    r = compile_loglik(body, names, 64, K, linear=True).resources
    assert r["scratch_bytes"] == 0 and r["vgpr_spills"] == 0, r
    assert r["wgs_per_cu"] >= BUDGET[inst]["min_wgs_per_cu"], (r, BUDGET[inst])
    r128 = compile_loglik(body, names, 128, K, linear=True).resources
    assert r128["scratch_bytes"] == 0 and r128["vgpr_spills"] == 0, r128
    assert r128["wgs_per_cu"] >= _guard_table_p128()[inst]["wgs_per_cu"], r128


@pytest.mark.parametrize("response", ["linear", "mix"])
def test_a_compiled_sampler_with_linear_leaves_is_refused_on_a_cpu_backend(oracle, response):
    rng = np.random.default_rng(0)
    X = rng.normal(size=(200, 3))
    Y = rng.poisson(2.0, 200).astype(float)
    st = PyBartSettings.from_data(X, np.log(Y + 0.5), m=5, num_particles=6, family="compiled", response=response)
    with pytest.raises(_abi.PGBError, match="linear / mix leaves.*HIP backend only"):
        PySampler(st, X, Y, np.zeros(3, np.int32), np.ones(3), backend=oracle)
    with pytest.warns(UserWarning), pytest.raises(_abi.PGBError, match="HIP backend only"):
        PGBART([BARTOp(X, np.log(Y + 0.5), m=5, response=response)], num_particles=6,
               likelihood=CompiledLikelihood(POISSON), observed=Y, random_seed=1, backend=oracle)
    # constant leaves still run there (the body as the callback family)
    st0 = PyBartSettings.from_data(X, np.log(Y + 0.5), m=5, num_particles=6, family="compiled")
    s = PySampler(st0, X, Y, np.zeros(3, np.int32), np.ones(3), backend=oracle)
    s.set_compiled_likelihood(CompiledLikelihood(POISSON))
    s.set_likelihood([])
    assert np.all(np.isfinite(s.step(True)[0]))


def test_a_likelihood_pickles_and_its_copy_builds_the_same_linear_variant():
    lik = CompiledLikelihood(CHECK_LOSS, params={"b": 0.25, "q": 0.9})
    twin = pickle.loads(pickle.dumps(lik))
    a, b = lik.compiled(64, linear=True), twin.compiled(64, linear=True)
    assert a.key == b.key and b.linear and b.param_names == ("b", "q")
    assert a.key != lik.compiled(64).key and twin.compiled(64).key == lik.compiled(64).key
    assert lik.compiled(64, linear=True) is a                        # (kept per (particle build, leaves))
    assert set(lik._builds) == {(64, False), (64, True)}
    assert lik.compiled(100, linear=True).max_particles == 128
    k2 = pickle.loads(pickle.dumps(CompiledLikelihood(MEANSCALE, n_outputs=2)))
    assert k2.compiled(64, linear=True).n_outputs == 2 and k2.compiled(64, linear=True).linear
