"""``pgb_set_loglik_code`` on the MI355X through the one loader of compiled code objects (csrc/pgb_compiled_host.h:
``compiled_load_code``): every object that is not this sampler's pass kernel is refused with the sentence that names its
reason -- all of them host-side comparisons of the layout record, made before any launch -- and a refusal leaves the
loaded module, its probe kernel and the chain exactly as they were."""
import hashlib

import numpy as np
import pytest

from pymc_bart_amd import _abi
from pymc_bart_amd.compiled import CompiledLikelihood, compile_loglik, compile_sampler
from pymc_bart_amd.sampler import PyBartSettings, PySampler

pytestmark = pytest.mark.gpu
BODY = "double z = (y - mu) / s;  return -0.5 * z * z - log(s);"
N, P, M = 257, 3, 5


@pytest.fixture(autouse=True)
def _jit_cache(tmp_path_factory, monkeypatch):
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit"))


def _step_digest(s) -> str:
    s.set_likelihood([0.5])
    sum_trees, vi = s.step(True)
    ta = s.export_trees(0)
    h = hashlib.sha256()
    for a in (sum_trees, vi, ta.var, ta.left, ta.right, ta.count, ta.split, ta.value):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_a_refused_object_names_its_reason_and_leaves_the_loaded_module_alone(hip):
    rng = np.random.default_rng(257)
    X = rng.uniform(0, 1, (N, P))
    Y = np.sin(3 * X[:, 0]) + 0.3 * rng.standard_normal(N)
    lik = CompiledLikelihood(BODY, params={"s": 0.5})
    st = PyBartSettings.from_data(X, Y, m=M, num_particles=10, seed=11, family="compiled")

    def chain():
        s = PySampler(st, X, Y, np.zeros(P, np.int32), np.ones(P), backend=hip)
        s.set_compiled_likelihood(lik)
        s.set_likelihood([0.5])
        return s

    s = chain()
    assert s.backend.lib.max_particles == 64
    mu = rng.normal(0, 1, N)
    want = s.compiled_probe(Y, mu).view(np.int64)
    first = _step_digest(s)
    refused = [
        (compile_loglik(BODY, ["s"], pointwise=True), 1,
         r"built with pointwise=True \(k_pointwise_compiled\), mark 1: pgb_set_loglik_code takes one built without "
         r"pointwise=True \(a sampler's pass kernel, k_loglik_compiled\)"),
        (compile_sampler("return mu + s * normal();", ["s"]), 1,
         r"built from a sampler body \(k_ppc_compiled\), mark 2: pgb_set_loglik_code takes one built without "
         r"pointwise=True \(a sampler's pass kernel, k_loglik_compiled\)"),
        (compile_loglik(BODY, ["s"], max_particles=128), 1, r"another particle build \(this library takes 64\)"),
        (compile_loglik(BODY, ["s"], linear=True), 1, "compiled for linear leaves, the sampler has response = constant"),
        (compile_loglik(BODY.replace("mu", "mu[0]").replace("log(s)", "log(s) * mu[1]"), ["s"], n_outputs=2), 1,
         "compiled for 2 outputs, the sampler has n_outputs = 1"),
        (compile_loglik(BODY.replace("log(s)", "log(s * t)"), ["s", "t"]), 1,
         "compiled for 2 params, the call gives n_params = 1"),
    ]
    set_code, _ = s.backend.lib.compiled_entry_points()
    for build, n_params, msg in refused:
        rc = set_code(s._h, build.code, len(build.code), n_params)
        assert rc == -1, (rc, msg)                                        # PGB_E_INVALID
        with pytest.raises(_abi.PGBError, match=msg):
            s.backend.lib.check(rc, "pgb_set_loglik_code")
        assert np.array_equal(s.compiled_probe(Y, mu).view(np.int64), want), msg   # the loaded module still answers
    second = _step_digest(s)
    twin = chain()                                                        # never saw a refusal
    assert np.array_equal(twin.compiled_probe(Y, mu).view(np.int64), want)
    assert (_step_digest(twin), _step_digest(twin)) == (first, second)
