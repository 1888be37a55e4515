"""Family "compiled" with linear / mix leaves on the MI355X: the code object's pass is the library's linear-leaf pass
(k_loglik<1, ., true>; K outputs: the run-time-K linear path with the K predictors of a row in an array) with the body
at every site a family is evaluated at -- the plain pass, the stump sum and the current-tree sum of a slot that starts
a tree.  No CPU backend runs this (the oracle's callback family has constant leaves), so the pin is transitive: a body
that restates a built-in family must be the SAME sampler as that family with linear leaves -- which the parity suite
holds to the oracle -- i.e. reproduce the committed fingerprints and, on random configurations and at size, every
step."""
import json
import os
import pickle
import warnings

import numpy as np
import pytest

from _cases import digest, make_case, random_case, run_case
from _restated_bodies import (CHECK_LOSS, MEANSCALE, POISSON, PROBIT, PROBIT_AUX, RESTATED, SOFTMAX, SOFTMAX_AUX)
from pymc_bart_amd import _abi, trees
from pymc_bart_amd.compiled import CompiledLikelihood, compile_loglik
from pymc_bart_amd.sampler import PyBartSettings, PySampler

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_runs.json")))


@pytest.fixture(autouse=True)
def _jit_cache(tmp_path_factory, monkeypatch):
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit"))


def _run(c, backend, lik, **kw):
    """run_case with the samplers it creates taking the compiled likelihood."""
    orig = PySampler.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        if self.settings.family == "compiled":
            self.set_compiled_likelihood(lik)

    PySampler.__init__ = init
    try:
        return run_case(c, backend, **kw)
    finally:
        PySampler.__init__ = orig


def _check_linear_build(smp, c):
    assert smp.backend.lib.backend_name == "hip-gfx950" and smp.settings.family == "compiled"
    assert smp.settings.response == c["response"] != "constant"
    assert smp.backend.lib.max_particles == (128 if c["P"] > 64 else 64)
    b = smp._cl_build
    assert b.linear and b.n_outputs == c.get("K", 1) and b.max_particles == smp.backend.lib.max_particles
    assert b.resources["scratch_bytes"] == 0


@pytest.mark.parametrize("name, body, aux_is_y", [
    ("linear_poisson", POISSON, False),
    ("mix_probit", PROBIT, False),
    ("mix_probit_mixed_rules", PROBIT, False),
    ("meanscale_k2_linear", MEANSCALE, False),
    ("categorical_k3_mix", SOFTMAX, False),
    ("categorical_k16_linear", SOFTMAX, False),
    ("categorical_k3_linear_mixed_rules", SOFTMAX, False),
    ("upstream/categorical_k3_linear_mixed_rules", SOFTMAX, False),
    ("mix_probit", PROBIT_AUX, True),            # the body ignores y: the aux column read under the linear pass
    ("categorical_k3_mix", SOFTMAX_AUX, True),   # ... and next to y in the K-output path
], ids=["linear_poisson", "mix_probit", "mix_probit_mixed_rules", "meanscale_k2_linear", "categorical_k3_mix",
        "categorical_k16_linear", "categorical_k3_linear_mixed_rules", "upstream-categorical_k3_linear_mixed_rules",
        "mix_probit-aux", "categorical_k3_mix-aux"])
def test_restated_bodies_reproduce_the_builtin_linear_fingerprints(hip, name, body, aux_is_y):
    c = dict(make_case(name))
    c["family"] = "compiled"
    lik = CompiledLikelihood(body, n_outputs=c.get("K", 1), aux=c["Y"] if aux_is_y else None)
    res = _run(c, hip, lik)
    _check_linear_build(res["sampler"], c)
    assert digest(res) == GOLD[name]


def _chain(X, Y, family, backend, K=1, lik=None, m=200, P=40, tune=10, draws=10, seed=7, checkpoint_at=None,
           params=(), offset=None, response="constant"):
    st = PyBartSettings.from_data(X, Y, m=m, num_particles=P, seed=seed, family=family, n_outputs=K, response=response)
    p = X.shape[1]

    def make():
        s = PySampler(st, X, Y, np.zeros(p, np.int32), np.ones(p), backend=backend)
        if lik is not None:
            s.set_compiled_likelihood(lik)
        if offset is not None:
            s.set_offset(offset)
        return s

    s = make()
    out = []
    for it in range(tune + draws):
        if checkpoint_at is not None and it == checkpoint_at:
            blob = s.checkpoint()
            s = make()
            s.restore(blob)
        s.set_likelihood(list(params))
        st_, vi = s.step(it < tune)
        ta = s.export_trees(0)
        out.append((st_.copy(), vi.copy(), np.concatenate([ta.var, ta.left, ta.right, ta.count, ta.split.view(np.int64),
                                                           ta.value.ravel().view(np.int64),
                                                           ta.slope.ravel().view(np.int64), ta.xbar.view(np.int64),
                                                           ta.svar])))
    return out, s


def _same(a, b):
    assert len(a) == len(b)
    for i, ((sa, va, ta), (sb, vb, tb)) in enumerate(zip(a, b)):
        assert np.array_equal(sa, sb) and np.array_equal(va, vb) and np.array_equal(ta, tb), f"astep {i}"


def _cfg2_data(n=100_000, p=50, seed=3415):  # (tools/compiled_family_timing.py: data)
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, p))
    f = 10 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 20 * (X[:, 2] - 0.5) ** 2 + 10 * X[:, 3] + 5 * X[:, 4]
    return X, f + rng.normal(0, 1.0 + X[:, 0], n)


def test_compiled_check_loss_with_linear_leaves_equals_the_builtin_at_cfg2_size(hip):
    X, Y = _cfg2_data()
    lik = CompiledLikelihood(CHECK_LOSS, params={"b": 0.25, "q": 0.9})
    a, _ = _chain(X, Y, "asymmetric_laplace", hip, params=[0.25, 0.9], response="linear")
    b, s = _chain(X, Y, "compiled", hip, lik=lik, params=[0.25, 0.9], response="linear")
    assert s._cl_build.linear and s._cl_build.resources["scratch_bytes"] == 0
    _same(a, b)


def test_compiled_meanscale_with_mix_leaves_equals_the_builtin_at_cfg2_size(hip):
    X, Y = _cfg2_data()
    lik = CompiledLikelihood(MEANSCALE, n_outputs=2)
    a, _ = _chain(X, Y, "normal_meanscale", hip, K=2, response="mix")
    b, s = _chain(X, Y, "compiled", hip, K=2, lik=lik, response="mix")
    assert s._cl_build.linear and s._cl_build.n_outputs == 2 and s._cl_build.resources["scratch_bytes"] == 0
    assert a[-1][0].shape == (2, X.shape[0])
    _same(a, b)


def _fuzz(hip, seeds, large):
    ran, fams, liks = 0, set(), {}
    for seed in seeds:
        c = random_case(seed, large=large)
        if c["family"] == "normal" or c["response"] == "constant":
            continue
        body, names = RESTATED[c["family"]]
        assert len(names) == len(c.get("lik_params", []))
        want = digest(run_case(c, hip))
        cc = dict(c)
        cc["family"] = "compiled"
        key = (c["family"], c["K"])
        if key not in liks:
            liks[key] = CompiledLikelihood(body, params={nm: 0.0 for nm in names}, n_outputs=c["K"])
        res = _run(cc, hip, liks[key])
        _check_linear_build(res["sampler"], cc)
        assert digest(res) == want, (seed, c["family"], c["K"], c["response"], c["P"], c["X"].shape)
        ran += 1
        fams.add(c["family"])
    return ran, fams


def test_fuzz_small_compiled_linear_equals_the_builtin_families(hip):
    ran, fams = _fuzz(hip, range(300), large=False)
    assert ran == 66
    assert fams == set(RESTATED)                                     # all nine per-row families occur


def test_fuzz_large_compiled_linear_equals_the_builtin_families(hip):
    ran, _ = _fuzz(hip, range(60), large=True)
    assert ran == 13


def test_code_objects_of_the_other_leaves_are_refused_without_a_launch(hip):
    rng = np.random.default_rng(2)
    X = rng.normal(size=(3000, 4))
    Y = rng.poisson(2.0, 3000).astype(float)
    bY = np.log(Y + 0.5)
    mk = lambda resp: PySampler(PyBartSettings.from_data(X, bY, m=6, num_particles=8, seed=5, family="compiled",  # noqa: E731
                                                         response=resp),
                                X, Y, np.zeros(4, np.int32), np.ones(4), backend=hip)
    s_lin, s_mix, s_con = mk("linear"), mk("mix"), mk("constant")
    set_code, _ = hip.lib.compiled_entry_points()
    con = compile_loglik(POISSON, []).code
    lin = compile_loglik(POISSON, [], linear=True).code
    for s, blob, msg in ((s_lin, con, "compiled for constant leaves, the sampler has response = linear"),
                         (s_mix, con, "compiled for constant leaves, the sampler has response = mix"),
                         (s_con, lin, "compiled for linear leaves, the sampler has response = constant")):
        assert set_code(s._h, blob, len(blob), 0) == -1                 # PGB_E_INVALID
        assert msg in s.backend.lib.lib.pgb_last_error().decode()
        with pytest.raises(_abi.PGBError, match="pgb_set_loglik_code first"):
            s.step(True)                                                  # nothing was installed, nothing launched
    lik = CompiledLikelihood(POISSON)
    for s in (s_lin, s_mix, s_con):                                       # the right one: the chain steps
        s.set_compiled_likelihood(lik)
        assert s._cl_build.linear == (s.settings.response != "constant")
        for it in range(4):
            s.set_likelihood([])
            st_, _ = s.step(it < 2)
            assert st_.shape == (3000,) and np.all(np.isfinite(st_))


def test_checkpoint_round_trip_of_compiled_linear_chains(hip):
    X, Y = _cfg2_data(n=20_000, p=6, seed=5)
    lik1 = CompiledLikelihood(CHECK_LOSS, params={"b": 0.25, "q": 0.9})
    kw = dict(m=20, P=20, tune=5, draws=5, params=[0.25, 0.9], response="linear", offset=np.full(20_000, 0.1))
    a, _ = _chain(X, Y, "compiled", hip, lik=lik1, **kw)
    b, _ = _chain(X, Y, "compiled", hip, lik=lik1, checkpoint_at=4, **kw)
    _same(a, b)
    lik2 = CompiledLikelihood(MEANSCALE, n_outputs=2)
    kw = dict(m=20, P=20, tune=5, draws=5, response="mix")
    a, _ = _chain(X, Y, "compiled", hip, K=2, lik=lik2, **kw)
    b, _ = _chain(X, Y, "compiled", hip, K=2, lik=lik2, checkpoint_at=7, **kw)
    _same(a, b)
    assert any(np.any(t[0] != a[0][0]) for t in a[1:])


def test_pgbart_with_a_compiled_poisson_and_linear_leaves(hip):
    from pymc_bart_amd.pgbart import PGBART, BARTOp

    rng = np.random.default_rng(33)
    n, m = 4000, 10
    X = rng.uniform(-2, 2, (n, 3))
    f = np.where(X[:, 0] < 0, X[:, 0] + 1.5, -0.8 * X[:, 0] + 1.5) + 0.4 * X[:, 1]
    Y = rng.poisson(np.exp(f)).astype(float)
    post, rmse = {}, {}
    for r in ("constant", "linear", "mix"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                           # (linear / mix: flagged experimental, as upstream)
            step = PGBART([BARTOp(X, np.log(Y + 0.5), m=m, response=r)], num_particles=12,
                          likelihood=CompiledLikelihood(POISSON), observed=Y, random_seed=9, backend=hip)
        assert step.sampler.backend.lib.backend_name == "hip-gfx950"
        assert step.sampler._cl_build.linear == (r != "constant")
        draws = []
        for it in range(300):
            if it == 150:
                step.stop_tuning()
            if it == 200 and r == "mix":                              # a pickled step method rebuilds the linear variant
                step = pickle.loads(pickle.dumps(step))
                assert step.sampler._cl_build.linear
            mu, _ = step.astep(None, {})
            if it >= 150:
                draws.append(np.array(mu))
        post[r] = np.mean(draws, axis=0)
        rmse[r] = float(np.sqrt(np.mean((post[r] - f) ** 2)))
        if r != "constant":  # linear leaves of a compiled chain export and predict
            forest = step.sampler.export_trees(1)
            pred = trees.predict_numpy(forest, np.arange(m)[None, :], step._X[:300])[0, 0]
            err = float(np.max(np.abs(pred - np.asarray(mu)[:300])))
            print(f"response={r}: predict vs sum_trees max abs err {err:.3g}, "
                  f"non-zero slopes {int(np.count_nonzero(forest.slope))}")
            assert err <= 1e-12, err
            assert np.count_nonzero(forest.slope) >= 1
    corr = float(np.corrcoef(post["linear"], f)[0, 1])
    print("rmse", rmse, "corr(linear)", corr)
    # (the built-in PoissonLikelihood on the CPU oracle, this recipe: rmse constant 0.19302, linear 0.13922 (corr
    #  0.9813), mix 0.14861; the compiled body is the same sampler bit for bit)
    assert rmse["linear"] < rmse["constant"], rmse
    assert rmse["mix"] < rmse["constant"], rmse
    assert corr > 0.97, corr
