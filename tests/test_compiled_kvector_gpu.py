"""Family "compiled" with K-vector leaves on the MI355X: a body of K predictors runs inside the library's K-vector
likelihood pass (k_loglik<K> / k_loglik<0>).  Bodies that restate the built-in families must be the SAME sampler as
them -- the committed fingerprints and, at size, every step -- and the device's values of any body must be its host
build's, bit for bit (the probe kernel)."""
import json
import os

import numpy as np
import pytest

from _cases import digest, make_case, run_case
from pymc_bart_amd import _abi
from pymc_bart_amd.compiled import CompiledLikelihood, compile_loglik
from pymc_bart_amd.sampler import PyBartSettings, PySampler
from pymc_bart_amd.workloads import cfg5

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_runs.json")))

# pgb_loglik_meanscale_t and pgb_loglik_cat_t, operation for operation (see tests/test_compiled_kvector.py)
MEANSCALE = """double sd = mu[1] < 0.0 ? -mu[1] : mu[1];
if (!(sd >= 1e-8)) sd = 1e-8;
if (sd > 1.0e300) sd = 1.0e300;
double z = (y - mu[0]) / sd;
return -log(sd) - 0.5 * (z * z);"""
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
# Gamma with mean exp(mu[0]) and shape exp(mu[1]) (rate = shape / mean)
GAMMA = """double a = exp(mu[1]);
return a * (mu[1] - mu[0]) - lgamma(a) + (a - 1.0) * log(y) - a * y * exp(-mu[0]);"""
# zero-inflated Poisson: log rate mu[0], logit of the zero probability mu[1]
ZIP = """double lam = exp(mu[0]);
double lpi = -softplus(-mu[1]);
double l1pi = -softplus(mu[1]);
if (y < 0.5) {
  double b = l1pi - lam;
  double mx = fmax(lpi, b);
  return mx + log(exp(lpi - mx) + exp(b - mx));
}
return l1pi + y * mu[0] - lam - lgamma(y + 1.0);"""
LGAMMA = "return lgamma(y + aux) - lgamma(fabs(mu[0]) + w) + 0.0 * mu[1];"


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


@pytest.mark.parametrize("name", ["meanscale_k2_reference", "categorical_k3_reference", "categorical_k4_cfg5_small",
                                  "categorical_k6_generic", "categorical_k12", "categorical_k3_offset",
                                  "stump_first_categorical", "categorical_k4_particles_100"])
def test_restated_bodies_reproduce_the_builtin_fingerprints(hip, name):
    c = dict(make_case(name))
    K = c["K"]
    c["family"] = "compiled"
    lik = CompiledLikelihood(MEANSCALE if name.startswith("meanscale") else SOFTMAX, n_outputs=K)
    res = _run(c, hip, lik)
    smp = res["sampler"]
    assert smp.backend.lib.backend_name == "hip-gfx950" and smp.settings.n_outputs == K
    assert smp.backend.lib.max_particles == (128 if c["P"] > 64 else 64)
    assert digest(res) == GOLD[name]


def _chain(X, Y, family, backend, K, lik=None, m=200, P=40, tune=10, draws=10, seed=7, checkpoint_at=None,
           params=(), offset=None):
    st = PyBartSettings.from_data(X, Y, m=m, num_particles=P, seed=seed, family=family, n_outputs=K)
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
                                                           ta.value.ravel().view(np.int64)])))
    return out, s


def _same(a, b):
    assert len(a) == len(b)
    for i, ((sa, va, ta), (sb, vb, tb)) in enumerate(zip(a, b)):
        assert np.array_equal(sa, sb) and np.array_equal(va, vb) and np.array_equal(ta, tb), f"astep {i}"


def _meanscale_data(n=100_000, p=50, seed=3415):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, p))
    f = 10 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 20 * (X[:, 2] - 0.5) ** 2 + 10 * X[:, 3] + 5 * X[:, 4]
    return X, f + rng.normal(0, 1.0 + X[:, 0], n)


def test_compiled_meanscale_equals_the_builtin_at_size(hip):
    X, Y = _meanscale_data()
    lik = CompiledLikelihood(MEANSCALE, n_outputs=2)
    a, _ = _chain(X, Y, "normal_meanscale", hip, 2)
    b, s = _chain(X, Y, "compiled", hip, 2, lik=lik)
    assert s._cl_build.resources["scratch_bytes"] == 0 and s.settings.family == "compiled"
    assert a[-1][0].shape == (2, X.shape[0])
    _same(a, b)


def test_compiled_softmax_equals_the_builtin_at_cfg5_size(hip):
    w = cfg5()
    lik = CompiledLikelihood(SOFTMAX, n_outputs=4)
    a, _ = _chain(w["X"], w["Y"], "categorical", hip, 4, m=w["m"], P=w["num_particles"])
    b, _ = _chain(w["X"], w["Y"], "compiled", hip, 4, lik=lik, m=w["m"], P=w["num_particles"])
    _same(a, b)


def _probe_grid(n, seed, y_kind):
    rng = np.random.default_rng(seed)
    # (predictors within pgb_exp_t's domain, |x| < 4.6e7, and NaN)
    edges = np.array([0.0, -0.0, 1e-300, 1e-9, -1e-9, 1.0, -1.0, 36.5, -36.5, 700.0, -700.0, 745.0, -745.0, 1e5, -1e5,
                      np.nan])
    mu = np.where(rng.random((2, n)) < 0.25, rng.choice(edges, (2, n)), rng.normal(0, 2, (2, n)))
    if y_kind == "counts":
        y = rng.poisson(2.0, n).astype(float)
    else:
        y = rng.gamma(2.0, 1.5, n)
    odd = rng.random(n) < 0.1
    y[odd] = rng.choice([0.0, -1.0, 1e-300, 1e300, 0.5, np.inf, np.nan], int(odd.sum()))
    aux = rng.uniform(0, 3, n)
    aux[rng.random(n) < 0.05] = 0.0
    return np.ascontiguousarray(y), np.ascontiguousarray(mu), aux


@pytest.mark.parametrize("body, params, kind", [(GAMMA, {}, "pos"), (ZIP, {}, "counts"), (LGAMMA, {"w": 1e-6}, "pos")])
def test_the_probe_equals_the_host_build_bit_for_bit(hip, body, params, kind):
    y, mu, aux = _probe_grid(50_000, seed=len(body), y_kind=kind)
    lik = CompiledLikelihood(body, params=params, n_outputs=2)
    rng = np.random.default_rng(0)
    X = rng.normal(size=(500, 3))
    st = PyBartSettings.from_data(X, np.abs(rng.normal(size=500)) + 0.1, m=4, num_particles=4, family="compiled",
                                  n_outputs=2)
    s = PySampler(st, X, st.init_sum + np.zeros(500), np.zeros(3, np.int32), np.ones(3), backend=hip)
    s.set_compiled_likelihood(lik)
    s.set_likelihood(list(params.values()))
    dev = s.compiled_probe(y, mu, aux)
    host = lik.compiled(64).host_eval(y, mu, aux, list(params.values()))
    bad = np.flatnonzero(dev.view(np.int64) != host.view(np.int64))
    assert bad.size == 0, (bad[:5], y[bad[:5]], mu[:, bad[:5]], dev[bad[:5]], host[bad[:5]])
    assert np.all((dev >= -2047.0) & (dev <= 2047.0))
    assert (dev > -2047.0).mean() > 0.5                                   # (most rows are inside the range)


def test_code_objects_of_the_wrong_k_are_refused_without_a_launch(hip):
    rng = np.random.default_rng(2)
    X = rng.normal(size=(3000, 4))
    Y = rng.gamma(2.0, 1.0, 3000)
    st2 = PyBartSettings.from_data(X, Y, m=6, num_particles=8, seed=5, family="compiled", n_outputs=2)
    st1 = PyBartSettings.from_data(X, Y, m=6, num_particles=8, seed=5, family="compiled", n_outputs=1)
    s2 = PySampler(st2, X, Y, np.zeros(4, np.int32), np.ones(4), backend=hip)
    s1 = PySampler(st1, X, Y, np.zeros(4, np.int32), np.ones(4), backend=hip)
    set_code, _ = hip.lib.compiled_entry_points()
    k3 = compile_loglik(SOFTMAX, [], n_outputs=3).code
    k2 = compile_loglik(GAMMA, [], n_outputs=2).code
    k1 = compile_loglik("return -(y - mu) * (y - mu);", []).code
    for s, blob, msg in ((s2, k3, "compiled for 3 outputs, the sampler has n_outputs = 2"),
                         (s2, k1, "compiled for 1 outputs, the sampler has n_outputs = 2"),
                         (s1, k2, "compiled for 2 outputs, the sampler has n_outputs = 1")):
        assert set_code(s._h, blob, len(blob), 0) == -1                 # PGB_E_INVALID
        assert msg in s.backend.lib.lib.pgb_last_error().decode()
        with pytest.raises(_abi.PGBError, match="pgb_set_loglik_code first"):
            s.step(True)                                                  # nothing was installed, nothing launched
    with pytest.raises(_abi.PGBError, match="3 outputs, the sampler n_outputs = 2"):
        s2.set_compiled_likelihood(CompiledLikelihood(SOFTMAX, n_outputs=3))
    s2.set_compiled_likelihood(CompiledLikelihood(GAMMA, n_outputs=2))
    for it in range(4):
        s2.set_likelihood([])
        st_, _ = s2.step(it < 2)
        assert st_.shape == (2, 3000) and np.all(np.isfinite(st_))


def test_checkpoint_round_trip_and_two_chains_on_one_gpu(hip):
    X, Y = _meanscale_data(n=20_000, p=6, seed=5)
    Yp = np.abs(Y) + 0.5
    lik = CompiledLikelihood(GAMMA, n_outputs=2)
    off = np.concatenate([np.full(20_000, 0.1), np.zeros(20_000)])
    kw = dict(m=20, P=20, tune=5, draws=5, offset=off)
    a, _ = _chain(X, Yp, "compiled", hip, 2, lik=lik, **kw)
    b, _ = _chain(X, Yp, "compiled", hip, 2, lik=lik, checkpoint_at=4, **kw)
    _same(a, b)
    # two chains of different seeds, stepped in turn on one GPU: each equals its solo run
    solo = {sd: _chain(X, Yp, "compiled", hip, 2, lik=lik, seed=sd, **kw)[0] for sd in (7, 8)}
    st = {sd: PyBartSettings.from_data(X, Yp, m=20, num_particles=20, seed=sd, family="compiled", n_outputs=2)
          for sd in (7, 8)}
    smp = {}
    for sd in (7, 8):
        smp[sd] = PySampler(st[sd], X, Yp, np.zeros(6, np.int32), np.ones(6), backend=hip)
        smp[sd].set_compiled_likelihood(lik)
        smp[sd].set_offset(off)
    for it in range(10):
        for sd in (7, 8):
            smp[sd].set_likelihood([])
            st_, vi = smp[sd].step(it < 5)
            assert np.array_equal(st_, solo[sd][it][0]) and np.array_equal(vi, solo[sd][it][1])
    assert not np.array_equal(solo[7][-1][0], solo[8][-1][0])


def test_pgbart_with_a_heteroscedastic_gamma_recovers_mean_and_shape(hip):
    from pymc_bart_amd.pgbart import PGBART, BARTOp

    rng = np.random.default_rng(21)
    n = 20_000
    X = rng.uniform(-1, 1, (n, 4))
    log_mean = 1.0 + 0.8 * np.sin(2.0 * X[:, 0])                      # the mean's function
    log_shape = 1.5 + 1.0 * X[:, 1]                                    # the shape's function (shape 1.6 .. 12)
    shape = np.exp(log_shape)
    Y = rng.gamma(shape, np.exp(log_mean) / shape)
    lik = CompiledLikelihood(GAMMA, n_outputs=2)
    step = PGBART([BARTOp(X, np.log(Y), m=50)], num_particles=20, likelihood=lik, observed=Y, random_seed=9,
                  backend=hip)
    assert step.shape == (2, n)
    draws = []
    for it in range(150):
        if it == 75:
            step.stop_tuning()
        mu, _ = step.astep(None, {})
        assert np.shape(mu) == (2, n)
        if it >= 75:
            draws.append(np.array(mu))
    post = np.mean(draws, axis=0)
    c_mean = np.corrcoef(post[0], log_mean)[0, 1]
    c_shape = np.corrcoef(post[1], log_shape)[0, 1]
    rmse_mean = float(np.sqrt(np.mean((post[0] - log_mean) ** 2)))
    rmse_shape = float(np.sqrt(np.mean((post[1] - log_shape) ** 2)))
    # (the chain is deterministic; observed on the MI355X: corr 0.9944 / 0.9757, rmse 0.0663 / 0.1311)
    assert c_mean > 0.99 and c_shape > 0.97, (c_mean, c_shape)
    assert rmse_mean < 0.08 and rmse_shape < 0.15, (rmse_mean, rmse_shape)
