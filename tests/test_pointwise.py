"""Pointwise log-likelihood / lppd / WAIC, on the build box (no GPU): the numeric contract of
``include/pgbart_logpdf.h`` against SciPy -- the ABSOLUTE densities of every built-in family, no mask, nothing
clamped -- its reduction over draws against ``logsumexp`` and a long-double variance, the argument validation of
``pymc_bart_amd.pointwise``, and the cross-compiled pointwise code object of a compiled body."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest
from scipy import special, stats

import _pointwise_host as host
from pymc_bart_amd import (AsymmetricLaplaceLikelihood, BernoulliLikelihood, CallbackLikelihood, CategoricalLikelihood,
                           CompiledLikelihood, NormalLikelihood, NormalMeanScaleLikelihood, StudentTLikelihood, compiled)
from pymc_bart_amd.compiled import compile_loglik
from pymc_bart_amd.pointwise import log_predictive_density, pointwise_log_likelihood
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20_000


@pytest.fixture(autouse=True)
def _jit_cache(tmp_path_factory, monkeypatch):
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit"))


def _check(family, y, mu, params, want, tol):
    """Every row, the absolute density: zero rows excluded, zero clamped."""
    got, n_clamped = host.logpdf(family, y, mu, params, return_clamped=True)
    assert np.all(np.isfinite(want)) and want.min() > -2047.0 and want.max() < 2047.0  # (the reference alone)
    assert n_clamped == 0 and got.shape == want.shape
    err = np.max(np.abs(got - want) / (1.0 + np.abs(want)))
    print(f"{family} {list(params)}: max scaled error {err:.3e} (tolerance {tol:g}); min {want.min():.1f} max {want.max():.2f}")
    assert err < tol, (family, params, err)


# ------------------------------------------------------------------ 1. densities against SciPy
def test_normal_density_against_scipy():
    rng = np.random.default_rng(0)
    y, mu = rng.normal(0, 2, N), rng.uniform(-3, 3, N)
    for sigma in (0.5, 1.0, 2.5):
        _check("normal", y, mu, [sigma], stats.norm.logpdf(y, mu, sigma), 1e-10)


def test_student_t_density_against_scipy():
    rng = np.random.default_rng(0)
    y, mu = rng.standard_t(3, N), rng.uniform(-3, 3, N)
    for sigma, nu in ((0.2, 3.0), (1.0, 4.0), (2.5, 30.0)):
        _check("student_t", y, mu, [sigma, nu], stats.t.logpdf(y, nu, loc=mu, scale=sigma), 1e-10)


def test_asymmetric_laplace_density_against_scipy():
    """The Yu-Moyeed density, log(q (1 - q) / b) included: scipy's laplace_asymmetric with kappa^2 = q / (1 - q),
    scale = b / sqrt(q (1 - q))."""
    rng = np.random.default_rng(0)
    y, mu = rng.normal(0, 2, N), rng.uniform(-3, 3, N)
    for b, q in ((0.25, 0.9), (1.0, 0.5), (2.0, 0.1)):
        kappa, scale = np.sqrt(q / (1 - q)), b / np.sqrt(q * (1 - q))
        _check("asymmetric_laplace", y, mu, [b, q], stats.laplace_asymmetric.logpdf(y, kappa, loc=mu, scale=scale), 1e-10)


def test_gamma_density_against_scipy():
    rng = np.random.default_rng(0)
    y, mu = rng.gamma(2.0, 1.5, N), rng.uniform(-1.5, 3, N)
    for alpha in (0.7, 3.0, 12.0):
        _check("gamma_log", y, mu, [alpha], stats.gamma.logpdf(y, alpha, scale=np.exp(mu) / alpha), 1e-9)


def test_count_densities_against_scipy():
    rng = np.random.default_rng(0)
    y, mu = rng.poisson(4.0, N).astype(float), rng.uniform(-1, 3, N)
    _check("poisson_log", y, mu, [], stats.poisson.logpmf(y, np.exp(mu)), 1e-9)
    for alpha in (0.5, 2.0, 9.0):
        _check("negbin_log", y, mu, [alpha], stats.nbinom.logpmf(y, alpha, alpha / (alpha + np.exp(mu))), 1e-9)


def test_bernoulli_densities_against_scipy():
    rng = np.random.default_rng(0)
    y, mu = (rng.random(N) < 0.4).astype(float), rng.uniform(-8, 8, N)
    s = np.where(y > 0.5, mu, -mu)
    _check("bernoulli_probit", y, mu, [], special.log_ndtr(s), 1e-12)
    _check("bernoulli_logit", y, mu, [], -np.logaddexp(0.0, -s), 1e-12)


def test_categorical_density_against_scipy():
    rng = np.random.default_rng(0)
    for K in (2, 3, 4, 8, 16):
        mu = rng.normal(0, 2, (K, N))
        y = rng.integers(0, K, N).astype(float)
        _check("categorical", y, mu, [], special.log_softmax(mu, axis=0)[y.astype(int), np.arange(N)], 1e-12)


def test_mean_scale_density_against_scipy():
    rng = np.random.default_rng(0)
    y = rng.normal(0, 1, N)
    mu = np.stack([rng.normal(0, 1, N), rng.uniform(0.3, 2.0, N) * rng.choice([-1.0, 1.0], N)])
    _check("normal_meanscale", y, mu, [], stats.norm.logpdf(y, mu[0], np.abs(mu[1])), 1e-10)


def test_params_outside_the_domain_are_refused_and_the_clamp_is_counted():
    y, mu = np.zeros(4), np.zeros(4)
    for family, prm in (("normal", [0.0]), ("normal", [np.nan]), ("asymmetric_laplace", [1.0, 1.0]), ("gamma_log", [-1.0])):
        with pytest.raises(ValueError):
            host.logpdf(family, y, mu, prm)
    got, nc = host.logpdf("normal", np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1e-4]), [1e-3], return_clamped=True)
    assert nc == 1 and got[1] == -2047.0 and got[0] > 0.0 and got[2] > 0.0   # ((1 / 1e-3)^2 / 2 = 5e5 below the bound)


# ------------------------------------------------------------------ 2. the reduction against SciPy
def _matrix(rng, D, n=600):
    ll = rng.normal(-3.0, 2.0, (D, n)) * rng.choice([1.0, 1.0, 30.0, 200.0], n)
    ll = np.clip(ll, -2047.0, 2047.0)
    ll[:, 0:20] = np.where(rng.random((D, 20)) < 0.3, -2047.0, ll[:, 0:20])  # rows that hold clamped entries
    ll[:, 20:30] = -2047.0                                                      # ... and nothing else
    ll[:, 30:50] = rng.normal(-5.0, 3.0, 20)[None, :]                           # identical values: var exactly 0
    return np.ascontiguousarray(ll)


def test_reduction_over_draws_against_scipy():
    C_ = host.chunk()
    assert C_ == 32
    rng = np.random.default_rng(0)
    for D in (1, 2, C_ - 1, C_, C_ + 1, 3 * C_ + 5):
        ll = _matrix(rng, D)
        lppd, mean, var = host.reduce(ll)
        want = special.logsumexp(ll, axis=0) - np.log(D)
        bound = (D + 16) * 2.3e-16 * (1.0 + np.abs(want))
        err = np.abs(lppd - want)
        print(f"D={D}: lppd max error / bound = {np.max(err / bound):.3f}")
        assert np.all(err <= bound), (D, np.max(err / bound))
        L = ll.astype(np.longdouble)
        m = L.mean(axis=0)
        v2 = ((L - m) ** 2).sum(axis=0) / max(D - 1, 1)          # long-double two-pass
        assert np.all(var[30:50] == 0.0) and np.all(var[20:30] == 0.0)
        if D == 1:
            assert np.all(var == 0.0) and np.array_equal(mean, ll[0])
            continue
        ok = np.asarray(v2, float) >= 0.01
        assert ok.sum() > 400
        tol = 8 * D * 2.0 ** -53 * (1.0 + np.asarray(m * m / np.where(ok, v2, 1.0), float))
        rel = np.abs(var - np.asarray(v2, float)) / np.asarray(np.where(ok, v2, 1.0), float)
        print(f"D={D}: var max error / bound = {np.max((rel / tol)[ok]):.3f}")
        assert np.all(rel[ok] <= tol[ok]), (D, np.max((rel / tol)[ok]))
        assert np.allclose(mean, np.asarray(m, float), rtol=1e-13, atol=1e-13)


# ------------------------------------------------------------------ 3. argument validation (no backend is touched)
class _NoBackend:
    """Any use of the backend is an AttributeError, not the ValueError the checks must raise first."""


def _sampler(K=1, draws=5, m=3):
    pool = TreeArrays.empty(m, m, K)                      # m stumps
    pool.tree_id[:] = np.arange(m)
    pool.node_off[:] = np.arange(m + 1)
    pool.var[:] = -1
    pool.count[:] = 10
    return PosteriorSampler(pool, np.tile(np.arange(m, dtype=np.int32), (draws, 1)), m, K, backend=_NoBackend())


@pytest.mark.parametrize("fn", [pointwise_log_likelihood, log_predictive_density])
def test_argument_errors_are_raised_before_a_backend_is_touched(fn):
    s = _sampler()
    X, y = np.zeros((8, 2)), np.zeros(8)
    lik = NormalLikelihood(1.0)
    with pytest.raises(ValueError, match="shape"):
        fn(s, X, np.zeros(7), lik)
    with pytest.raises(ValueError, match="matrix"):
        fn(s, np.zeros((2, 2, 2)), y, lik)
    with pytest.raises(ValueError, match="finite"):
        fn(s, X, np.where(np.arange(8) == 3, np.nan, 0.0), lik)
    with pytest.raises(ValueError, match="offset must have shape"):
        fn(s, X, y, lik, offset=np.zeros((2, 8)))
    with pytest.raises(ValueError, match="offset must be finite"):
        fn(s, X, y, lik, offset=np.full(8, np.inf))
    with pytest.raises(ValueError, match="offset must be finite"):
        fn(s, X, y, lik, offset=np.full(8, 2e6))
    with pytest.raises(ValueError, match="one point per draw"):
        fn(s, X, y, NormalLikelihood("sigma"), points=[{"sigma": 1.0}] * 4)
    with pytest.raises(ValueError, match="one value per draw"):
        fn(s, X, y, NormalLikelihood("sigma"), points={"sigma": np.ones(4)})
    with pytest.raises(ValueError, match="draws must index"):
        fn(s, X, y, lik, draws=[0, 5])

    class Two(NormalLikelihood):  # a likelihood whose params() disagrees with its family
        def params(self, point=None):
            return [1.0, 2.0]

    with pytest.raises(ValueError, match="takes 1 params"):
        fn(s, X, y, Two())
    with pytest.raises(ValueError, match="n_outputs"):
        fn(s, X, y, CategoricalLikelihood(3))              # K mismatch: the trees have one output
    with pytest.raises(ValueError, match="n_outputs"):
        fn(_sampler(K=3), X, y, NormalMeanScaleLikelihood())
    with pytest.raises(ValueError, match="n_outputs"):
        fn(_sampler(K=2), X, y, StudentTLikelihood())
    with pytest.raises(ValueError, match="callback"):
        fn(s, X, y, CallbackLikelihood(lambda yy, mu: -(yy - mu) ** 2))
    with pytest.raises(ValueError, match="aux"):
        fn(s, X, y, CompiledLikelihood("return -(y - mu) * (y - mu) - aux;", aux=np.zeros(5)))
    with pytest.raises(TypeError):
        fn(object(), X, y, lik)
    # a call that passes every check reaches the backend (here: none)
    for good in (dict(likelihood=lik), dict(likelihood=BernoulliLikelihood("logit")),
                 dict(likelihood=AsymmetricLaplaceLikelihood(0.5, "b"), points={"b": np.ones(5)})):
        with pytest.raises(AttributeError):
            fn(s, X, y, **good)


# ------------------------------------------------------------------ 4. cross-compilation
BODY = "double z = (y - mu) / s;  return -log(s) - 0.5 * z * z - aux;"


def _symbols(code: bytes, tmp_path) -> str:
    p = tmp_path / "k.co"
    p.write_bytes(code)
    return subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--symbols", str(p)], text=True)


def _record(code: bytes):
    from test_compiled_kvector import _elf_symbol_bytes

    rec = _elf_symbol_bytes(code, "pgb_compiled_layout_record")
    magic, _mp, n_params, n_outputs = struct.unpack_from("<iiii", rec, 0)
    (hh,) = struct.unpack_from("<Q", rec, 56)
    linear, pointwise = struct.unpack_from("<ii", rec, 64)
    return magic, n_params, n_outputs, hh, linear, pointwise


def test_a_pointwise_code_object_holds_its_own_kernel_and_says_so(tmp_path):
    b = compile_loglik(BODY, ["s"], pointwise=True)
    syms = _symbols(b.code, tmp_path)
    assert " k_pointwise_compiled\n" in syms and "k_loglik_compiled" not in syms
    assert _record(b.code) == (0x43424750, 1, 1, compiled.headers_hash(), 0, 1)
    assert b.pointwise and b.resources["vgpr_spills"] == 0
    k2 = compile_loglik("return -(y - mu[0]) * (y - mu[0]) - fabs(mu[1]);", [], n_outputs=2, pointwise=True)
    assert _record(k2.code)[1:3] == (0, 2) and _record(k2.code)[5] == 1
    # the same body without the flag: what it yields today -- the sampler's pass kernel and the probe, mark 0
    a = compile_loglik(BODY, ["s"])
    syms = _symbols(a.code, tmp_path)
    assert " k_loglik_compiled\n" in syms and " k_loglik_compiled_probe\n" in syms and "k_pointwise" not in syms
    assert _record(a.code) == (0x43424750, 1, 1, compiled.headers_hash(), 0, 0)
    assert a.key != b.key and not a.pointwise
    with pytest.raises(ValueError):
        compile_loglik(BODY, ["s"], linear=True, pointwise=True)
    lik = CompiledLikelihood(BODY, params={"s": 1.0})
    assert lik.compiled(pointwise=True).key == b.key and lik.compiled(128, pointwise=True) is lik.compiled(pointwise=True)


@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_point(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    if not os.path.exists(path):
        pytest.skip(f"{so} has not been built")
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    assert " pgb_pointwise_loglik\n" in syms


def test_the_abi_header_is_untouched():
    """The entry point lives in include/pgbart_pointwise.h: pgbart.h -- what every backend exports in full -- is the
    parent's, byte for byte.  (Re-pinned once since: its Limits comment now names the tests that hold the two limits on
    tree size; no declaration moved.  And a second time: the Limits comment states what covariates, regressed columns
    and range_exp the sampler takes, and the tests that hold it; again no declaration moved.)"""
    with open(os.path.join(ROOT, "include", "pgbart.h"), "rb") as fh:
        assert hashlib.sha256(fh.read()).hexdigest() == "c717cc477d8b58a9b629b90f5938de4e47493707fb3438ea98ef8c73f5b2a211"
    from pymc_bart_amd import _abi

    assert "pgb_pointwise_loglik" not in _abi.SYMBOLS
