"""Replicated observations (``include/pgbart_ppc.h``) on the host: the distribution of every family's sampler against
SciPy within the Dvoretzky-Kiefer-Wolfowitz bound, the addressing of the random numbers, the caps, the PIT counts, and
the Python surface's refusals (no backend touched).

The DKW bound: for N independent values of ANY law (discrete ones included) the empirical CDF lies within
``eps = sqrt(ln(2 / alpha) / (2 N))`` of the true one with probability 1 - alpha.  alpha = 1e-9 and N = 2^18 give
eps = 0.00639: derived, not tuned -- a correct sampler fails a case with probability 1e-9.  NumPy's own samplers sit at
0.0005 .. 0.002 on these cases; a Poisson sampler that is off by one at rate 1000 sits at 0.0125."""
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import stats

import _ppc_host as host
from pymc_bart_amd import (CallbackLikelihood, CategoricalLikelihood, NormalLikelihood, PoissonLikelihood, _abi, compiled,
                           posterior_predictive, predictive_pit, predictive_summary)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DD = NN = 512
N = DD * NN                                               # 2^18
ALPHA = 1e-9
EPS = math.sqrt(math.log(2.0 / ALPHA) / (2.0 * N))        # 0.006391
Z = float(stats.norm.isf(ALPHA / 2.0))                    # 6.11: the same alpha, two-sided normal


def test_the_bound_is_what_the_derivation_says():
    assert N == 1 << 18 and abs(EPS - 0.00639) < 1e-5 and abs(Z - 6.11) < 5e-3


def draw(family, mu, params=(), **kw):
    x, _, flags = host.constant(family, mu, DD, NN, params, **kw)
    assert flags == (0, 0), (family, mu, params, flags)
    assert np.all(np.isfinite(x))
    return x.ravel()


def ks_continuous(x, cdf) -> float:
    x = np.sort(x)
    F = cdf(x)
    i = np.arange(x.size)
    return float(max(np.max((i + 1) / x.size - F), np.max(F - i / x.size)))


def ks_discrete(x, cdf) -> float:
    """sup |F_n - F| of an integer law: at every observed support point and just below it (between two of them F_n is
    flat and F grows, so the largest gap there is the one just below the next)."""
    v, cnt = np.unique(x, return_counts=True)
    assert np.all(v == np.floor(v)) and v[0] >= 0
    cum = np.cumsum(cnt) / x.size
    return float(max(np.max(np.abs(cum - cdf(v))), np.max(np.abs((cum - cnt / x.size) - cdf(v - 1.0)))))


# ------------------------------------------------------------------ 1. distributions
@pytest.mark.parametrize("sigma", [0.1, 3.0])
def test_normal(sigma):
    assert ks_continuous(draw("normal", 0.7, [sigma]), stats.norm(0.7, sigma).cdf) <= EPS


@pytest.mark.parametrize("mu1, sd", [(-2.0, 2.0), (3e-9, 1e-8), (-1e-12, 1e-8)])
def test_normal_meanscale(mu1, sd):
    assert ks_continuous(draw("normal_meanscale", [0.3, mu1]), stats.norm(0.3, sd).cdf) <= EPS


@pytest.mark.parametrize("link", ["probit", "logit"])
@pytest.mark.parametrize("mu", [-8.0, -1.0, 0.0, 2.0, 8.0])
def test_bernoulli(link, mu):
    x = draw("bernoulli_" + link, mu)
    assert set(np.unique(x)) <= {0.0, 1.0}
    p = stats.norm.cdf(mu) if link == "probit" else 1.0 / (1.0 + math.exp(-mu))
    assert abs(x.mean() - p) <= EPS


@pytest.mark.parametrize("K", [2, 3, 16])
def test_categorical(K):
    mu = np.random.default_rng(K).normal(0.0, 1.5, K)
    mu[(int(np.argmax(mu)) + 1) % K] = mu.max() - 40.0           # one class 40 below the maximum
    x = draw("categorical", mu)
    assert set(np.unique(x)) <= set(float(k) for k in range(K))
    p = np.exp(mu - mu.max())
    p /= p.sum()
    freq = np.bincount(x.astype(int), minlength=K) / x.size
    assert np.max(np.abs(np.cumsum(freq) - np.cumsum(p))) <= EPS
    assert freq[int(np.argmin(mu))] == 0.0                       # e^-40 of 2^18 values


@pytest.mark.parametrize("q", [0.1, 0.5, 0.9])
def test_asymmetric_laplace(q):
    b, mu = 1.7, -0.4
    kappa = math.sqrt(q / (1.0 - q))                             # SciPy's parametrisation of the Yu-Moyeed law
    ref = stats.laplace_asymmetric(kappa, loc=mu, scale=b / math.sqrt(q * (1.0 - q)))
    assert abs(ref.cdf(mu) - q) < 1e-12                          # (mu is the q-quantile)
    assert ks_continuous(draw("asymmetric_laplace", mu, [b, q]), ref.cdf) <= EPS


@pytest.mark.parametrize("nu", [1.5, 5.0, 30.0])
def test_student_t(nu):
    assert ks_continuous(draw("student_t", 1.2, [0.8, nu]), stats.t(nu, 1.2, 0.8).cdf) <= EPS


@pytest.mark.parametrize("alpha", [0.05, 0.3, 1.0, 2.5, 50.0])
def test_gamma(alpha):
    mu = 0.9
    assert ks_continuous(draw("gamma_log", mu, [alpha]), stats.gamma(alpha, scale=math.exp(mu) / alpha).cdf) <= EPS


def _rates():
    s = host.poisson_switch()
    return [0.5, 1000.0, s * (1.0 - 1e-6), s, s * (1.0 + 1e-6)]


@pytest.mark.parametrize("which", range(5))
def test_poisson(which):
    rate = _rates()[which]
    assert ks_discrete(draw("poisson_log", math.log(rate)), stats.poisson(rate).cdf) <= EPS


def test_poisson_at_a_large_rate():
    lam = 1.0e6
    x = draw("poisson_log", math.log(lam))
    assert ks_discrete(x, stats.poisson(lam).cdf) <= EPS
    assert abs(x.mean() - lam) <= Z * math.sqrt(lam / N)


@pytest.mark.parametrize("alpha, mean", [(0.5, 3.0), (0.5, 200.0), (5.0, 200.0)])
def test_negative_binomial(alpha, mean):
    ref = stats.nbinom(alpha, alpha / (alpha + mean))
    assert ks_discrete(draw("negbin_log", math.log(mean), [alpha]), ref.cdf) <= EPS


# ------------------------------------------------------------------ 2. addressing
@pytest.mark.parametrize("family, K, params", [("normal", 1, [0.5]), ("negbin_log", 1, [0.7]), ("categorical", 3, [])])
def test_a_block_of_rows_is_the_same_rows_of_the_whole(family, K, params):
    rng = np.random.default_rng(5)
    D, n = 7, 300
    mu = rng.normal(1.0, 1.0, (D, K, n))
    par = np.tile(np.asarray(params, np.float64), (D, 1))
    for base in (0, (1 << 32) + 5):
        whole, _, _ = host.fill(family, mu, par, row0=base, seed=11)
        for r0, r1 in ((0, 64), (64, 65), (65, 300), (17, 211)):
            part, _, _ = host.fill(family, mu[:, :, r0:r1], par, row0=base + r0, seed=11)
            assert np.array_equal(part.view(np.uint64), whole[:, r0:r1].view(np.uint64)), (base, r0, r1)
    low, _, _ = host.fill(family, mu, par, row0=5, seed=11)
    high, _, _ = host.fill(family, mu, par, row0=(1 << 32) + 5, seed=11)
    assert not np.array_equal(low, high)                          # the high word of the row is part of the address


def test_seeds_differ_and_no_value_repeats():
    a = draw("normal", 0.0, [1.0], seed=1)
    b = draw("normal", 0.0, [1.0], seed=2)
    c = draw("normal", 0.0, [1.0], seed=1 << 32)                  # (the high word of the seed is part of the key)
    assert not np.any(a == b) and not np.any(a == c)
    assert np.unique(a).size == N
    assert np.array_equal(a, draw("normal", 0.0, [1.0], seed=1))


def test_neighbours_are_uncorrelated():
    x = draw("normal", 0.0, [1.0], seed=3).reshape(DD, NN)
    for a, b in ((x[:, :-1], x[:, 1:]), (x[:-1, :], x[1:, :])):   # along the rows, along the draws
        r = float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
        assert abs(r) <= Z / math.sqrt(a.size), r


def test_the_purposes_are_not_the_samplers():
    mine, samplers = host.purposes()
    assert len(mine) >= 5 and len(samplers) == 6 and not set(mine) & set(samplers)


# ------------------------------------------------------------------ 3. caps
def test_one_attempt_exhausts_and_stays_finite():
    for family, mu, params in (("gamma_log", 0.3, [0.3]), ("poisson_log", math.log(50.0), [])):
        x, _, (capped, exhausted) = host.constant(family, mu, 64, 256, params, max_tries=1)
        assert exhausted > 0 and capped == 0 and np.all(np.isfinite(x)), family
        assert exhausted < x.size // 2                              # (most first attempts are accepted)
        _, _, flags = host.constant(family, mu, 64, 256, params)
        assert flags == (0, 0), family


def test_a_rate_beyond_the_cap_is_capped_and_counted():
    assert host.max_rate() == 2.0 ** 30 and math.exp(25.0) > host.max_rate()
    x, _, (capped, exhausted) = host.constant("poisson_log", 25.0, 16, 256)
    assert capped == x.size and exhausted == 0
    assert np.all(np.abs(x - 2.0 ** 30) <= 7.0 * 2.0 ** 15)        # 7 standard deviations of Poisson(2^30)
    x, _, (capped, _) = host.constant("gamma_log", 800.0, 4, 64, [2.0])
    assert capped == x.size and np.all(x == 1.7976931348623157e308)


# ------------------------------------------------------------------ 4. PIT counts
@pytest.mark.parametrize("family, params", [("poisson_log", []), ("student_t", [0.5, 4.0])])
def test_pit_counts_are_numpys(family, params):
    rng = np.random.default_rng(9)
    D, n = 65, 257
    mu = rng.normal(1.0, 0.3, (D, 1, n))
    par = np.tile(np.asarray(params, np.float64), (D, 1))
    yrep, _, _ = host.fill(family, mu, par, row0=3, seed=4)
    y = yrep[rng.integers(0, D, n), np.arange(n)] if family == "poisson_log" else rng.normal(1.0, 1.0, n)
    same, pit, _ = host.fill(family, mu, par, row0=3, seed=4, y=y)
    assert np.array_equal(same, yrep)
    assert np.array_equal(pit[0], (yrep < y).sum(0)) and np.array_equal(pit[1], (yrep == y).sum(0))
    if family == "poisson_log":
        assert np.all(pit[1] >= 1) and np.any(pit[1] > 5)          # ties
    else:
        assert not np.any(pit[1])
    only, pit2, _ = host.fill(family, mu, par, row0=3, seed=4, y=y, values=False)
    assert only is None and np.array_equal(pit2, pit)


# ------------------------------------------------------------------ 5. the Python surface
def _calls():
    return (lambda s, X, lik, **kw: posterior_predictive(s, X, lik, **kw),
            lambda s, X, lik, **kw: predictive_summary(s, X, lik, **kw),
            lambda s, X, lik, **kw: predictive_pit(s, X, np.zeros(np.shape(X)[0]), lik, **kw))


@pytest.mark.parametrize("which", range(3))
def test_argument_errors_are_raised_before_a_backend_is_touched(which):
    from test_pointwise import _sampler

    class Compiled:                                        # (what the check reads of a CompiledLikelihood)
        family, n_outputs, param_names = "compiled", 1, []

    fn = _calls()[which]
    s = _sampler(draws=5)
    X = np.zeros((8, 2))
    lik = NormalLikelihood(1.0)
    with pytest.raises(ValueError, match="the callback family has a log density only, no sampler"):
        fn(s, X, CallbackLikelihood(lambda y, mu: -(y - mu) ** 2))
    with pytest.raises(ValueError, match="the compiled family has a log density only, no sampler"):
        fn(s, X, Compiled())
    with pytest.raises(ValueError, match="n_outputs = 3"):
        fn(s, X, CategoricalLikelihood(3))
    with pytest.raises(ValueError, match="does not take n_outputs = 2"):
        class Two(PoissonLikelihood):
            n_outputs = 2
        fn(_sampler(K=2), X, Two())
    with pytest.raises(ValueError, match=r"one point per draw \(5\), got 4"):
        fn(s, X, NormalLikelihood("sigma"), points=[{"sigma": 1.0}] * 4)
    with pytest.raises(ValueError, match=r"one value per draw \(5\)"):
        fn(s, X, NormalLikelihood("sigma"), points={"sigma": np.ones(4)})
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="the params of draw 3 are outside the normal family's domain"):
            fn(s, X, NormalLikelihood("sigma"), points={"sigma": np.array([1.0, 1.0, 1.0, bad, bad])})
    with pytest.raises(ValueError, match="offset must be finite"):
        fn(s, X, lik, offset=np.where(np.arange(8) == 2, np.nan, 0.0))
    with pytest.raises(ValueError, match="offset must be finite"):
        fn(s, X, lik, offset=np.full(8, np.inf))
    with pytest.raises(ValueError, match="offset must have shape"):
        fn(s, X, lik, offset=np.zeros((2, 8)))
    with pytest.raises(ValueError, match="draws must index the 5 stored draws"):
        fn(s, X, lik, draws=[0, 5])
    with pytest.raises(ValueError, match="draws must index the 5 stored draws"):
        fn(s, X, lik, draws=[-1])
    with pytest.raises(ValueError, match="no draws"):
        fn(s, X, lik, draws=[])
    with pytest.raises(ValueError, match="excluded must index"):
        fn(s, X, lik, excluded=[2])
    with pytest.raises(ValueError, match="matrix"):
        fn(s, np.zeros((2, 2, 2)), lik)
    with pytest.raises(ValueError, match="random_seed"):
        fn(s, X, lik, random_seed=-1)
    with pytest.raises(TypeError, match="sampler must be"):
        fn(object(), X, lik)
    with pytest.raises(AttributeError):                     # a call that passes every check reaches the backend (none)
        fn(s, X, lik)


def test_more_argument_errors():
    from test_pointwise import _sampler

    s = _sampler(draws=5)
    X = np.zeros((8, 2))
    with pytest.raises(ValueError, match="y must hold one value per row"):
        predictive_pit(s, X, np.zeros(7), NormalLikelihood(1.0))
    with pytest.raises(ValueError, match="y must be finite"):
        predictive_pit(s, X, np.where(np.arange(8) == 3, np.nan, 0.0), NormalLikelihood(1.0))
    with pytest.raises(ValueError, match="at least 2 draws"):
        predictive_summary(s, X, NormalLikelihood(1.0), draws=[2])
    with pytest.raises(ValueError, match=r"quantiles must be in \[0, 1\]"):
        predictive_summary(s, X, NormalLikelihood(1.0), quantiles=[1.5])


@pytest.mark.parametrize("which", range(3))
def test_a_backend_that_is_not_hip_is_refused(which):
    from _oracle import oracle_backend
    from pymc_bart_amd.trees import PosteriorSampler
    from test_pointwise import _sampler

    s = _sampler(draws=5)
    with pytest.raises(_abi.PGBError, match="HIP backend only"):
        _calls()[which](PosteriorSampler(s.pool, s.forest_idx, s.m, 1, backend=oracle_backend()), np.zeros((8, 2)),
                        NormalLikelihood(1.0))


@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_point(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    if not os.path.exists(path):
        pytest.skip(f"{so} has not been built")
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    assert " pgb_ppc_draw\n" in syms and "pgb_ppc_draw" not in _abi.SYMBOLS


UNIT = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "pgbart.h"
#include "pgbart_spec.h"
#include "pgbart_compiled.h"
#include "pgbart_ppc.h"
static thread_local char g_err[512];
static int fail(int code, const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); return code; }
static int fail_hip(hipError_t e, const char* what) { snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e)); return PGB_E_DEVICE; }
#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail_hip(e_, #expr); } while (0)
#include "k_ppc.h"
"""


def test_the_kernel_cross_compiles_for_gfx950_and_is_budgeted(tmp_path):
    """``csrc/k_ppc.h`` with the library's flags for gfx950 (device side; the few host names it takes from the
    translation unit stated above it): two instances, the one-output one without scratch; and the committed occupancy
    budget knows both."""
    import json

    src, out = tmp_path / "unit.hip", tmp_path / "unit.s"
    src.write_text(UNIT)
    r = subprocess.run([compiled.hipcc_path(), *compiled.DEVICE_FLAGS, f"-I{compiled.CSRC}", "--cuda-device-only", "-S",
                        str(src), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    assert asm.count(".amdhsa_kernel ") == 2
    meta = asm[asm.index("amdhsa.kernels"):]
    one = [rec for rec in meta.split("\n  - ") if ".name:           _Z5k_ppcILb1EEv7PpcArgs" in rec]   # one kernel's record
    assert len(one) == 1
    for field in (".private_segment_fixed_size: 0", ".vgpr_spill_count: 0", ".group_segment_fixed_size: 0"):
        assert field in one[0], field
    budget = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    assert budget["k_ppc<true>"]["max_scratch_bytes"] == 0 and budget["k_ppc<true>"]["min_wgs_per_cu"] >= 3
    assert budget["k_ppc<false>"]["min_wgs_per_cu"] >= 2
