"""PSIS-LOO on the build box (no GPU): the numeric contract of ``include/pgbart_psis.h`` (``tests/_psis_host.py``)
against the algorithm restated with NumPy / SciPy libm (``tests/_psis_numpy.py``), on synthetic matrices and on the
edge cases of the tail; and the host-side validation of ``pymc_bart_amd.loo``.

The tolerance is measured, not chosen: ``profiles/psis_accuracy.json`` (``tools/psis_accuracy.py``) holds the largest
absolute difference, header against NumPy, over ``pareto_k_i`` and ``elpd_loo_i`` on the synthetic matrices below; the
bound is 8 x that figure (the accumulated table exp / log error over up to D + M m_est terms moves with the inputs)."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
from scipy import stats
from scipy.special import logsumexp

import _psis_host as host
import _psis_numpy as ref
from pymc_bart_amd import CallbackLikelihood, NormalLikelihood, _abi, compiled
from pymc_bart_amd.loo import loo, psis_loo_matrix

loo_mod = sys.modules["pymc_bart_amd.loo"]  # (the package exports the function under the module's name)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = os.path.join(ROOT, "profiles", "psis_accuracy.json")


def bound() -> float:
    with open(ACCURACY) as fh:
        return 8.0 * float(json.load(fh)["max_abs_diff"])


def synthetic(D: int, n: int = 400) -> np.ndarray:
    """Normal log densities of n observations (five of them outliers) under D draws of (mu, sigma)."""
    rng = np.random.default_rng(0)
    y = rng.normal(0, 1, n)
    y[:5] *= 6
    mu = rng.normal(0, .15, (D, 1)) + rng.normal(0, .1, (D, n))
    sigma = np.exp(rng.normal(0, .1, (D, 1)))
    return stats.norm.logpdf(y[None, :], mu, sigma)


def compare(ll, reff=1.0, what=""):
    """Header against restatement on the rows PSIS itself trusts (k <= 0.7) and on those without a fit (k = inf, the
    plain importance-sampling value); -> (header elpd, header k, restated k, restated T, rows compared)."""
    M = ref.tail_length(ll.shape[0], reff)
    assert M == loo_mod.tail_length(ll.shape[0], reff)
    e, k = host.psis(ll, M)
    er, kr, T = ref.psis_matrix(ll, reff)
    nofit = np.isinf(kr)
    assert np.array_equal(np.isinf(k), nofit) and np.all(k[nofit] > 0), what
    ok = nofit | (kr <= 0.7)
    fin = ok & ~nofit
    dk = float(np.max(np.abs(k[fin] - kr[fin]))) if fin.any() else 0.0
    de = float(np.max(np.abs(e[ok] - er[ok]))) if ok.any() else 0.0
    print(f"{what}: D = {ll.shape[0]}, M = {M}, {int((~ok).sum())} of {ok.size} rows left out, max |dk| = {dk:.3e}, "
          f"max |d elpd| = {de:.3e} (bound {bound():.3e})")
    assert dk <= bound() and de <= bound(), what
    return e, k, kr, T, ok


# ------------------------------------------------------------------ 1. synthetic matrices
@pytest.mark.parametrize("D", [400, 1000, 4000])
def test_header_against_the_numpy_restatement(D):
    ll = synthetic(D)
    e, k, kr, T, ok = compare(ll, what="synthetic")
    assert int((~ok).sum()) <= 0.02 * ok.size              # the k <= 0.7 filter leaves out at most 2 % of the rows
    assert np.all(np.isfinite(k)) and np.all(np.isfinite(kr)) and np.all(T == ref.tail_length(D))
    assert np.all(np.isfinite(e))


def test_the_committed_accuracy_figure_is_the_measured_one():
    fig = json.load(open(ACCURACY))
    worst = 0.0
    for D in (400, 1000, 4000):
        ll = synthetic(D)
        M = ref.tail_length(D)
        e, k = host.psis(ll, M)
        er, kr, _ = ref.psis_matrix(ll)
        ok = kr <= 0.7
        worst = max(worst, float(np.max(np.abs(k - kr)[ok])), float(np.max(np.abs(e - er)[ok])))
    print(f"measured {worst:.3e}, committed {fig['max_abs_diff']:.3e}")
    assert worst <= 8.0 * fig["max_abs_diff"] and fig["max_abs_diff"] <= 8.0 * worst   # (libm may differ by a few ulp)


# ------------------------------------------------------------------ 2. edge cases of the tail
def test_few_distinct_values_have_no_tail():
    rng = np.random.default_rng(1)
    ll = np.log(rng.choice([.2, .5, .9], (1000, 40)))
    e, k, kr, T, ok = compare(ll, what="three distinct values")
    assert np.all(T == 0) and np.all(np.isinf(k)) and ok.all()
    plain = np.log(ll.shape[0]) - logsumexp(-ll, axis=0)   # the unsmoothed importance-sampling value
    assert np.max(np.abs(e - plain)) <= bound()


def _tied(rng, D, n_tail, n_cols=12):
    """Columns whose n_tail smallest values are distinct and whose next D / 2 values are one number."""
    ll = rng.normal(-1.0, 0.3, (D, n_cols))
    for c in range(n_cols):
        order = rng.permutation(D)
        ll[order[:D // 2], c] = -2.5
        ll[order[D // 2:D // 2 + n_tail], c] = -2.5 - rng.uniform(0.2, 3.0, n_tail)
    return ll


def test_a_tail_of_exactly_five_is_fitted_and_one_of_four_is_not():
    rng = np.random.default_rng(2)
    e, k, kr, T, ok = compare(_tied(rng, 1000, 5), what="five above the ties")
    assert np.all(T == 5) and np.all(np.isfinite(k))
    e, k, kr, T, ok = compare(_tied(rng, 1000, 4), what="four above the ties")
    assert np.all(T == 4) and np.all(np.isinf(k))


@pytest.mark.parametrize("D", [2, 25])
def test_the_smallest_matrices(D):
    rng = np.random.default_rng(3)
    ll = rng.normal(-1.0, 0.7, (D, 64))
    e, k, kr, T, ok = compare(ll, what="small D")
    assert np.all(T == ref.tail_length(D)) and np.all(np.isfinite(e))
    assert np.all(np.isinf(k)) if D == 2 else np.all(np.isfinite(k))


def test_columns_with_the_clamp_values():
    rng = np.random.default_rng(4)
    D = 600
    ll = rng.normal(-1.0, 0.5, (D, 30))
    for c in range(30):
        rows = rng.permutation(D)
        if c % 3 == 0:
            ll[rows[:1 + c % 7], c] = -2047.0              # draws that cannot explain the row at all: the floored cutoff
        elif c % 3 == 1:
            ll[rows[:3], c] = 2047.0
        else:
            ll[rows[:8], c] = -2047.0 + np.arange(8) * 3.0  # more than four beyond the floor: fitted
            ll[rows[8:11], c] = 2047.0
    ll[:, 29] = -2047.0                                      # every value the lower bound
    e, k, kr, T, ok = compare(ll, what="clamp values")
    assert np.all(np.isfinite(e)) and np.all(T[2::3][:9] == 8)


def test_a_column_with_a_negative_k():
    rng = np.random.default_rng(5)
    ll = -0.5 * rng.uniform(0.0, 1.0, (2000, 16))           # bounded importance ratios: a short tail
    e, k, kr, T, ok = compare(ll, what="bounded ratios")
    assert ok.all() and np.all(k < 0.0)


def test_reff_lengthens_the_tail():
    ll = synthetic(1000, n=50)
    assert ref.tail_length(1000, 0.25) == 190 and loo_mod.tail_length(1000, 0.25) == 190
    compare(ll, reff=0.25, what="reff = 0.25")


def test_the_helpers_where_libm_would_be_safe():
    L = host.lib()
    x = -np.concatenate([10.0 ** np.arange(-300.0, 0.0, 7.3), np.linspace(1e-3, 0.9995, 400)])
    got = np.array([L.psis_log1p(v) for v in x])
    assert np.max(np.abs(got / np.log1p(x) - 1.0)) < 1e-15
    yv = np.concatenate([-x, x, np.linspace(-40, 40, 801)])
    yv = yv[yv != 0.0]
    got = np.array([L.psis_expm1(v) for v in yv])
    assert np.max(np.abs(got / np.expm1(yv) - 1.0)) < 2e-15
    q = np.array([m / (j - 0.5) for m in range(32, 52) for j in range(1, m + 1)])
    got = np.array([L.psis_sqrt(v) for v in q])
    assert np.max(np.abs(got / np.sqrt(q) - 1.0)) <= 2.0 ** -52


# ------------------------------------------------------------------ 3. host-side validation
def test_argument_errors_are_raised_before_a_backend_is_touched():
    from test_pointwise import _sampler

    X, y = np.zeros((8, 2)), np.zeros(8)
    lik = NormalLikelihood(1.0)
    s = _sampler()
    with pytest.raises(ValueError, match="callback"):
        loo(s, X, y, CallbackLikelihood(lambda yy, mu: -(yy - mu) ** 2))
    with pytest.raises(ValueError, match="at least 2 draws"):
        loo(_sampler(draws=1), X, y, lik)
    with pytest.raises(ValueError, match="at least 2 draws"):
        loo(s, X, y, lik, draws=[3])
    with pytest.raises(ValueError, match="shape"):
        loo(s, X, np.zeros(7), lik)
    with pytest.raises(ValueError, match="offset must have shape"):
        loo(s, X, y, lik, offset=np.zeros((2, 8)))
    for bad in (0.0, -0.5, 1.5, np.nan):
        with pytest.raises(ValueError, match="reff"):
            loo(s, X, y, lik, reff=bad)
        with pytest.raises(ValueError, match="reff"):
            psis_loo_matrix(np.zeros((10, 4)), reff=bad)
    with pytest.raises(AttributeError):                     # a call that passes every check reaches the backend (none)
        loo(s, X, y, lik)
    with pytest.raises(ValueError, match="matrix"):
        psis_loo_matrix(np.zeros(10))
    with pytest.raises(ValueError, match="at least 2 draws"):
        psis_loo_matrix(np.zeros((1, 4)))
    with pytest.raises(ValueError, match="finite"):
        psis_loo_matrix(np.full((10, 4), np.nan))
    with pytest.raises(ValueError, match="at most"):
        psis_loo_matrix(np.zeros((loo_mod.MAX_DRAWS + 1, 1)))
    with pytest.raises(ValueError, match="tail"):
        psis_loo_matrix(np.zeros((8000, 1)), reff=0.05)
    assert loo_mod.MAX_DRAWS == host.max_draws() and loo_mod.MAX_TAIL == host.max_tail()
    assert loo_mod.MAX_DRAWS >= 8000 and loo_mod.tail_length(loo_mod.MAX_DRAWS) <= loo_mod.MAX_TAIL
    assert loo_mod.khat_threshold(4000) == 0.7 and loo_mod.khat_threshold(100) == 0.5


def test_a_backend_that_is_not_hip_is_refused():
    from _oracle import oracle_backend

    with pytest.raises(_abi.PGBError, match="HIP backend only"):
        psis_loo_matrix(np.zeros((10, 4)), backend=oracle_backend())


def test_the_result_names_the_untrusted_rows():
    e, k = np.array([-1.0, -2.0, -4.0]), np.array([0.1, 0.9, np.inf])
    with pytest.warns(UserWarning, match=r"2 of 3 rows have a Pareto k above 0\.700"):
        r = loo_mod._result(e, k, 4000, 190, 0, lppd_i=np.array([-0.9, -1.5, -3.0]))
    assert r["n_high_k"] == 2 and r["elpd_loo"] == -7.0 and r["p_loo"] == pytest.approx(1.6)
    assert r["se_elpd_loo"] == pytest.approx(np.sqrt(3 * e.var())) and r["tail_len"] == 190 and r["n_draws"] == 4000
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = loo_mod._result(e, np.array([0.1, 0.2, 0.69]), 4000, 190, 3)
    assert r["n_high_k"] == 0 and r["n_clamped"] == 3 and "lppd_i" not in r


@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_point(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    if not os.path.exists(path):
        pytest.skip(f"{so} has not been built")
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    assert " pgb_psis_rows\n" in syms and "pgb_psis_rows" not in _abi.SYMBOLS
