"""PSIS-weighted expectations on the build box (no GPU): ``pgb_psis_row_expect`` of ``include/pgbart_psis.h``
(``tests/_psis_expect_host.py``) -- its first two outputs pinned to ``pgb_psis_row``'s bits, the exact identities of
the self-normalised sum, and the NumPy / SciPy restatement (``tests/_psis_expect_numpy.py``) on synthetic matrices; and
the host-side validation of ``pymc_bart_amd.loo``'s new entries.

The tolerance is measured, not chosen: ``profiles/psis_expect_accuracy.json`` (``tools/psis_expect_accuracy.py``) holds
the largest difference per kind, header against NumPy, relative to max(1, |E|); the bound is 8 x that figure, as in
``tests/test_psis.py``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import stats

import _psis_expect_host as host
import _psis_expect_numpy as ref
import _psis_host as psis_host
import _psis_numpy as psis_ref
from pymc_bart_amd import (CallbackLikelihood, CompiledLikelihood, NormalLikelihood, _abi, compiled, loo_pit, loo_predictive,
                           psis_expectation_matrix)

loo_mod = sys.modules["pymc_bart_amd.loo"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = os.path.join(ROOT, "profiles", "psis_expect_accuracy.json")
SIZES = (400, 1000, 4000)


def synthetic(D: int, n: int = 400) -> np.ndarray:
    """``tests/test_psis.py``'s generator, restated: Normal log densities of n observations (five of them outliers)
    under D draws of (mu, sigma)."""
    rng = np.random.default_rng(0)
    y = rng.normal(0, 1, n)
    y[:5] *= 6
    mu = rng.normal(0, .15, (D, 1)) + rng.normal(0, .1, (D, n))
    sigma = np.exp(rng.normal(0, .1, (D, 1)))
    return stats.norm.logpdf(y[None, :], mu, sigma)


def functionals(D: int, n: int = 400):
    """The second matrices held against the synthetic ll: Normal draws (with their y), Poisson draws (ties with the
    integer y)."""
    rng = np.random.default_rng(100 + D)
    return {"normal": (rng.normal(0.3, 1.2, (D, n)), rng.normal(0.3, 1.2, n)),
            "poisson": (rng.poisson(3.0, (D, n)).astype(float), rng.poisson(3.0, n).astype(float))}


_CACHE = {}


def case(D: int):
    """(ll, M, pgb_psis_row's outputs, the restated k) of one size, computed once."""
    if D not in _CACHE:
        ll = synthetic(D)
        M = psis_ref.tail_length(D)
        _CACHE[D] = (ll, M, psis_host.psis(ll, M), psis_ref.psis_matrix(ll)[1])
    return _CACHE[D]


def differences(D: int) -> dict:
    """The largest |header - restatement| / max(1, |E|) per kind on the rows with k <= 0.7 or no fit, and the rows
    left out (computed once per size)."""
    if ("diff", D) in _CACHE:
        return _CACHE["diff", D]
    ll, M, _, kr = case(D)
    p, k2 = ref.weights_matrix(ll)
    assert np.array_equal(np.isinf(k2), np.isinf(kr))
    ok = np.isinf(kr) | (kr <= 0.7)
    out = {"value": 0.0, "pit": 0.0, "left_out": int((~ok).sum()), "n": int(ok.size)}
    for name, (g, y) in functionals(D).items():
        for kind in ("value", "pit"):
            got = host.expect(ll, g, M, y=y, kind=kind)[2:]
            want = ref.expect_from_weights(p, g, y, kind)
            d = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            out[kind] = max(out[kind], float(d[:, ok].max()))
    _CACHE["diff", D] = out
    return out


def bounds() -> dict:
    with open(ACCURACY) as fh:
        fig = json.load(fh)
    return {kind: 8.0 * float(fig["max_rel_diff"][kind]) for kind in ("value", "pit")}


def bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ------------------------------------------------------------------ 1. pinned bits
@pytest.mark.parametrize("D", SIZES)
def test_the_first_two_outputs_are_pgb_psis_rows_bits(D):
    ll, M, (e, k), _ = case(D)
    for name, (g, y) in functionals(D).items():
        for kind in ("value", "pit"):
            out = host.expect(ll, g, M, y=y, kind=kind)
            assert out.shape == (4 if kind == "value" else 3, ll.shape[1])
            assert bits(out[0], e) and bits(out[1], k), (name, kind)


def _edge_matrices():
    rng = np.random.default_rng(7)
    out = {"three distinct values": np.log(rng.choice([.2, .5, .9], (1000, 12))), "small": rng.normal(-1.0, 0.7, (25, 16)),
           "two draws": rng.normal(-1.0, 0.7, (2, 9)), "constant": np.full((300, 5), -1.25)}
    ll = rng.normal(-1.0, 0.5, (600, 9))
    for c in range(9):
        rows = rng.permutation(600)
        if c % 3 == 0:
            ll[rows[:1 + c % 7], c] = -2047.0
        elif c % 3 == 1:
            ll[rows[:3], c] = 2047.0
        else:
            ll[rows[:8], c] = -2047.0 + np.arange(8) * 3.0
            ll[rows[8:11], c] = 2047.0
    out["clamp values"] = ll
    return out


def test_pinned_bits_and_exact_identities_on_every_matrix():
    mats = {f"synthetic {D}": case(D)[0][:, :60] for D in SIZES}
    mats.update(_edge_matrices())
    for what, ll in mats.items():
        D, n = ll.shape
        M = psis_ref.tail_length(D)
        e, k = psis_host.psis(ll, M)
        rng = np.random.default_rng(D)
        g = rng.normal(0.0, 2.0, (D, n))
        hi, lo = np.full(n, g.max() + 1.0), np.full(n, g.min() - 1.0)
        for out in (host.expect(ll, g, M), host.expect(ll, g, M, y=hi, kind="pit")):
            assert bits(out[0], e) and bits(out[1], k), what
        # a constant functional comes back exactly: numerator and denominator are the same sums
        one = host.expect(ll, np.ones((D, n)), M)
        assert np.all(one[2] == 1.0) and np.all(one[3] == 1.0), what
        two = host.expect(ll, np.full((D, n), 2.0), M)
        assert np.all(two[2] == 2.0) and np.all(two[3] == 4.0), what
        assert np.all(host.expect(ll, g, M, y=hi, kind="pit")[2] == 1.0), what      # y above every g
        assert np.all(host.expect(ll, g, M, y=lo, kind="pit")[2] == 0.0), what      # y below every g
        yy = rng.normal(0.0, 1.0, n)
        assert np.all(host.expect(ll, np.tile(yy, (D, 1)), M, y=yy, kind="pit")[2] == 0.5), what   # g == y
        # +-1e200 behaves as +-1e150
        big = g.copy()
        big[::3] = 1e200
        big[1::3] = -1e200
        assert bits(host.expect(ll, big, M), host.expect(ll, np.clip(big, -1e150, 1e150), M)), what
        assert np.all(np.isfinite(host.expect(ll, big, M)[2:])), what
    assert host.g_max() == 1e150 == loo_mod.G_MAX


def _lane_sum(t: np.ndarray) -> float:
    """The header's LANE SUM: 64 partials by index mod 64, each in ascending order, then added in lane order."""
    part = np.zeros(64)
    for d, v in enumerate(t):
        part[d % 64] = part[d % 64] + v
    s = 0.0
    for v in part:
        s = s + v
    return s


@pytest.mark.parametrize("D", [25, 300, 1003])
def test_a_column_of_constant_ll_has_unit_weights(D):
    rng = np.random.default_rng(D)
    ll = np.full((D, 6), -0.75)
    M = psis_ref.tail_length(D)
    g = rng.poisson(3.0, (D, 6)).astype(float)
    y = np.array([0.0, 2.0, 3.0, 3.0, 5.0, 40.0])
    pit = host.expect(ll, g, M, y=y, kind="pit")
    assert np.all(np.isinf(pit[1]))                               # T = 0: no fit, every weight 1
    assert np.array_equal(pit[2], ((g < y).sum(axis=0) + 0.5 * (g == y).sum(axis=0)) / D)
    gv = rng.normal(1.0, 3.0, (D, 6))
    val = host.expect(ll, gv, M)
    for c in range(6):
        assert val[2, c] == _lane_sum(gv[:, c]) / D and val[3, c] == _lane_sum(gv[:, c] * gv[:, c]) / D


# ------------------------------------------------------------------ 2. against the NumPy restatement
@pytest.mark.parametrize("D", SIZES)
def test_header_against_the_numpy_restatement(D):
    d = differences(D)
    b = bounds()
    print(f"D = {D}: {d['left_out']} of {d['n']} rows left out, max rel |d| value = {d['value']:.3e} (bound "
          f"{b['value']:.3e}), pit = {d['pit']:.3e} (bound {b['pit']:.3e})")
    assert d["left_out"] <= 0.02 * d["n"]
    assert d["value"] <= b["value"] and d["pit"] <= b["pit"]


def test_the_committed_accuracy_figure_is_the_measured_one():
    with open(ACCURACY) as fh:
        fig = json.load(fh)["max_rel_diff"]
    worst = {"value": 0.0, "pit": 0.0}
    for D in SIZES:
        d = differences(D)
        for kind in worst:
            worst[kind] = max(worst[kind], d[kind])
    for kind in worst:
        print(f"{kind}: measured {worst[kind]:.3e}, committed {fig[kind]:.3e}")
        assert worst[kind] <= 8.0 * fig[kind] and fig[kind] <= 8.0 * worst[kind]   # (libm may differ by a few ulp)


# ------------------------------------------------------------------ 3. host-side validation
def test_argument_errors_are_raised_before_a_backend_is_touched():
    from test_pointwise import _sampler

    X, y = np.zeros((8, 2)), np.zeros(8)
    lik = NormalLikelihood(1.0)
    s = _sampler()
    for fn in (loo_pit, lambda *a, **kw: loo_predictive(*a, kind="y", **kw)):
        with pytest.raises(ValueError, match="callback family has a log density only, no sampler"):
            fn(s, X, y, CallbackLikelihood(lambda yy, mu: -(yy - mu) ** 2))
        with pytest.raises(ValueError, match="compiled family has a log density only, no sampler"):
            fn(s, X, y, CompiledLikelihood("return -0.5 * (y - mu) * (y - mu);"))
        with pytest.raises(ValueError, match="random_seed"):
            fn(s, X, y, lik, random_seed=-1)
        with pytest.raises(ValueError, match="domain"):
            fn(s, X, y, NormalLikelihood(-1.0))
    for fn in (loo_pit, loo_predictive):
        with pytest.raises(ValueError, match="at least 2 draws"):
            fn(s, X, y, lik, draws=[3])
        with pytest.raises(ValueError, match="shape"):
            fn(s, X, np.zeros(7), lik)
        with pytest.raises(ValueError, match="offset must have shape"):
            fn(s, X, y, lik, offset=np.zeros((2, 8)))
        with pytest.raises(ValueError, match="reff"):
            fn(s, X, y, lik, reff=0.0)
        with pytest.raises(AttributeError):                 # a call that passes every check reaches the backend (none)
            fn(s, X, y, lik)
    with pytest.raises(ValueError, match="callback"):        # (the linear predictor needs no sampler, but a density)
        loo_predictive(s, X, y, CallbackLikelihood(lambda yy, mu: -(yy - mu) ** 2))
    with pytest.raises(ValueError, match="kind must be 'mu' or 'y'"):
        loo_predictive(s, X, y, lik, kind="pit")
    ll, g = np.zeros((10, 4)), np.zeros((10, 4))
    with pytest.raises(ValueError, match="matrix"):
        psis_expectation_matrix(np.zeros(10), np.zeros(10))
    with pytest.raises(ValueError, match="g must have ll's shape"):
        psis_expectation_matrix(ll, np.zeros((10, 5)))
    with pytest.raises(ValueError, match="kind must be 'value' or 'pit'"):
        psis_expectation_matrix(ll, g, kind="mean")
    with pytest.raises(ValueError, match="at least 2 draws"):
        psis_expectation_matrix(np.zeros((1, 4)), np.zeros((1, 4)))
    with pytest.raises(ValueError, match="reff"):
        psis_expectation_matrix(ll, g, reff=1.5)
    with pytest.raises(ValueError, match="ll must be finite"):
        psis_expectation_matrix(np.full((10, 4), np.inf), g)
    with pytest.raises(ValueError, match="NaN"):
        psis_expectation_matrix(ll, np.full((10, 4), np.nan))
    with pytest.raises(ValueError, match="needs the observed y"):
        psis_expectation_matrix(ll, g, kind="pit")
    with pytest.raises(ValueError, match="one value per row"):
        psis_expectation_matrix(ll, g, y=np.zeros(3), kind="pit")
    with pytest.raises(ValueError, match="y must be finite"):
        psis_expectation_matrix(ll, g, y=np.full(4, np.inf), kind="pit")
    assert loo_mod.KINDS == host.KINDS


def test_a_backend_that_is_not_hip_is_refused():
    from _oracle import oracle_backend

    with pytest.raises(_abi.PGBError, match="HIP backend only"):
        psis_expectation_matrix(np.zeros((10, 4)), np.zeros((10, 4)), backend=oracle_backend())
    with pytest.raises(_abi.PGBError, match="HIP backend only"):
        psis_expectation_matrix(np.zeros((10, 4)), np.zeros((10, 4)), y=np.zeros(4), kind="pit", backend=oracle_backend())


@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_point(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    if not os.path.exists(path):
        pytest.skip(f"{so} has not been built")
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    for name in ("pgb_psis_expect", "pgb_add_offset"):
        assert f" {name}\n" in syms and name not in _abi.SYMBOLS
