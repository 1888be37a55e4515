"""Per-row posterior summaries on the build box (no GPU): the numeric contract of ``include/pgbart_rowsummary.h``
(``tests/_rowsummary_host.py``) against NumPy / SciPy and ``importance.hdi``, the properties the contract promises
(no output depends on the order of the draws, the order is the bit order), the transforms against libm within 8 x the
measured difference (``profiles/rowsummary_accuracy.json``, ``tools/rowsummary_accuracy.py``), the host-side
validation of ``pymc_bart_amd.summary`` and ``partial_dependence(summary=...)``, and the library's export.

Bounds (u = 2^-53, the unit roundoff; M = max |x| of the column):

* order statistics are copies: exact.
* an interpolated quantile ``t_lo + (t_hi - t_lo) * frac`` makes three roundings (the difference, the product, the
  sum), each at most u times a quantity below 2 M: together under 2.5 * 2^-52 M from the exact interpolant at the
  same ``pos``; NumPy's own formula rounds as often.  The bound is 8 * 2^-52 * max(|t_lo|, |t_hi|).
* the mean: a sum of D terms in any order is within (D - 1) u sum|x| <= D (D - 1) u M of the exact sum, the division
  adds one rounding; NumPy's pairwise sum is inside the same bound.  The bound is D * 2^-52 * M on the mean.
* the variance is a two-pass sum.  With delta = D * 2^-52 * M the bound on the computed mean, sum (x - mean')^2 =
  sum (x - mean)^2 + D (mean' - mean)^2 exactly; every term (x - mean')^2 carries three roundings (relative 3 u), the
  sum of D non-negative terms (D - 1) u relative, the division one more: relative (D + 3) u in all, and NumPy's own
  evaluation as much again.  The bound is 2 (D + 3) 2^-53 * var + 2 delta^2 (D / (D - 1) <= 2).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.special import expit, ndtr

import _rowsummary_host as host
from pymc_bart_amd import _abi, compiled, partial_dependence, posterior_summary, summarize_matrix
from pymc_bart_amd.importance import hdi

summary_mod = sys.modules["pymc_bart_amd.summary"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = os.path.join(ROOT, "profiles", "rowsummary_accuracy.json")

DS = (2, 3, 5, 63, 64, 65, 100, 127, 1000, 2049)
EPS = 2.0 ** -52


def cases(D: int, n: int = 6):
    """(name, matrix (D, n)): scales 1e-3, 1, 1e6 x shifts 0, 1e3, and one of integer-rounded values (ties)."""
    rng = np.random.default_rng(1000 + D)
    out = []
    for scale in (1e-3, 1.0, 1e6):
        for shift in (0.0, 1e3):
            out.append((f"scale {scale:g} shift {shift:g}", rng.normal(0.0, 1.0, (D, n)) * scale + shift))
    out.append(("integers", np.round(rng.normal(0.0, 3.0, (D, n)))))
    return out


def transform_inputs() -> np.ndarray:
    rng = np.random.default_rng(5)
    return np.concatenate([np.linspace(-30.0, 30.0, 2401), rng.uniform(-30.0, 30.0, 1600)])


def transform_differences() -> dict:
    """The largest |header / libm - 1| of every transform on x in [-30, 30] (the reference is NumPy / SciPy)."""
    x = transform_inputs()
    refs = {"exp": np.exp(x), "logistic": expit(x), "probit": ndtr(x)}
    return {name: float(np.max(np.abs(host.value(x, name) / ref - 1.0))) for name, ref in refs.items()}


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------ 1. the header against NumPy
@pytest.mark.parametrize("D", DS)
def test_header_against_numpy(D):
    exact_q = [0.0, 1.0] + ([0.5] if D % 2 == 1 else []) + ([0.25] if D % 4 == 1 else [])
    interp_q = [0.03, 0.123, 0.5, 0.75, 0.97]
    q = np.array(exact_q + interp_q)
    worst = {"quantile": 0.0, "mean": 0.0, "var": 0.0}
    for name, x in cases(D):
        n = x.shape[1]
        xs = np.sort(x, axis=0)
        M = np.max(np.abs(x), axis=0)
        for prob in (0.94, 0.5, 1.0):
            k = host.hdi_k(D, prob)
            s = host.summary(x, q, k)
            want = np.array([hdi(x[:, c], prob) for c in range(n)]).T
            assert np.array_equal(s[2 + q.size:], want), (name, prob)
        # order statistics
        assert np.array_equal(s[2], xs[0]) and np.array_equal(s[3], xs[-1]), name
        for j, qq in enumerate(exact_q):
            pos = qq * (D - 1)
            assert pos == int(pos)
            assert np.array_equal(s[2 + j], xs[int(pos)]), (name, qq)
        # interpolated quantiles
        for j, qq in enumerate(interp_q, start=len(exact_q)):
            lo = min(int(qq * (D - 1)), D - 1)
            hi = min(lo + 1, D - 1)
            tol = 8.0 * EPS * np.maximum(np.abs(xs[lo]), np.abs(xs[hi]))
            err = np.abs(s[2 + j] - np.quantile(x, qq, axis=0))
            worst["quantile"] = max(worst["quantile"], float(np.max(err / np.where(tol > 0, tol, 1.0))))
            assert np.all(err <= tol), (name, qq)
        # mean and variance
        delta = D * EPS * M
        err = np.abs(s[0] - np.mean(x, axis=0))
        worst["mean"] = max(worst["mean"], float(np.max(err / delta)))
        assert np.all(err <= delta), name
        ref = np.var(x, axis=0, ddof=1)
        tol = 2.0 * (D + 3) * 2.0 ** -53 * ref + 2.0 * delta ** 2
        err = np.abs(s[1] - ref)
        worst["var"] = max(worst["var"], float(np.max(err / tol)))
        assert np.all(err <= tol), name
    print(f"D = {D}: largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("D", [3, 64, 65, 1000])
def test_permuting_the_draws_changes_no_bit(D):
    rng = np.random.default_rng(7)
    q = np.array([0.0, 0.03, 0.5, 0.97, 1.0])
    for name, x in cases(D)[::3]:
        off = rng.normal(0, 1, x.shape[1])
        for tf in host.TRANSFORMS:
            z = x / np.max(np.abs(x)) * 5.0 if tf != "identity" else x
            a = host.summary(z, q, host.hdi_k(D, 0.9), tf, off)
            b = host.summary(z[rng.permutation(D)], q, host.hdi_k(D, 0.9), tf, off)
            assert np.array_equal(bits(a), bits(b)), (name, tf)


def test_the_order_is_the_bit_order():
    x = np.array([0.0, -0.0, 0.0, -0.0, -0.0, 1.5, -1.5, 0.0])
    t = host.sorted_column(x)
    assert np.array_equal(t, np.sort(x))
    assert np.array_equal(np.signbit(t), [True, True, True, True, False, False, False, False])
    z = np.array([[0.0, 0.0], [-0.0, 0.0], [0.0, 0.0], [-0.0, 0.0]])
    s = host.summary(z, [0.0, 1.0], 2)
    assert np.signbit(s[2, 0]) and not np.signbit(s[3, 0])            # min is -0.0, max +0.0
    assert not np.signbit(s[2, 1]) and not np.signbit(s[3, 1])
    assert np.all(s[0] == 0.0) and np.all(s[1] == 0.0)
    # an offset is added before anything else: -0.0 + 0.0 = +0.0; without one nothing is added
    assert np.signbit(host.sorted_column(np.array([-0.0, -0.0]))).all()
    assert not np.signbit(host.sorted_column(np.array([-0.0, -0.0]), offset=0.0)).any()
    # the keys are a bijection that keeps the order of the values
    v = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, np.inf])
    assert np.array_equal(bits(host.sorted_column(v[::-1].copy())), bits(v))


def test_constant_columns():
    """A constant column: every order statistic and both ends of the HDI are the constant, and the variance is 0
    whenever the D-fold lane sum of the constant is exact (then mean == c) -- dyadic constants below.  For a constant
    such as 0.1 the contract's mean is sum / D like NumPy's, which may differ from c within the mean's bound delta =
    D 2^-52 |c| (module docstring); the variance is then sum (c - mean')^2 / (D - 1) <= 2 delta^2, not 0, and is held
    to that."""
    q = [0.0, 0.3, 0.5, 1.0]
    for D in (2, 3, 64, 65, 1000):
        for c in (2.5, -7.0, 0.0, 1024.0, -0.375):
            s = host.summary(np.full((D, 3), c), q, host.hdi_k(D, 0.94))
            assert np.all(s[0] == c) and np.all(s[1] == 0.0) and np.all(s[2:] == c), (D, c)
        s = host.summary(np.full((D, 3), 0.1), q, host.hdi_k(D, 0.94))
        delta = D * EPS * 0.1
        assert np.all(s[2:] == 0.1) and np.all(np.abs(s[0] - 0.1) <= delta)
        assert np.all(s[1] <= 2.0 * delta ** 2 * (1.0 + 1e-9)), (D, s[1])


def test_hdi_lengths_and_quantile_positions():
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (10, 4))
    xs = np.sort(x, axis=0)
    s0 = host.summary(x, [], 0)
    assert s0.shape == (4, 4) and np.all(s0[2:] == 0.0)               # hdi_k = 0: no interval
    for k in (10, 11, 1000):                                            # hdi_k >= D: the whole range
        s = host.summary(x, [], k)
        assert np.array_equal(s[2], xs[0]) and np.array_equal(s[3], xs[-1])
    s = host.summary(x, [], 9)                                          # D - 1: one candidate
    assert np.array_equal(s[2], xs[0]) and np.array_equal(s[3], xs[-1])
    s = host.summary(x, [], 1)                                          # the closest pair of neighbours
    i = np.argmin(np.diff(xs, axis=0), axis=0)
    assert np.array_equal(s[2], xs[i, np.arange(4)]) and np.array_equal(s[3], xs[i + 1, np.arange(4)])
    q = np.linspace(0.0, 1.0, 16)
    s = host.summary(x, q, 0)
    assert s.shape == (20, 4) and np.allclose(s[2:18], np.quantile(x, q, axis=0), rtol=1e-14, atol=0)
    assert summary_mod.hdi_length(10, 0.94) == 9 and summary_mod.hdi_length(10, 0.01) == 1
    assert summary_mod.hdi_length(10, 1.0) == 10 and summary_mod.hdi_length(10, None) == 0


def test_offset_and_transform_are_applied_after_the_sort_by_position():
    rng = np.random.default_rng(4)
    x = rng.normal(0, 2, (101, 5))
    off = rng.normal(0, 1, 5)
    q = [0.0, 0.5, 1.0]
    for tf, f in (("identity", lambda v: v), ("exp", np.exp), ("logistic", expit), ("probit", ndtr)):
        s = host.summary(x, q, host.hdi_k(101, 0.9), tf, off)
        t = f(np.sort(x, axis=0) + off)
        assert np.allclose(s[2:5], t[[0, 50, 100]], rtol=1e-13, atol=0), tf
        assert np.allclose(s[0], t.mean(axis=0), rtol=1e-13) and np.allclose(s[1], t.var(axis=0, ddof=1), rtol=1e-11), tf
        for c in range(5):
            assert np.array_equal(host.sorted_column(x[:, c], tf, off[c])[[0, 50, 100]], s[2:5, c]), tf
            assert np.allclose(s[5:, c], hdi(t[:, c], 0.9), rtol=1e-13, atol=0), tf


# ------------------------------------------------------------------ 2. the transforms against libm
def test_transforms_against_numpy_and_scipy():
    fig = json.load(open(ACCURACY))
    got = transform_differences()
    for name, d in got.items():
        print(f"{name}: measured {d:.3e}, committed {fig['max_rel_diff'][name]:.3e}")
        assert d <= 8.0 * fig["max_rel_diff"][name], name
        assert fig["max_rel_diff"][name] <= 8.0 * max(d, 2.0 ** -53), name   # (the committed figure is the measured one)
    x = np.array([-30.0, -1.0, -0.0, 0.0, 1.0, 30.0])
    assert np.array_equal(bits(host.value(x, "identity")), bits(x))
    assert np.all(host.value(x, "logistic") + host.value(-x, "logistic") == pytest.approx(1.0, abs=4 * EPS))


# ------------------------------------------------------------------ 3. host-side validation
def test_argument_errors_are_raised_before_a_backend_is_touched():
    from test_pointwise import _sampler

    s = _sampler(draws=5)
    X = np.zeros((8, 2))
    with pytest.raises(ValueError, match="matrix"):
        posterior_summary(s, np.zeros((2, 2, 2)))
    with pytest.raises(ValueError, match=r"quantiles must be in \[0, 1\]"):
        posterior_summary(s, X, quantiles=[0.5, 1.5])
    with pytest.raises(ValueError, match=r"quantiles must be in \[0, 1\]"):
        posterior_summary(s, X, quantiles=[-0.1])
    with pytest.raises(ValueError, match=r"quantiles must be in \[0, 1\]"):
        posterior_summary(s, X, quantiles=[np.nan])
    with pytest.raises(ValueError, match="at most 16 quantiles"):
        posterior_summary(s, X, quantiles=np.linspace(0, 1, 17))
    with pytest.raises(ValueError, match="vector of levels"):
        posterior_summary(s, X, quantiles=[[0.5]])
    with pytest.raises(ValueError, match="at least 2 draws"):
        posterior_summary(_sampler(draws=1), X)
    with pytest.raises(ValueError, match="at least 2 draws"):
        posterior_summary(s, X, draws=[3])
    with pytest.raises(ValueError, match="at most 16384 draws"):
        posterior_summary(s, X, draws=np.zeros(summary_mod.MAX_DRAWS + 1, int))
    with pytest.raises(ValueError, match="draws must index"):
        posterior_summary(s, X, draws=[0, 5])
    with pytest.raises(ValueError, match="hdi_prob"):
        posterior_summary(s, X, hdi_prob=1.5)
    with pytest.raises(ValueError, match="hdi_prob"):
        posterior_summary(s, X, hdi_prob=0.0)
    with pytest.raises(ValueError, match="unknown transform"):
        posterior_summary(s, X, transform="log")
    with pytest.raises(ValueError, match="offset must have shape"):
        posterior_summary(s, X, offset=np.zeros((2, 8)))
    with pytest.raises(ValueError, match="offset must be finite"):
        posterior_summary(s, X, offset=np.full(8, np.inf))
    with pytest.raises(ValueError, match="excluded must index"):
        posterior_summary(s, X, excluded=[2])
    with pytest.raises(TypeError, match="sampler must be"):
        posterior_summary(object(), X)
    with pytest.raises(AttributeError):                     # a call that passes every check reaches the backend (none)
        posterior_summary(s, X)
    with pytest.raises(ValueError, match="matrix"):
        summarize_matrix(np.zeros(10))
    with pytest.raises(ValueError, match="matrix"):
        summarize_matrix(np.zeros((10, 0)))
    with pytest.raises(ValueError, match="at least 2 draws"):
        summarize_matrix(np.zeros((1, 4)))
    with pytest.raises(ValueError, match="at most 16384 draws"):
        summarize_matrix(np.zeros((summary_mod.MAX_DRAWS + 1, 1)))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            summarize_matrix(np.where(np.arange(40).reshape(10, 4) == 7, bad, 0.0))
    with pytest.raises(ValueError, match=r"quantiles must be in \[0, 1\]"):
        summarize_matrix(np.zeros((10, 4)), quantiles=[2.0])
    with pytest.raises(ValueError, match="at most 16 quantiles"):
        summarize_matrix(np.zeros((10, 4)), quantiles=np.linspace(0, 1, 17))
    with pytest.raises(ValueError, match="unknown transform"):
        summarize_matrix(np.zeros((10, 4)), transform="sqrt")
    assert summary_mod.MAX_DRAWS == host.max_draws() and summary_mod.MAX_QUANTILES == host.max_q()
    assert summary_mod.TRANSFORMS == host.TRANSFORMS


def test_a_backend_that_is_not_hip_is_refused():
    from _oracle import oracle_backend
    from pymc_bart_amd.trees import PosteriorSampler
    from test_pointwise import _sampler

    be = oracle_backend()
    with pytest.raises(_abi.PGBError, match="HIP backend only"):
        summarize_matrix(np.zeros((10, 4)), backend=be)
    s = _sampler(draws=5)
    with pytest.raises(_abi.PGBError, match="HIP backend only"):
        posterior_summary(PosteriorSampler(s.pool, s.forest_idx, s.m, 1, backend=be), np.zeros((8, 2)))


# ------------------------------------------------------------------ 4. partial_dependence
@pytest.fixture(scope="module")
def oracle_fit():
    from _oracle import oracle_backend
    from pymc_bart_amd import BARTOp
    from pymc_bart_amd.chains import sample_chain

    be = oracle_backend()
    rng = np.random.default_rng(8)
    X = rng.uniform(-1, 1, size=(120, 3))
    Y = 2.0 * X[:, 0] + (X[:, 2] > 0) + rng.normal(0, 0.1, 120)
    op = BARTOp(X, Y, m=8)
    sample_chain(op, tune=20, draws=15, random_seed=11, backend=be)
    return be, op, X


def test_partial_dependence_without_a_summary_is_what_it_was(oracle_fit):
    """summary=None: the function's earlier body, restated -- one ``_sample_posterior`` call per covariate on the
    grid, from one generator -- gives the same arrays (``tests/test_oracle_behaviour.py`` pins the same call's
    statistics)."""
    from pymc_bart_amd.partial import pdp_grid
    from pymc_bart_amd.utils import _get_posterior_sampler, _sample_posterior

    be, op, X = oracle_fit
    got = partial_dependence(op, X, xs_interval="linear", xs_values=7, samples=12, random_seed=3, backend=be)
    assert sorted(got) == ["labels", "pd", "reference", "x"]
    sampler = _get_posterior_sampler(op, backend=be)
    rng = np.random.default_rng(3)
    grid = pdp_grid(X, "linear", 7)
    means = []
    for j in range(3):
        want = _sample_posterior(sampler, X=grid, rng=rng, size=12, excluded=[v for v in range(3) if v != j])
        assert want.shape == (12, 7, 1) and np.array_equal(got["pd"][j], want), j
        assert np.array_equal(got["x"][j], grid[:, j]) and got["labels"][j] == f"X_{j}"
        means.append(float(want[:, :, 0].mean()))
    assert got["reference"] == float(np.mean(means))
    doubled = partial_dependence(op, X, var_idx=[1], xs_interval="linear", xs_values=7, samples=12, random_seed=3,
                                 func=lambda a: 2 * a, backend=be, summary=None)
    rng = np.random.default_rng(3)
    want = _sample_posterior(sampler, X=grid, rng=rng, size=12, excluded=[0, 2])
    assert np.array_equal(doubled["pd"][1], 2 * want)


def test_partial_dependence_refusals_of_the_summary_mode(oracle_fit):
    be, op, X = oracle_fit
    with pytest.raises(ValueError, match="func cannot be combined with summary"):
        partial_dependence(op, X, samples=12, func=np.exp, summary={}, backend=be)
    with pytest.raises(ValueError, match="summary takes the keys"):
        partial_dependence(op, X, samples=12, summary={"prob": 0.9}, backend=be)
    with pytest.raises(ValueError, match=r"quantiles must be in \[0, 1\]"):
        partial_dependence(op, X, samples=12, summary={"quantiles": [1.5]}, backend=be)
    with pytest.raises(ValueError, match="at most 16 quantiles"):
        partial_dependence(op, X, samples=12, summary={"quantiles": np.linspace(0, 1, 17)}, backend=be)
    with pytest.raises(ValueError, match="at least 2 draws"):
        partial_dependence(op, X, samples=1, summary={}, backend=be)
    with pytest.raises(ValueError, match="unknown transform"):
        partial_dependence(op, X, samples=12, summary={"transform": "log"}, backend=be)
    with pytest.raises(_abi.PGBError, match="HIP backend only"):
        partial_dependence(op, X, samples=12, summary={}, backend=be)


# ------------------------------------------------------------------ 5. the library
@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_point(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    if not os.path.exists(path):
        pytest.skip(f"{so} has not been built")
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    assert " pgb_row_summary\n" in syms and "pgb_row_summary" not in _abi.SYMBOLS


UNIT = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <vector>
#include "pgbart.h"
#include "pgbart_spec.h"
#include "pgbart_rowsummary.h"
#define PGB_STR2(x) #x
#define PGB_STR(x) PGB_STR2(x)
static thread_local char g_err[512];
static int fail(int code, const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); return code; }
static int fail_hip(hipError_t e, const char* what) { snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e)); return PGB_E_DEVICE; }
#include "k_rowsummary.h"
"""


def test_the_kernel_cross_compiles_for_gfx950_and_is_budgeted(tmp_path):
    """``csrc/k_rowsummary.h`` with the library's flags for gfx950 (device side; the few host names it takes from the
    translation unit stated above it): one kernel, no scratch; and the committed occupancy budget knows it."""
    src, out = tmp_path / "unit.hip", tmp_path / "unit.s"
    src.write_text(UNIT)
    r = subprocess.run([compiled.hipcc_path(), *compiled.DEVICE_FLAGS, f"-I{compiled.CSRC}", "--cuda-device-only", "-S",
                        str(src), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    assert asm.count(".amdhsa_kernel ") == 1 and ".amdhsa_kernel k_rowsum" in asm.replace("_Z8k_rowsum", "k_rowsum")
    meta = asm[asm.index("amdhsa.kernels"):]
    assert ".private_segment_fixed_size: 0" in meta and ".vgpr_spill_count: 0" in meta
    budget = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    row = budget["k_rowsum"]
    assert row["max_scratch_bytes"] == 0 and row["max_vgpr_spills"] == 0 and row["min_wgs_per_cu"] >= 2
