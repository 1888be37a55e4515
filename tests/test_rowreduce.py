"""Per-draw averages over rows on the build box (no GPU): the numeric contract of ``include/pgbart_rowreduce.h``
(``tests/_rowreduce_host.py``) against exact rational arithmetic, the identities the contract promises, the host-side
validation of ``pymc_bart_amd.average``, and the library's exports, kernels and budget.

The bound on a sum (u = 2^-53, the unit roundoff).  A LANE SUM over n rows is a tree of additions of depth at most
t = ceil(n / 64) + 64: at most ceil(n / 64) additions onto a partial, then 64 additions of the partials; the first
addition of either chain is onto 0.0 and exact, so a term passes through at most t - 2 rounded additions.  The term
itself, computed from the header's own v (which the exact sum below takes as given), carries the rounding of
u = v - c (or r = y - v), which counts twice in a square, the rounding of the square and that of the product with w: at
most 4 roundings for S2 and E2, 2 for S1 and E1, none for W.  Every rounding multiplies by (1 + d), |d| <= u, so the
computed sum is sum term_i (1 + e_i) with |e_i| <= (1 + u)^(t + 2) - 1 <= (t + 2) u / (1 - (t + 2) u) < (t + 3) u for
every t here ((t + 2)^2 u < 1):  |computed - exact| <= (t + 3) * 2^-53 * sum |term_i|, the terms and both sums in
exact arithmetic.  (No term here underflows: weights and values are of moderate size.)
"""
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import _rowreduce_host as host
from pymc_bart_amd import _abi, average_contrast, average_prediction, bayes_r2, compiled

average_mod = sys.modules["pymc_bart_amd.average"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, want) -> bool:
    """Bit for bit; a NaN on both sides counts as equal (the payload of a generated NaN is the hardware's)."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def data(n: int, D: int = 3, K: int = 2, G: int = 3, seed: int = 0, layout: str = "random"):
    rng = np.random.default_rng(1000 * n + seed)
    a, b = rng.normal(0.0, 2.0, (D, K, n)), rng.normal(0.0, 2.0, (D, K, n))
    w = rng.uniform(0.1, 3.0, n)
    if layout == "random":
        g = rng.integers(0, G, n)
    elif layout == "contiguous":
        g = np.sort(rng.integers(0, G, n))
    else:                                                       # interleaved row by row
        g = np.arange(n) % G
    return a, b, w, g.astype(np.int32), rng.normal(0.0, 2.0, n), rng.normal(0.0, 1.0, (K, n)), rng.normal(0.0, 1.0, (K, n))


def lane_sum(part: np.ndarray) -> float:
    s = 0.0
    for x in part:
        s = s + float(x)
    return s


def sums_of(r: dict, D, K, G, ns) -> tuple:
    """The finished LANE SUMS (D, K, G, ns) and the weights (G,) from the workspace of ``host.reduce``."""
    ws = r["ws"]
    part = ws[:D * K * G * ns * 64].reshape(D, K, G, ns, 64)
    wpart = ws[D * K * G * ns * 64:D * K * G * ns * 64 + G * 64].reshape(G, 64)
    S = np.array([[[[lane_sum(part[d, k, g, j]) for j in range(ns)] for g in range(G)] for k in range(K)] for d in range(D)])
    return S, np.array([lane_sum(wpart[g]) for g in range(G)])


# ------------------------------------------------------------------ 1. the header against exact arithmetic
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 200, 1000])
@pytest.mark.parametrize("transform", ["identity", "logistic"])
def test_every_sum_is_within_the_derived_bound_of_the_exact_sum(n, transform):
    D, G = 2, 3
    a, _, w, g, y, off, _ = data(n, D=D, K=1, G=G)
    centre = np.array([[0.3, -1.1, 0.0]])
    r = host.reduce(a, w, g, G, y=y, off_a=off, centre=centre, transform=transform)
    S, W = sums_of(r, D, 1, G, 4)
    t = math.ceil(n / 64) + 64
    bound = (t + 3) * Fraction(2) ** -53
    worst = 0.0
    for gi in range(G):
        rows = np.flatnonzero(g == gi)
        fw = [Fraction(float(w[i])) for i in rows]
        exact_W = sum(fw, Fraction(0))
        assert abs(Fraction(float(W[gi])) - exact_W) <= bound * exact_W, ("W", gi)
        for d in range(D):
            fu = [Fraction(float(r["v"][d, 0, i])) - Fraction(float(centre[0, gi])) for i in rows]
            fr = [Fraction(float(y[i])) - Fraction(float(r["v"][d, 0, i])) for i in rows]
            terms = ([x * u for x, u in zip(fw, fu)], [x * u * u for x, u in zip(fw, fu)],
                     [x * q for x, q in zip(fw, fr)], [x * q * q for x, q in zip(fw, fr)])
            for j, name in enumerate(("S1", "S2", "E1", "E2")):
                exact, mass = sum(terms[j], Fraction(0)), sum((abs(x) for x in terms[j]), Fraction(0))
                err = abs(Fraction(float(S[d, 0, gi, j])) - exact)
                assert err <= bound * mass, (name, d, gi, float(err), float(bound * mass))
                if mass:
                    worst = max(worst, float(err / (bound * mass)))
    print(f"n = {n}, {transform}: largest error / bound {worst:.4f}")


def test_the_finish_is_the_stated_formula():
    D, K, G, n = 3, 1, 4, 300
    a, _, w, g, y, _, _ = data(n, D=D, K=K, G=G)
    centre = np.random.default_rng(2).normal(0, 1, (K, G))
    r = host.reduce(a, w, g, G, y=y, centre=centre)
    S, W = sums_of(r, D, K, G, 4)
    out = r["out"]
    assert same(r["W"], W)
    m1 = S[..., 0] / W
    var_fit = np.maximum(S[..., 1] / W - m1 * m1, 0.0)
    bias, mse = S[..., 2] / W, S[..., 3] / W
    var_res = np.maximum(mse - bias * bias, 0.0)
    for j, want in enumerate((centre[None] + m1, var_fit, bias, mse, var_res, var_fit / (var_fit + var_res))):
        assert same(out[j], want), j
    # and it is the weighted mean, the Bayesian R-squared and the MSE NumPy computes
    for gi in range(G):
        m = g == gi
        v = a[:, 0, m]
        mean = (w[m] * v).sum(1) / w[m].sum()
        assert np.allclose(out[0][:, 0, gi], mean, rtol=1e-13, atol=1e-14)
        vf = (w[m] * (v - mean[:, None]) ** 2).sum(1) / w[m].sum()
        res = y[m] - v
        rb = (w[m] * res).sum(1) / w[m].sum()
        vr = (w[m] * (res - rb[:, None]) ** 2).sum(1) / w[m].sum()
        assert np.allclose(out[3][:, 0, gi], (w[m] * res ** 2).sum(1) / w[m].sum(), rtol=1e-13)
        assert np.allclose(out[5][:, 0, gi], vf / (vf + vr), rtol=1e-12)


def test_a_zero_over_zero_r2_stays_nan_and_a_zero_weight_group_is_not_finite():
    a = np.full((2, 1, 70), 1.5)
    r = host.reduce(a, np.ones(70), np.zeros(70, np.int32), 1, y=np.full(70, 1.5))
    assert np.all(r["out"][1] == 0.0) and np.all(r["out"][4] == 0.0) and np.all(np.isnan(r["out"][5]))
    r = host.reduce(a, np.ones(70), np.zeros(70, np.int32), 2)               # group 1 has no row
    assert np.all(r["out"][0][..., 0] == 1.5) and np.all(np.isnan(r["out"][0][..., 1])) and r["W"][1] == 0.0


# ------------------------------------------------------------------ 2. the identities the contract promises
@pytest.mark.parametrize("n", [1, 64, 65, 200, 333])
@pytest.mark.parametrize("layout", ["random", "contiguous", "interleaved"])
def test_the_blocking_changes_no_bit(n, layout):
    a, b, w, g, y, oa, ob = data(n, D=2, K=1, G=3, layout=layout)
    kw = dict(b=b, y=y, off_a=oa, off_b=ob, centre=np.array([[0.5, -0.5, 0.25]]), transform="logistic")
    whole = host.reduce(a, w, g, 3, **kw)
    for variant in (dict(chunk=64), dict(chunk=128), dict(whole_call=True)):
        got = host.reduce(a, w, g, 3, **kw, **variant)
        assert same(got["out"], whole["out"]) and same(got["W"], whole["W"]) and same(got["v"], whole["v"]), variant
        assert np.array_equal(bits(got["ws"]), bits(whole["ws"])), variant
        assert got["n_nonfinite"] == whole["n_nonfinite"] == 0


@pytest.mark.parametrize("factor", [2.0, 0.5])
def test_scaling_the_weights_changes_no_bit_of_mean_mse_r2(factor):
    a, _, w, g, y, _, _ = data(500, D=3, K=1, G=3)
    one = host.reduce(a, w, g, 3, y=y, transform="probit")
    two = host.reduce(a, w * factor, g, 3, y=y, transform="probit")
    assert same(two["out"], one["out"]) and same(two["W"], one["W"] * factor)


def test_equal_arms_give_a_mean_of_exactly_zero():
    a, _, w, g, _, oa, _ = data(300, D=3, K=2, G=3)
    for tf in host.TRANSFORMS:
        r = host.reduce(a, w, g, 3, b=a.copy(), off_a=oa, off_b=oa, transform=tf)
        assert np.all(r["out"] == 0.0) and not np.signbit(r["out"][0]).any() and np.all(r["v"] == 0.0), tf


def test_default_weights_and_groups_and_relabelling():
    n = 200
    a, _, w, g, y, _, _ = data(n, D=2, K=2, G=3)
    assert np.array_equal(average_mod.check_weights(None, n), np.ones(n))
    labels, gid, n_rows = average_mod.check_groups(None, n, np.ones(n))
    assert np.array_equal(labels, [0]) and gid.dtype == np.int32 and not gid.any() and np.array_equal(n_rows, [n])
    one = host.public(a)                                                  # weights=None, groups=None
    assert same(one["mean"], host.public(a, weights=np.ones(n), groups=np.full(n, "all"))["mean"])
    assert one["mean"].shape == (2, 1, 2) and np.array_equal(one["weight"], [float(n)])
    # labels of any kind: np.unique orders them, the outputs follow
    names = np.array(["c", "a", "b"])[g]                                   # group 0 -> "c", 1 -> "a", 2 -> "b"
    by_id, by_name = host.public(a, w, g), host.public(a, w, names)
    assert list(by_name["group_labels"]) == ["a", "b", "c"]
    perm = [1, 2, 0]                                                        # where "a", "b", "c" were
    assert same(by_name["mean"], by_id["mean"][:, perm]) and same(by_name["weight"], by_id["weight"][perm])
    assert np.array_equal(by_name["n_rows"], by_id["n_rows"][perm])
    lab, gid2, _ = average_mod.check_groups(names, n, w)
    assert list(lab) == ["a", "b", "c"] and np.array_equal(np.array(perm)[gid2], g)


def test_r2_lies_in_the_unit_interval():
    rng = np.random.default_rng(9)
    for scale in (1e-3, 1.0, 1e3):
        a = rng.normal(0, scale, (20, 1, 150))
        y = a[0, 0] + rng.normal(0, scale * rng.choice([1e-6, 1.0, 1e3]), 150)
        r2 = host.public(a, rng.uniform(0, 2, 150), rng.integers(0, 4, 150), y=y)["r2"]
        assert r2.shape == (20, 4) and np.all((r2 >= 0.0) & (r2 <= 1.0))


def test_non_finite_terms_are_counted_and_still_added():
    rng = np.random.default_rng(3)
    a = rng.normal(0, 1, (4, 2, 130))
    a[rng.random(a.shape) < 0.1] = 800.0                                   # exp overflows: inf
    n_inf = int((a == 800.0).sum())
    r = host.reduce(a, np.ones(130), np.zeros(130, np.int32), 1, transform="exp")
    assert r["n_nonfinite"] == int((~np.isfinite(np.exp(a))).sum()) == n_inf > 0
    has = (a == 800.0).any(axis=2)
    assert np.array_equal(np.isinf(r["out"][0][..., 0]), has)              # still added
    # inf - inf in a contrast is a NaN and counts as well
    r = host.reduce(a, np.ones(130), np.zeros(130, np.int32), 1, b=a.copy(), transform="exp")
    assert r["n_nonfinite"] == n_inf and np.array_equal(np.isnan(r["out"][0][..., 0]), has)
    # a row without a group adds nothing and is counted once, not once per draw
    g = np.zeros(130, np.int32)
    g[[5, 77]] = (-1, 1)
    r = host.reduce(a, np.ones(130), g, 1, transform="exp")
    assert r["n_bad_group"] == 2 and r["W"][0] == 128.0
    assert r["n_nonfinite"] == int((a[:, :, np.flatnonzero(g == 0)] == 800.0).sum())


# ------------------------------------------------------------------ 3. the Python layer
def test_argument_errors_are_raised_before_a_backend_is_touched(monkeypatch):
    from test_pointwise import _sampler

    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    s, s2 = _sampler(draws=5), _sampler(K=2, draws=5)
    n = 8
    X, y = np.zeros((n, 2)), np.zeros(n)
    calls = (lambda **kw: average_prediction(s, X, **kw), lambda **kw: average_contrast(s, X, X, **kw),
             lambda **kw: bayes_r2(s, X, y, **kw))
    for call in calls:
        with pytest.raises(ValueError, match=r"weights must hold one value per row of X: shape \(8,\)"):
            call(weights=np.ones(7))
        with pytest.raises(ValueError, match=r"weights must hold one value per row"):
            call(weights=np.ones((n, 1)))
        for bad in (np.nan, np.inf, -1.0):
            with pytest.raises(ValueError, match="weights must be finite and >= 0"):
                call(weights=np.where(np.arange(n) == 3, bad, 1.0))
        with pytest.raises(ValueError, match="group 1 has total weight 0"):
            call(weights=np.array([1.0] * 4 + [0.0] * 4), groups=np.array([0] * 4 + [1] * 4))
        with pytest.raises(ValueError, match="total weight 0"):
            call(weights=np.zeros(n))
        with pytest.raises(ValueError, match=r"groups must hold one label per row of X: shape \(8,\)"):
            call(groups=np.zeros(9, int))
        with pytest.raises(ValueError, match="groups must not hold NaN labels"):
            call(groups=np.where(np.arange(n) == 2, np.nan, 1.0))
        with pytest.raises(ValueError, match="groups must hold labels that can be ordered"):
            call(groups=np.array([1, "a", 2.5, None] * 2, dtype=object))
        with pytest.raises(ValueError, match="unknown transform"):
            call(transform="log")
        with pytest.raises(ValueError, match="draws must index"):
            call(draws=[0, 5])
        with pytest.raises(ValueError, match="at least 1 draw"):
            call(draws=[])
        with pytest.raises(AttributeError):                 # a call that passes every check reaches the backend (none)
            call(groups=np.arange(n) % 3, weights=np.arange(n) + 1.0)
    # more groups than the cap; partial sums larger than a block
    big = average_mod.MAX_GROUPS + 1
    with pytest.raises(ValueError, match=f"at most {average_mod.MAX_GROUPS} groups per call, got {big}"):
        average_prediction(s, np.zeros((big, 2)), groups=np.arange(big))
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(1 << 16))
    assert average_mod.workspace_bytes(5, 1, 30, False) > (1 << 16)
    with pytest.raises(ValueError, match="partial sums of 5 draws x 1 outputs x 30 groups take 168976 bytes"):
        average_prediction(s, np.zeros((60, 2)), groups=np.arange(60) % 30)
    with pytest.raises(AttributeError):
        average_prediction(s, np.zeros((60, 2)), groups=np.arange(60) % 3)
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES")
    # the second arm
    with pytest.raises(ValueError, match=r"X_b must have the shape of X_a \(8, 2\), got \(8, 3\)"):
        average_contrast(s, X, np.zeros((n, 3)))
    with pytest.raises(ValueError, match=r"X_b must have the shape of X_a \(8, 2\), got \(7, 2\)"):
        average_contrast(s, X, np.zeros((7, 2)))
    with pytest.raises(ValueError, match="X_b must have the shape"):
        average_contrast(s, X, None)
    with pytest.raises(ValueError, match="offset must have shape"):
        average_contrast(s, X, X, offset_b=np.zeros((2, n)))
    with pytest.raises(ValueError, match="offset must be finite"):
        average_contrast(s, X, X, offset_a=np.full(n, np.inf))
    with pytest.raises(ValueError, match="at least 2 draws"):           # rows=True: summary.spec's limits
        average_contrast(s, X, X, draws=[1], rows=True)
    with pytest.raises(ValueError, match=r"quantiles must be in \[0, 1\]"):
        average_contrast(s, X, X, rows=True, quantiles=[1.5])
    with pytest.raises(ValueError, match="hdi_prob"):
        average_contrast(s, X, X, rows=True, hdi_prob=0.0)
    with pytest.raises(AttributeError):                                   # (without rows the spec is not looked at)
        average_contrast(s, X, X, draws=[1], quantiles=[1.5])
    # y
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="y must be finite"):
            bayes_r2(s, X, np.where(np.arange(n) == 2, bad, 0.0))
    with pytest.raises(ValueError, match="y must hold one value per row"):
        bayes_r2(s, X, np.zeros(7))
    with pytest.raises(ValueError, match="y takes a fit with one output, this one has 2"):
        bayes_r2(s2, X, y)
    with pytest.raises(ValueError, match="matrix"):
        average_prediction(s, np.zeros((2, 2, 2)))
    with pytest.raises(ValueError, match="excluded must index"):
        average_prediction(s, X, excluded=[2])
    with pytest.raises(TypeError, match="sampler must be"):
        average_prediction(object(), X)
    assert average_mod.MAX_GROUPS == host.max_groups() and average_mod.LANES == 64
    for D, K, G, has_y in ((1, 1, 1, False), (5, 2, 3, False), (7, 1, 70, True)):
        assert average_mod.workspace_bytes(D, K, G, has_y) == 8 * host.ws_doubles(D, K, G, has_y)


def test_a_backend_that_is_not_hip_is_refused():
    from _oracle import oracle_backend
    from pymc_bart_amd.trees import PosteriorSampler
    from test_pointwise import _sampler

    s = _sampler(draws=5)
    ps = PosteriorSampler(s.pool, s.forest_idx, s.m, 1, backend=oracle_backend())
    X = np.zeros((8, 2))
    for call in (lambda: average_prediction(ps, X), lambda: average_contrast(ps, X, X), lambda: bayes_r2(ps, X, np.zeros(8))):
        with pytest.raises(_abi.PGBError, match="HIP backend only"):
            call()


# ------------------------------------------------------------------ 4. the library
@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_points(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    if not os.path.exists(path):
        pytest.skip(f"{so} has not been built")
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    for name in ("pgb_row_reduce", "pgb_row_reduce_finish", "pgb_row_reduce_workspace_bytes"):
        assert f" {name}\n" in syms and name not in _abi.SYMBOLS, name


UNIT = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include "pgbart.h"
#include "pgbart_spec.h"
#include "pgbart_rowreduce.h"
#define PGB_STR2(x) #x
#define PGB_STR(x) PGB_STR2(x)
static thread_local char g_err[512];
static int fail(int code, const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); return code; }
static int fail_hip(hipError_t e, const char* what) { snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e)); return PGB_E_DEVICE; }
#include "k_rowreduce.h"
"""


def test_the_kernels_cross_compile_for_gfx950_and_are_budgeted(tmp_path):
    """``csrc/k_rowreduce.h`` with the library's flags for gfx950 (device side; the few host names it takes from the
    translation unit stated above it): two kernels, neither with scratch or spills; and the committed occupancy budget
    knows both, at two or more workgroups per CU."""
    src, out = tmp_path / "unit.hip", tmp_path / "unit.s"
    src.write_text(UNIT)
    r = subprocess.run([compiled.hipcc_path(), *compiled.DEVICE_FLAGS, f"-I{compiled.CSRC}", "--cuda-device-only", "-S",
                        str(src), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    assert asm.count(".amdhsa_kernel ") == 2
    assert ".amdhsa_kernel _Z11k_rowreduce" in asm and ".amdhsa_kernel _Z18k_rowreduce_finish" in asm
    meta = asm[asm.index("amdhsa.kernels"):]
    assert meta.count(".private_segment_fixed_size: 0") == 2 and meta.count(".vgpr_spill_count: 0") == 2
    budget = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    for name in ("k_rowreduce", "k_rowreduce_finish"):
        row = budget[name]
        assert row["max_scratch_bytes"] == 0 and row["max_vgpr_spills"] == 0 and row["min_wgs_per_cu"] >= 2, name
