"""Exact Shapley attributions on the MI355X: ``pgb_predict_shap`` (``k_shap``) against the host build of the header it
compiles (``include/pgbart_shap.h`` through ``tests/_shap_host.py``) -- one text, stated order of operations, so the
comparison is ``np.array_equal``, not a tolerance -- over the row counts, column counts, path lengths and leaf kinds at
which the kernel takes another path; then the device against its own brute force (16 ``sample_posterior`` calls with
exclusions at p = 4), efficiency against ``pgb_predict``, and ``shap_summary`` against ``summarize_matrix``.

The tolerances of the brute-force and efficiency tests are worked out, not measured here: the CPU test's ``8 x figure x
M`` (``profiles/shap_accuracy.json``, ``M`` the sum of ``|coef|`` over the entry's leaf terms) for an attribution, and
``_predict_exact``'s ``gamma_N S`` for a prediction of the walk."""
import ctypes as C
import itertools
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _ice_host as ice_host
import _predict_exact as ex
import _shap_host as host
from _predict_exact import Leaf
from pymc_bart_amd import BARTOp, _abi, shap_summary, shap_values, summarize_matrix
from pymc_bart_amd.chains import sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler, _MultiChainSampler

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAXP = int(re.search(r"#define PRED_LDS_MAXP (\d+)", open(os.path.join(ROOT, "pymc_bart_amd", "csrc", "pgb_pred_walk.h")).read()).group(1))
FAST = _abi.SHAP_FAST_U
ONEHOT, SUBSET = _abi.RULE_ONEHOT, _abi.RULE_SUBSET


def _history(s):
    return s.pooled_history() if hasattr(s, "pooled_history") else (s.pool, s.forest_idx)


def _check(s, X, picks):
    """``s.shap`` against the host build of the header, bit for bit; returns ``(values (n_picks, K, n, p), base)``."""
    X = np.ascontiguousarray(X, np.float64)
    pool, table = _history(s)
    got, base = s.shap(X, picks)
    want, wb = host.rows(pool, np.asarray(table), X, picks=picks)
    assert got.shape == (len(picks), s.n_outputs, X.shape[0], X.shape[1]) and base.shape == (len(picks), s.n_outputs)
    assert np.array_equal(got, np.swapaxes(want, 2, 3)) and np.array_equal(base, wb)
    return got, base


def _raw(hip, pool, table, Xw, p, picks, guard=None):
    """The entry point itself on a matrix whose leading dimension exceeds ``p``: ``(n_picks, K, p, n)``.  ``guard``:
    64 cells of it lie behind the output and come back third."""
    mem, lib = hip.mem, hip.lib
    n, ldx = Xw.shape
    K = int(pool.n_outputs)
    fidx = np.ascontiguousarray(table, np.int32)
    picks = np.ascontiguousarray(picks, np.int32)
    xd = mem.from_host(np.ascontiguousarray(Xw))
    size = picks.size * K * p * n
    od = mem.empty((size,), np.float64) if guard is None else mem.from_host(np.full(size + 64, guard))
    base = np.empty((picks.size, K))
    carr = pool.as_c()
    rc = lib.shap_entry_point()(C.byref(carr), fidx.ctypes.data, fidx.shape[0], fidx.shape[1], mem.ptr(xd), n, p, ldx,
                                picks.ctypes.data, picks.size, mem.ptr(od), base.ctypes.data, mem.stream_ptr)
    lib.check(rc, "pgb_predict_shap")
    got = mem.to_host(od)
    if guard is not None:
        return got[:size].reshape(picks.size, K, p, n), base, got[size:]
    return got.reshape(picks.size, K, p, n), base


def _data(rng, n, p, rules=None, nan_rate=0.08):
    X = rng.normal(size=(n, p))
    for j, r in enumerate([] if rules is None else rules):
        if r == ONEHOT:
            X[:, j] = rng.integers(0, 4, n)
        elif r == SUBSET:
            X[:, j] = rng.integers(0, 8, n)
    X[rng.random((n, p)) < nan_rate] = np.nan
    return X


# ------------------------------------------------------------------ 1. row counts, pick counts
@pytest.fixture(scope="module")
def plain(hip):
    """Continuous splits on every column, K = 1; leaves regress on column 3."""
    rng = np.random.default_rng(211)
    pool = ice_host.random_pool(rng, 24, 5, linear=[3])
    return ice_host.pool_sampler(rng, pool, 7, 6, hip), _data(rng, 257, 5)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_row_counts(plain, n):
    s, X = plain
    got, _ = _check(s, X[:n], [0, 5, 0, 2])                           # repeated picks
    assert np.array_equal(got[0], got[2]) and np.count_nonzero(got) > 0
    assert np.all(got[:, :, np.isnan(X[:n])] == 0.0)                  # a NaN entry's attribution is exactly 0.0


def test_one_pick(plain):
    s, X = plain
    _check(s, X[:65], [3])


# ------------------------------------------------------------------ 2. columns, trees, outputs, rules
@pytest.mark.parametrize("p,m,K", [(1, 1, 1), (5, 5, 3), (LDS_MAXP, 7, 1), (LDS_MAXP + 1, 7, 3)])
def test_column_counts_and_a_leading_dimension(hip, p, m, K):
    """p = 1, a few, the last width staged in LDS and the first one read from global memory; ldx > p; linear leaves."""
    rng = np.random.default_rng(300 + p)
    pool = ice_host.random_pool(rng, 3 * m, p, K=K, depth=5, linear=[0, p - 1])
    s = ice_host.pool_sampler(rng, pool, m, 4, hip)
    X = _data(rng, 70, p)
    got, base = _check(s, X, [1, 3, 1])
    wide = np.full((70, p + 3), 55.5)
    wide[:, :p] = X
    raw, rb = _raw(hip, pool, s.forest_idx, wide, p, [1, 3, 1])
    assert np.array_equal(np.swapaxes(raw, 2, 3), got) and np.array_equal(rb, base)


@pytest.mark.parametrize("K", [1, 3])
def test_one_hot_and_subset_columns_mix_leaves(hip, K):
    rng = np.random.default_rng(41 + K)
    rules = [0, ONEHOT, 0, SUBSET, 0]
    pool = ice_host.random_pool(rng, 20, 5, K=K, depth=5, rules=rules, linear=[1, 2, 4])
    s = ice_host.pool_sampler(rng, pool, 5, 5, hip)
    _check(s, _data(rng, 130, 5, rules), [4, 0, 2])


def test_the_hand_built_pools(hip):
    """Zero-count siblings (one and both), -0.0 against a split at 0.0, infinities, a stump, an unused column."""
    for name, pool, fidx, X in host.pools():
        s = PosteriorSampler(pool, fidx, fidx.shape[1], pool.n_outputs, backend=hip)
        got, base = _check(s, X, [0, 1, 2, 1])
        if name == "edges-K1":
            assert np.all(got[1] == 0.0) and base[1, 0] == 3.25 * 5 and np.all(got[:, :, :, 3] == 0.0)


# ------------------------------------------------------------------ 3. path lengths
@pytest.mark.parametrize("depth,linear", [(0, ()), (1, ()), (FAST, ()), (FAST - 1, (FAST,)), (FAST + 1, ()), (FAST, (FAST + 1,)),
                                          (64, ()), (64, (3, 66))])
def test_path_lengths(hip, depth, linear):
    """u = 0, 1, the unrolled evaluation's last length and the next one -- reached by the path alone and by the
    regressor's slot -- and 64 distinct columns on one path at p = 70 (65 slots with the regressor)."""
    if depth == 0:
        pool, fidx = ex.build_pool([Leaf([1.25, -0.5])], 2), np.zeros((1, 1), np.int32)
        X = _data(np.random.default_rng(1), 65, 3)
    else:
        pool, fidx, rng = host.chain_pool(depth, K=2, side="right" if depth % 2 else "left", linear=linear)
        X = host.chain_rows(pool, depth, 70 if depth == 64 else depth + 3, rng, n=65)
        X[1:][rng.random((64, X.shape[1])) < 0.03] = np.nan           # (row 0 follows the whole chain)
    s = PosteriorSampler(pool, fidx, 1, 2, backend=hip)
    got, base = _check(s, X, [0, 0])
    if depth == 0:
        assert np.all(got == 0.0) and base.tolist() == [[1.25, -0.5]] * 2
    else:
        assert np.count_nonzero(got[0, 0, 0]) >= min(depth, 8)


# ------------------------------------------------------------------ 4. two chains, blocking
def test_two_chains_pooled(hip):
    rng = np.random.default_rng(21)
    a = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 14, 4), 7, 5, hip)
    b = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 18, 4, depth=6, linear=[2]), 7, 3, hip)
    s = _MultiChainSampler([a, b])
    X = _data(rng, 100, 4)
    got, base = _check(s, X, [0, 6, 4, 7, 5])                          # chain a, b, a, b, b
    solo, sb = b.shap(X, [1, 2, 0])
    assert np.array_equal(got[[1, 3, 4]], solo) and np.array_equal(base[[1, 3, 4]], sb)


def test_results_do_not_depend_on_the_blocking(plain, monkeypatch):
    s, X = plain
    big = np.concatenate([X, X[:200]])                                # 457 rows, 8 x 4 x 1 x 5 = 160 B of output each
    picks = [1, 4, 1, 0]
    monkeypatch.delenv("PGB_SHAP_BLOCK_BYTES", raising=False)
    ref, rb = _check(s, big, picks)                                   # the default: one block
    summary = shap_summary(s, big, draws=picks, hdi_prob=0.5)
    for limit in ("65536", "4096"):                                   # blocks of 384 rows; the floor: blocks of 64 rows
        monkeypatch.setenv("PGB_SHAP_BLOCK_BYTES", limit)
        got, gb = s.shap(big, picks)
        assert np.array_equal(got, ref) and np.array_equal(gb, rb), limit
        res = shap_summary(s, big, draws=picks, hdi_prob=0.5)
        for key in ("mean", "sd", "quantiles", "hdi", "importance", "base_mean"):
            assert np.array_equal(res[key], summary[key]), (limit, key)


# ------------------------------------------------------------------ 5. a fitted chain: brute force, efficiency
@pytest.fixture(scope="module")
def fit(hip):
    rng = np.random.default_rng(77)
    X = rng.uniform(-1, 1, size=(120, 4))
    Y = 2.0 * X[:, 0] + np.where(X[:, 1] > 0, X[:, 2], -1.0) + rng.normal(0, 0.2, 120)
    op = BARTOp(X, Y, m=10)
    sample_chain(op, tune=30, draws=8, num_particles=10, random_seed=6, sigma=0.2, backend=hip)
    s = _get_posterior_sampler(op, backend=hip)
    rows = X[:24].copy()
    rows[3, 1] = rows[7, 0] = rows[7, 3] = np.nan
    draws = [0, 3, 7]
    pool, table = s.pooled_history()
    pool = pool.decoded() if hasattr(pool, "decoded") else pool
    accuracy = json.load(open(os.path.join(ROOT, "profiles", "shap_accuracy.json")))["max"]
    M, _ = host.magnitude(pool, np.asarray(table)[draws], rows)       # (D, 1, n)
    got = shap_values(s, rows, draws=draws)
    return dict(s=s, rows=rows, draws=draws, pool=pool, table=np.asarray(table), tol=8.0 * accuracy * M[:, 0, :], got=got)


def _gamma_S(exact):
    """``gamma_N S`` per entry (D, K, n) of a walk: ``_predict_exact.bound_ratio``'s bound."""
    D, K, n = exact.R.shape
    out = np.empty((D, K, n), object)
    for d in range(D):
        for i in range(n):
            N = 2 * int(exact.L[d, i]) + 4 + int(exact.T[d, i])
            g = N * ex.U / (1 - N * ex.U)
            for k in range(K):
                out[d, k, i] = g * exact.S[d, k, i]
    return out


def test_the_device_against_its_own_brute_force(fit):
    """16 ``sample_posterior(excluded=...)`` calls combined with the Shapley weights -- in ``Fraction``, so that the
    combination adds no rounding of its own.  Every prediction is within ``gamma_N S`` of its exact value and enters
    an attribution once with a weight of at most 1, every attribution of the device within the CPU test's tolerance."""
    s, rows, draws, got = fit["s"], fit["rows"], fit["draws"], fit["got"]
    assert got["values"].shape == (3, 24, 4) and got["base"].shape == (3,) and got["draws"].tolist() == draws
    p = 4
    to_frac = np.vectorize(lambda x: Fraction(float(x)), otypes=[object])
    v, slack = {}, np.full((3, 24), Fraction(0), object)
    for size in range(p + 1):
        for S in itertools.combinations(range(p), size):
            excl = [j for j in range(p) if j not in S]
            v[frozenset(S)] = to_frac(np.asarray(s.sample_posterior(rows, draws, excl))[:, 0, :])    # (D, n)
            slack = slack + _gamma_S(ex.walk(fit["pool"], fit["table"][draws], rows, excluded=excl))[:, 0, :]
    W = host.shapley_weights(p)
    bound = to_frac(fit["tol"]) + slack
    worst = 0.0
    for j in range(p):
        phi = np.full((3, 24), Fraction(0), object)
        for S, vs in v.items():
            if j not in S:
                phi = phi + W[len(S)] * (v[S | {j}] - vs)
        err = np.abs(to_frac(got["values"][:, :, j]) - phi)
        worst = max(worst, max(float(e / b) for e, b in zip(err.ravel(), bound.ravel()) if b > 0))
        assert np.all(err <= bound), j
    print(f"max |device - brute force| / bound = {worst:.3f}")
    assert np.all(np.abs(to_frac(got["base"]) - v[frozenset()][:, 0]) <= bound[:, 0])


def test_efficiency_on_the_device(fit):
    s, rows, draws, got = fit["s"], fit["rows"], fit["draws"], fit["got"]
    pred = np.asarray(s.sample_posterior(rows, draws, None))[:, 0, :]
    slack = _gamma_S(ex.walk(fit["pool"], fit["table"][draws], rows))[:, 0, :]
    for d in range(3):
        for i in range(24):
            total = Fraction(float(got["base"][d])) + sum(Fraction(float(x)) for x in got["values"][d, i])
            assert abs(total - Fraction(float(pred[d, i]))) <= 5 * Fraction(float(fit["tol"][d, i])) + slack[d, i], (d, i)
    assert np.all(got["values"][:, 3, 1] == 0.0) and np.all(got["values"][:, 7, [0, 3]] == 0.0)


# ------------------------------------------------------------------ 6. the summary, the public calls
def test_shap_summary_is_summarize_matrix_of_shap_values(fit, hip):
    s, rows = fit["s"], fit["rows"]
    draws = [0, 1, 2, 3, 4, 5, 6, 7, 3]
    vals = shap_values(s, rows, draws=draws)
    res = shap_summary(s, rows, draws=draws, quantiles=(0.1, 0.5), hdi_prob=0.8)
    want = summarize_matrix(vals["values"].reshape(len(draws), -1), quantiles=(0.1, 0.5), hdi_prob=0.8, backend=hip)
    assert res["mean"].shape == (24, 4) and res["quantiles"].shape == (2, 24, 4) and res["hdi"].shape == (2, 24, 4)
    for key in ("mean", "sd", "var"):
        assert np.array_equal(res[key], want[key].reshape(24, 4)), key
    assert np.array_equal(res["quantiles"], want["quantiles"].reshape(2, 24, 4))
    assert np.array_equal(res["hdi"], want["hdi"].reshape(2, 24, 4))
    assert np.array_equal(res["importance"], np.abs(res["mean"]).mean(axis=0)) and res["importance"].shape == (4,)
    assert res["base_mean"] == vals["base"].mean() and res["n_draws"] == 9 and res["draws"].tolist() == draws
    assert shap_summary(s, rows, samples=5, random_seed=3, hdi_prob=None)["hdi"] is None


def test_the_public_call_with_several_outputs(hip):
    rng = np.random.default_rng(9)
    pool = ice_host.random_pool(rng, 18, 3, K=3, depth=4)
    s = ice_host.pool_sampler(rng, pool, 6, 4, hip)
    X = _data(rng, 66, 3)
    every = shap_values(s, X)
    assert every["values"].shape == (4, 3, 66, 3) and every["base"].shape == (4, 3) and every["draws"].tolist() == [0, 1, 2, 3]
    want, wb = host.rows(pool, s.forest_idx, X)
    assert np.array_equal(every["values"], np.swapaxes(want, 2, 3)) and np.array_equal(every["base"], wb)
    some = shap_values(s, X, samples=6, random_seed=12)
    picks = np.random.default_rng(12).integers(0, 4, size=6)
    assert some["draws"].tolist() == picks.tolist() and np.array_equal(some["values"], every["values"][picks])
    res = shap_summary(s, X)
    assert res["mean"].shape == (3, 66, 3) and res["importance"].shape == (3, 3) and res["base_mean"].shape == (3,)
    ref = summarize_matrix(every["values"].reshape(4, -1), backend=hip)
    assert np.array_equal(res["mean"], ref["mean"].reshape(3, 66, 3)) and np.array_equal(res["hdi"], ref["hdi"].reshape(2, 3, 66, 3))
