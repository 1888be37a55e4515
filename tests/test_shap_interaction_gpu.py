"""Exact SHAP interaction values on the MI355X: ``pgb_predict_shap_interactions`` (``k_shap_interaction``) against the
host build of the header it compiles (``include/pgbart_shap_interaction.h`` through ``tests/_shap_interaction_host.py``)
-- one text, stated order of operations, so the comparison is ``np.array_equal``, not a tolerance -- over the row
counts, column counts, column subsets, path lengths and leaf kinds at which the kernel takes another path; then row sums
against ``shap_values``, the total against ``pgb_predict``, ``shap_interaction_summary`` against ``summarize_matrix`` and
the slot limit.

The tolerances of the row-sum and total tests are the CPU test's: ``8 x figure x M`` per entry
(``profiles/shap_interaction_accuracy.json``, ``M`` the sum of ``|coef|`` over the entry's leaf terms), ``p + 1`` of them
for a row sum and ``p p + 1`` for the total, to which the prediction adds ``_predict_exact``'s ``gamma_N S`` of its own."""
import ctypes as C
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _ice_host as ice_host
import _predict_exact as ex
import _shap_host as host
import _shap_interaction_host as hx
from _predict_exact import Leaf
from pymc_bart_amd import BARTOp, _abi, shap_interaction_summary, shap_interaction_values, shap_values, summarize_matrix
from pymc_bart_amd.chains import sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler, _MultiChainSampler

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAXP = int(re.search(r"#define PRED_LDS_MAXP (\d+)", open(os.path.join(ROOT, "pymc_bart_amd", "csrc", "pgb_pred_walk.h")).read()).group(1))
FAST = _abi.SHAP_FAST_U
LIMIT = _abi.SHAPX_MAX_U
ONEHOT, SUBSET = _abi.RULE_ONEHOT, _abi.RULE_SUBSET
E_INVALID = -1


def _history(s):
    return s.pooled_history() if hasattr(s, "pooled_history") else (s.pool, s.forest_idx)


def _check(s, X, picks, cols=None):
    """``s.shap_interactions`` against the host build of the header, bit for bit; returns ``(values (n_picks, K, n, q,
    q), base)``."""
    X = np.ascontiguousarray(X, np.float64)
    pool, table = _history(s)
    got, base = s.shap_interactions(X, picks, cols)
    want, wb = hx.rows(pool, np.asarray(table), X, cols=cols, picks=picks)
    q = X.shape[1] if cols is None else len(cols)
    assert got.shape == (len(picks), s.n_outputs, X.shape[0], q, q) and base.shape == (len(picks), s.n_outputs)
    assert np.array_equal(got, np.moveaxis(want, 4, 2)) and np.array_equal(base, wb)
    return got, base


def _raw(hip, pool, table, Xw, p, cols, picks, fill=None, guard=None):
    """The entry point itself on a matrix whose leading dimension may exceed ``p``: ``(rc, (n_picks, K, q, q, n),
    base)``; ``fill``: what the output holds before the call; ``guard``: 64 cells of it lie behind the output and come
    back fourth."""
    mem, lib = hip.mem, hip.lib
    n, ldx = Xw.shape
    K = int(pool.n_outputs)
    fidx = np.ascontiguousarray(table, np.int32)
    picks = np.ascontiguousarray(picks, np.int32)
    cols = np.ascontiguousarray(cols, np.int32)
    q = int(cols.size)
    xd = mem.from_host(np.ascontiguousarray(Xw))
    size = picks.size * K * q * q * n
    od = mem.empty((size,), np.float64) if fill is None else mem.from_host(np.full(size, fill))
    if guard is not None:
        od = mem.from_host(np.concatenate([np.full(size, guard if fill is None else fill), np.full(64, guard)]))
    base = np.empty((picks.size, K))
    carr = pool.as_c()
    rc = lib.shap_interactions_entry_point()(C.byref(carr), fidx.ctypes.data, fidx.shape[0], fidx.shape[1], mem.ptr(xd), n, p,
                                             ldx, cols.ctypes.data, q, picks.ctypes.data, picks.size, mem.ptr(od),
                                             base.ctypes.data, mem.stream_ptr)
    got = mem.to_host(od)
    if guard is not None:
        return rc, got[:size].reshape(picks.size, K, q, q, n), base, got[size:]
    return rc, got.reshape(picks.size, K, q, q, n), base


def _data(rng, n, p, rules=None, nan_rate=0.08):
    X = rng.normal(size=(n, p))
    for j, r in enumerate([] if rules is None else rules):
        if r == ONEHOT:
            X[:, j] = rng.integers(0, 4, n)
        elif r == SUBSET:
            X[:, j] = rng.integers(0, 8, n)
    X[rng.random((n, p)) < nan_rate] = np.nan
    return X


def _with_regressor(pool, col):
    for g in np.flatnonzero(np.asarray(pool.var) < 0):
        pool.svar[g], pool.xbar[g] = col, 0.25
        pool.slope[g] = 0.5
    return pool


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
    assert np.array_equal(got, np.swapaxes(got, 3, 4))                # bitwise symmetric
    nan = np.isnan(X[:n])
    for i, j in zip(*np.nonzero(nan)):                                # a NaN entry's row and column are exactly 0.0
        assert np.all(got[:, :, i, j, :] == 0.0) and np.all(got[:, :, i, :, j] == 0.0)


# ------------------------------------------------------------------ 2. columns, trees, outputs, rules
@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("p,m,K", [(1, 1, 1), (5, 5, 3), (LDS_MAXP, 7, 1), (LDS_MAXP + 1, 7, 3)])
def test_column_counts_subsets_and_a_leading_dimension(hip, p, m, K, subset):
    """p = 1, a few, the last width staged in LDS and the first one read from global memory; every column and a
    subset of 3 in an order of its own; ldx > p; linear leaves."""
    rng = np.random.default_rng(300 + p)
    pool = ice_host.random_pool(rng, 3 * m, p, K=K, depth=5, linear=[0, p - 1])
    s = ice_host.pool_sampler(rng, pool, m, 4, hip)
    X = _data(rng, 70, p)
    cols = None if not subset else ([0] if p == 1 else [p - 1, 0, p // 2])
    got, base = _check(s, X, [1, 3, 1], cols)
    wide = np.full((70, p + 3), 55.5)
    wide[:, :p] = X
    rc, raw, rb = _raw(hip, pool, s.forest_idx, wide, p, np.arange(p) if cols is None else cols, [1, 3, 1])
    assert rc == 0 and np.array_equal(np.moveaxis(raw, 4, 2), got) and np.array_equal(rb, base)
    if subset and p == 5:                                             # a subset is a slice of the full result
        full, _ = s.shap_interactions(X, [1, 3, 1])
        assert np.array_equal(got, full[:, :, :, cols][:, :, :, :, cols])


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
        _check(s, X, [2, 0], cols=[3, 1, 2])
        if name == "edges-K1":
            assert np.all(got[1] == 0.0) and base[1, 0] == 3.25 * 5
            assert np.all(got[:, :, :, 3] == 0.0) and np.all(got[:, :, :, :, 3] == 0.0)


# ------------------------------------------------------------------ 3. path lengths
@pytest.mark.parametrize("depth,regressor", [(0, None), (0, 1), (1, None), (FAST - 1, None), (FAST - 2, FAST - 1), (FAST, None),
                                             (FAST - 1, FAST), (FAST + 1, None), (FAST, FAST + 1), (LIMIT, None),
                                             (LIMIT - 1, LIMIT + 1)])
def test_path_lengths(hip, depth, regressor):
    """u = 0, 1, the unrolled evaluation's last length, the ones on either side of it and the limit of 32 slots --
    reached by the path alone and by the regressor's slot."""
    if depth == 0:
        pool, fidx = ex.build_pool([Leaf([1.25, -0.5])], 2), np.zeros((1, 1), np.int32)
        if regressor is not None:
            _with_regressor(pool, regressor)                          # a stump that regresses: one slot
        X = _data(np.random.default_rng(1), 65, 3)
        assert hx.slots(pool, 3) == (regressor is not None)
    else:
        pool, fidx, rng = host.chain_pool(depth, K=2, side="right" if depth % 2 else "left")
        if regressor is not None:
            _with_regressor(pool, regressor)
        X = host.chain_rows(pool, depth, depth + 3, rng, n=65)
        X[1:][rng.random((64, X.shape[1])) < 0.03] = np.nan           # (row 0 follows the whole chain)
        assert hx.slots(pool, depth + 3) == depth + (regressor is not None)
    s = PosteriorSampler(pool, fidx, 1, 2, backend=hip)
    got, base = _check(s, X, [0, 0])
    if depth == 0:
        assert base.tolist() == [[1.25, -0.5]] * 2
        off = got.copy()
        if regressor is not None:                                     # only the regressor's main effect: 0.5 (x - 0.25), NaN: 0.0
            assert np.array_equal(got[0, 0, :, 1, 1], np.nan_to_num(0.5 * (X[:, 1] - 0.25)))
            off[:, :, :, regressor, regressor] = 0.0
        assert np.all(off == 0.0)
    else:
        assert np.count_nonzero(got[0, 0, 0]) >= min(depth, 8)


def test_more_than_32_slots_return_invalid_and_launch_nothing(hip):
    pool, fidx, rng = host.chain_pool(LIMIT, K=1, side="left")
    _with_regressor(pool, LIMIT + 1)
    X = host.chain_rows(pool, LIMIT, LIMIT + 3, rng, n=3)
    rc, out, _ = _raw(hip, pool, fidx, X, LIMIT + 3, [0, LIMIT + 1], [0], fill=-7.5)
    msg = hip.lib.lib.pgb_last_error().decode()
    assert rc == E_INVALID and "a leaf of 33 slots" in msg and "the limit is 32" in msg, msg
    assert np.all(out == -7.5)                                        # nothing was written
    s = PosteriorSampler(pool, fidx, 1, 1, backend=hip)
    with pytest.raises(Exception, match="a leaf of 33 slots"):
        s.shap_interactions(X, [0])


# ------------------------------------------------------------------ 4. two chains, blocking
def test_two_chains_pooled(hip):
    rng = np.random.default_rng(21)
    a = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 14, 4), 7, 5, hip)
    b = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 18, 4, depth=6, linear=[2]), 7, 3, hip)
    s = _MultiChainSampler([a, b])
    X = _data(rng, 100, 4)
    got, base = _check(s, X, [0, 6, 4, 7, 5])                          # chain a, b, a, b, b
    solo, sb = b.shap_interactions(X, [1, 2, 0])
    assert np.array_equal(got[[1, 3, 4]], solo) and np.array_equal(base[[1, 3, 4]], sb)


def test_results_do_not_depend_on_the_blocking(plain, monkeypatch):
    s, X = plain
    big = np.concatenate([X, X[:200]])                                # 457 rows, 8 x 4 x 1 x 25 = 800 B of output each
    picks = [1, 4, 1, 0]
    monkeypatch.delenv("PGB_SHAP_BLOCK_BYTES", raising=False)
    ref, rb = _check(s, big, picks)                                   # the default: one block
    sub, _ = s.shap_interactions(big, picks, [4, 1])
    summary = shap_interaction_summary(s, big, draws=picks, hdi_prob=0.5)
    for limit in ("65536", "4096"):                                   # blocks of 64 rows (81 rows fit), and the floor
        monkeypatch.setenv("PGB_SHAP_BLOCK_BYTES", limit)
        got, gb = s.shap_interactions(big, picks)
        assert np.array_equal(got, ref) and np.array_equal(gb, rb), limit
        assert np.array_equal(s.shap_interactions(big, picks, [4, 1])[0], sub), limit   # 128 B each: blocks of 512 rows at 65536
        res = shap_interaction_summary(s, big, draws=picks, hdi_prob=0.5)
        for key in ("mean", "sd", "quantiles", "hdi", "strength", "base_mean"):
            assert np.array_equal(res[key], summary[key]), (limit, key)


# ------------------------------------------------------------------ 5. a fitted chain: row sums, the total
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
    accuracy = json.load(open(os.path.join(ROOT, "profiles", "shap_interaction_accuracy.json")))["max"]
    M, _ = host.magnitude(pool, np.asarray(table)[draws], rows)       # (D, 1, n)
    got = shap_interaction_values(s, rows, draws=draws)
    return dict(s=s, rows=rows, draws=draws, pool=pool, table=np.asarray(table), tol=8.0 * accuracy * M[:, 0, :], got=got)


def test_row_sums_and_the_total_on_the_device(fit):
    s, rows, draws, got = fit["s"], fit["rows"], fit["draws"], fit["got"]
    p = 4
    assert got["values"].shape == (3, 24, p, p) and got["base"].shape == (3,) and got["draws"].tolist() == draws
    assert got["cols"].tolist() == [0, 1, 2, 3]
    want, wb = hx.rows(fit["pool"], fit["table"], rows, picks=draws)
    assert np.array_equal(got["values"], np.moveaxis(want, 4, 2)[:, 0]) and np.array_equal(got["base"], wb[:, 0])
    shap = shap_values(s, rows, draws=draws)
    assert np.array_equal(shap["base"], got["base"])
    pred = np.asarray(s.sample_posterior(rows, draws, None))[:, 0, :]
    exact = ex.walk(fit["pool"], fit["table"][draws], rows)
    worst_row = worst_total = 0.0
    for d in range(3):
        for i in range(24):
            tol = Fraction(float(fit["tol"][d, i]))
            for a in range(p):
                row = sum(Fraction(float(x)) for x in got["values"][d, i, a])
                err = abs(row - Fraction(float(shap["values"][d, i, a])))
                worst_row = max(worst_row, float(err / ((p + 1) * tol)) if tol else 0.0)
                assert err <= (p + 1) * tol, (d, i, a)
            N = 2 * int(exact.L[d, i]) + 4 + int(exact.T[d, i])
            slack = N * ex.U / (1 - N * ex.U) * exact.S[d, 0, i]
            total = Fraction(float(got["base"][d])) + sum(Fraction(float(x)) for x in got["values"][d, i].ravel())
            err = abs(total - Fraction(float(pred[d, i])))
            worst_total = max(worst_total, float(err / ((p * p + 1) * tol + slack)))
            assert err <= (p * p + 1) * tol + slack, (d, i)
    print(f"max row-sum error / bound = {worst_row:.3f}, max total error / bound = {worst_total:.3f}")
    assert np.all(got["values"][:, 3, 1] == 0.0) and np.all(got["values"][:, 3, :, 1] == 0.0)
    assert np.all(got["values"][:, 7, [0, 3]] == 0.0) and np.all(got["values"][:, 7][:, :, [0, 3]] == 0.0)
    assert np.count_nonzero(got["values"][:, :, 1, 2]) > 0            # the data's interaction is there


# ------------------------------------------------------------------ 6. the summary, the public calls
def test_the_summary_is_summarize_matrix_of_the_values(fit, hip):
    s, rows = fit["s"], fit["rows"]
    draws = [0, 1, 2, 3, 4, 5, 6, 7, 3]
    for cols, q in ((None, 4), ([2, 0, 1], 3)):
        vals = shap_interaction_values(s, rows, cols=cols, draws=draws)
        res = shap_interaction_summary(s, rows, cols=cols, draws=draws, quantiles=(0.1, 0.5), hdi_prob=0.8)
        want = summarize_matrix(vals["values"].reshape(len(draws), -1), quantiles=(0.1, 0.5), hdi_prob=0.8, backend=hip)
        assert res["mean"].shape == (24, q, q) and res["quantiles"].shape == (2, 24, q, q) and res["hdi"].shape == (2, 24, q, q)
        for key in ("mean", "sd", "var"):
            assert np.array_equal(res[key], want[key].reshape(24, q, q)), key
        assert np.array_equal(res["quantiles"], want["quantiles"].reshape(2, 24, q, q))
        assert np.array_equal(res["hdi"], want["hdi"].reshape(2, 24, q, q))
        assert np.array_equal(res["strength"], np.abs(res["mean"]).mean(axis=0)) and res["strength"].shape == (q, q)
        assert res["base_mean"] == vals["base"].mean() and res["n_draws"] == 9 and res["draws"].tolist() == draws
        assert res["cols"].tolist() == vals["cols"].tolist() == ([0, 1, 2, 3] if cols is None else cols)
    assert shap_interaction_summary(s, rows, samples=5, random_seed=3, hdi_prob=None)["hdi"] is None


def test_the_public_call_with_several_outputs(hip):
    rng = np.random.default_rng(9)
    pool = ice_host.random_pool(rng, 18, 3, K=3, depth=4)
    s = ice_host.pool_sampler(rng, pool, 6, 4, hip)
    X = _data(rng, 66, 3)
    every = shap_interaction_values(s, X)
    assert every["values"].shape == (4, 3, 66, 3, 3) and every["base"].shape == (4, 3) and every["draws"].tolist() == [0, 1, 2, 3]
    want, wb = hx.rows(pool, s.forest_idx, X)
    assert np.array_equal(every["values"], np.moveaxis(want, 4, 2)) and np.array_equal(every["base"], wb)
    some = shap_interaction_values(s, X, cols=[2, 1], samples=6, random_seed=12)
    picks = np.random.default_rng(12).integers(0, 4, size=6)
    assert some["draws"].tolist() == picks.tolist()
    assert np.array_equal(some["values"], every["values"][picks][:, :, :, [2, 1]][:, :, :, :, [2, 1]])
    res = shap_interaction_summary(s, X)
    assert res["mean"].shape == (3, 66, 3, 3) and res["strength"].shape == (3, 3, 3) and res["base_mean"].shape == (3,)
    ref = summarize_matrix(every["values"].reshape(4, -1), backend=hip)
    assert np.array_equal(res["mean"], ref["mean"].reshape(3, 66, 3, 3))
    assert np.array_equal(res["hdi"], ref["hdi"].reshape(2, 3, 66, 3, 3))
