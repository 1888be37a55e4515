"""Permutation importance on the MI355X: ``pgb_predict_permuted`` (``k_permimp``) against the host reference of
``tests/_permimp_host.py`` -- the oracle's ``pgb_predict`` of the use lists, two NumPy roundings -- bit for bit in both
modes, over the row counts, widths, outputs, leaf kinds, split rules, list lengths and NaN patterns at which the kernel
takes another path; every refusal; row blocking; then ``permutation_importance`` end to end on a two-chain fit.

The one tolerance (``mse_permuted`` against ``bayes_r2`` of the host-permuted matrix) is derived in
:func:`test_end_to_end_against_bayes_r2`'s docstring; everything else is ``np.array_equal`` on the bits."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _ice_host as ice_host
import _permimp_host as host
import _predict_exact as ex
import _rowreduce_host as rowred
from pymc_bart_amd import BARTOp, _abi, bayes_r2, permutation_importance
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.utils import _get_posterior_sampler

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAXP = int(re.search(r"#define PRED_LDS_MAXP (\d+)", open(os.path.join(ROOT, "pymc_bart_amd", "csrc", "pgb_pred_walk.h")).read()).group(1))
ONEHOT, SUBSET = _abi.RULE_ONEHOT, _abi.RULE_SUBSET
PRED, DELTA = host.PRED, host.DELTA
GUARD = -7.75e300    # behind the output: no call may touch it
POISON = 7.0e77      # the padding of ldx > p: no result may show it
E_INVALID = -1


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _call(hip, pool, table, X, first_row, nb, cols, R, seed, picks, mode, pad=3, change=None):
    """The entry point itself on the rows ``first_row .. first_row + nb`` of ``X`` with a leading dimension of
    ``p + pad`` -> ``(rc, out (n_picks, q, R, K, nb), the guard behind it, f)``.  ``change``: arguments replaced after
    everything is laid out (the refusals)."""
    mem, lib = hip.mem, hip.lib
    n, p = X.shape
    K = int(pool.n_outputs)
    table = np.ascontiguousarray(table, np.int32)
    cols, picks = np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(picks, np.int32)
    block = X[first_row:first_row + nb]
    wide = np.full((nb, p + pad), POISON)
    wide[:, :p] = block
    xd, xcols = mem.from_host(wide), mem.from_host(np.ascontiguousarray(X[:, cols].T))
    f = host.predict(hip, pool, table[picks], block) if mode == PRED else None
    fd = None if f is None else mem.from_host(f)
    cells = picks.size * cols.size * R * K * nb
    od = mem.from_host(np.full(cells + 64, GUARD))
    carr = pool.as_c()
    a = dict(fidx=table.ctypes.data, n_forests=table.shape[0], m=table.shape[1], X_dev=mem.ptr(xd), nb=nb, p=p, ldx=p + pad,
             xcols=mem.ptr(xcols), n_total=n, first_row=first_row, cols=cols.ctypes.data, q=cols.size, R=R, seed=seed,
             picks=picks.ctypes.data, n_picks=picks.size, f=None if fd is None else mem.ptr(fd), mode=mode, out=mem.ptr(od))
    a.update(change or {})
    rc = lib.predict_permuted_entry_point()(C.byref(carr), a["fidx"], a["n_forests"], a["m"], a["X_dev"], a["nb"], a["p"], a["ldx"],
                                            a["xcols"], a["n_total"], a["first_row"], a["cols"], a["q"], a["R"], a["seed"],
                                            a["picks"], a["n_picks"], a["f"], a["mode"], a["out"], mem.stream_ptr)
    got = mem.to_host(od)
    return rc, got[:cells].reshape(picks.size, cols.size, R, K, nb), got[cells:], f


def _check(hip, oracle, pool, table, X, first_row, nb, cols, R, seed, picks, pad=3):
    """Both modes against the host reference, bit for bit; the guard untouched; ``f`` the oracle's.  -> the deltas."""
    out = None
    for mode in (PRED, DELTA):
        rc, got, guard, f = _call(hip, pool, table, X, first_row, nb, cols, R, seed, picks, mode, pad)
        hip.lib.check(rc, "pgb_predict_permuted")
        want = host.reference(oracle, pool, table, X, first_row, nb, cols, R, seed, picks, mode)
        assert np.all(guard == GUARD)
        assert np.array_equal(bits(got), bits(want)), (mode, int((bits(got) != bits(want)).sum()), got.size)
        if mode == PRED:
            assert np.array_equal(bits(f), bits(host.predict(oracle, pool, np.asarray(table)[np.asarray(picks)], X[first_row:first_row + nb])))
        out = got
    return out


def _rows(rng, n, p, rules=None, nan_rate=0.05):
    X = rng.normal(size=(n, p))
    for j, r in enumerate([] if rules is None else rules):
        if r == ONEHOT:
            X[:, j] = rng.integers(0, 4, n)
        elif r == SUBSET:
            X[:, j] = rng.integers(0, 8, n)
    X[rng.random((n, p)) < nan_rate] = np.nan
    return X


def _forests(rng, n_trees, m, D):
    return np.stack([rng.permutation(n_trees)[:m] for _ in range(D)]).astype(np.int32)


# ------------------------------------------------------------------ 1. row counts, list lengths, repeats, picks
@pytest.fixture(scope="module")
def lengths():
    """Use lists of 1, 3, 4, 8, 9 and 0 trees: both sides of PRED_WALKS and of its prefetch; K = 1."""
    rng = np.random.default_rng(101)
    pool = host.lengths_pool(rng, 1)
    table = _forests(rng, 12, 12, 3)                                   # the same trees in three orders
    off, _ = host.use_lists(pool, table, 6, list(range(6)))
    assert np.diff(off).reshape(3, 6).tolist() == [list(host.LENGTHS) + [0]] * 3
    return pool, table, _rows(rng, 130, 6)


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 130])
def test_row_counts_and_list_lengths(hip, oracle, lengths, nb):
    pool, table, X = lengths
    delta = _check(hip, oracle, pool, table, X[:nb], 0, nb, list(range(6)), 3, 2024, [0, 2, 0])   # a repeated pick
    assert np.array_equal(bits(delta[0]), bits(delta[2]))
    assert np.all(bits(delta[:, 5]) == 0)                              # the unused column: +0.0 everywhere
    if nb >= 63:
        assert np.count_nonzero(delta[:, :5]) > 0


def test_clean_rows_take_the_fixed_length_walk_too(hip, oracle, lengths):
    pool, table, X = lengths
    clean = np.nan_to_num(X, nan=0.25)
    _check(hip, oracle, pool, table, clean, 0, 130, [4, 0, 3, 5], 1, 7, [1])


def test_a_block_in_the_middle_with_three_outputs_and_linear_leaves(hip, oracle):
    rng = np.random.default_rng(102)
    pool = host.lengths_pool(rng, 3, linear=True)
    table = _forests(rng, 12, 12, 2)
    X = _rows(rng, 300, 6)
    donors = host.perm(55, 4, 0, 300, 128, 100)
    assert donors.min() < 128 and donors.max() >= 228                  # donors lie outside the block
    _check(hip, oracle, pool, table, X, 128, 100, [4, 5, 1], 3, 55, [1, 0])


def test_two_calls_are_the_slices_of_one(hip, oracle, lengths):
    pool, table, X = lengths
    cols, picks = [3, 1, 4], [2, 1]
    for mode in (PRED, DELTA):
        _, whole, _, _ = _call(hip, pool, table, X, 0, 130, cols, 2, 9, picks, mode)
        _, a, _, _ = _call(hip, pool, table, X, 0, 64, cols, 2, 9, picks, mode)
        _, b, _, _ = _call(hip, pool, table, X, 64, 66, cols, 2, 9, picks, mode, pad=0)
        assert np.array_equal(bits(whole[..., :64]), bits(a)) and np.array_equal(bits(whole[..., 64:]), bits(b))


# ------------------------------------------------------------------ 2. widths, outputs, trees per forest, leaves, rules
@pytest.mark.parametrize("p,K,m,linear,R", [(3, 1, 1, False, 3), (3, 3, 12, True, 1), (LDS_MAXP + 1, 1, 12, True, 3),
                                            (LDS_MAXP + 1, 3, 1, False, 1)])
def test_widths_outputs_and_forest_sizes(hip, oracle, p, K, m, linear, R):
    """p = 3 is staged in LDS, p = 127 is the first width read from global memory; constant and linear leaves."""
    rng = np.random.default_rng(200 + p + K)
    pool = ice_host.random_pool(rng, 2 * m + 2, p, K=K, depth=5, linear=[0, p - 1] if linear else None)
    table = _forests(rng, pool.n_trees, m, 3)
    X = _rows(rng, 70, p)
    cols = [p - 1, 0, 1] if p == 3 else [p - 1, 0, 64, 5]
    _check(hip, oracle, pool, table, X, 0, 70, cols, R, 31, [2, 0])


@pytest.mark.parametrize("p,K", [(5, 1), (5, 3), (LDS_MAXP + 1, 1)])
def test_one_hot_and_subset_rules(hip, oracle, p, K):
    """The instances without the continuous rule, staged and not."""
    rng = np.random.default_rng(300 + p + K)
    rules = [0, ONEHOT, 0, SUBSET, 0] + [0] * (p - 5)
    pool = ice_host.random_pool(rng, 16, p, K=K, depth=5, rules=rules, linear=[2, 4], split_cols=[0, 1, 2, 3, 4])
    table = _forests(rng, 16, 8, 2)
    X = _rows(rng, 130, p, rules)
    _check(hip, oracle, pool, table, X, 64, 66, [1, 3, 0, 4], 2, 77, [0, 1])


# ------------------------------------------------------------------ 3. NaN
def test_nan_in_the_donor_values_only(hip, oracle, lengths):
    """A tile without a NaN whose permuted walk is not clean: the rows of the block hold none, the rest of the two
    columns is NaN in every third row."""
    pool, table, X = lengths
    X = np.nan_to_num(np.concatenate([X, X[:70]]), nan=-0.5)           # 200 rows
    X[64::3, 3] = np.nan
    X[65::3, 4] = np.nan
    for c in (3, 4):
        donors = X[host.perm(12, c, 0, 200, 0, 64), c]
        assert np.isnan(donors).any() and not np.isnan(donors).all()
    assert not np.isnan(X[:64]).any()
    _check(hip, oracle, pool, table, X, 0, 64, [3, 4, 0], 2, 12, [0, 1])


# ------------------------------------------------------------------ 4. refusals
def test_every_refusal_leaves_the_output_untouched(hip, lengths):
    pool, table, X = lengths
    bad_cols, twice = np.array([0, 9, 1], np.int32), np.array([2, 0, 2], np.int32)
    bad_picks, many = np.array([0, 3], np.int32), np.zeros(64, np.int32)
    cases = [
        (dict(X_dev=None), "X_dev is null"), (dict(xcols=None), "xcols_dev is null"), (dict(cols=None), "cols_host is null"),
        (dict(picks=None), "picks_host is null"), (dict(fidx=None), "forest_tree_idx is null"),
        (dict(m=0), "n_forests, m and p must be >= 1"), (dict(nb=0), "nb must be >= 1"), (dict(n_total=0), "n_total must be >= 1"),
        (dict(q=0), "q must be >= 1"), (dict(R=0), "n_repeats must be >= 1"), (dict(n_picks=0), "n_picks must be >= 1"),
        (dict(ldx=5), "ldx must be >= p"), (dict(first_row=-64), "first_row"), (dict(first_row=64), "first_row"),
        (dict(n_total=1 << 62, first_row=0), "n_total must be below 2^62"),
        (dict(R=65536), "n_repeats must be <= 65535"), (dict(mode=2), "mode must be"), (dict(mode=-1), "mode must be"),
        (dict(f=None), "f_dev is null in mode PGB_PERMIMP_PRED"),
        (dict(mode=DELTA), "f_dev must be null in mode PGB_PERMIMP_DELTA"),
        (dict(cols=bad_cols.ctypes.data), "cols_host[1] = 9 is outside [0, p = 6)"),
        (dict(cols=twice.ctypes.data), "repeats cols_host"),
        (dict(picks=bad_picks.ctypes.data), "picks_host[1] = 3 is outside [0, n_forests = 3)"),
        (dict(nb=(1 << 37) - 64, n_total=1 << 38, R=65535, picks=many.ctypes.data, n_picks=64), "overflows a 64-bit size"),
    ]
    for change, msg in cases:
        rc, got, guard, _ = _call(hip, pool, table, X, 0, 130, [2, 0, 4], 2, 5, [0, 1], PRED, change=change)
        text = hip.lib.lib.pgb_last_error().decode()
        assert rc == E_INVALID and msg in text and text.startswith("pgb_predict_permuted: "), (change, rc, text)
        assert np.all(got == GUARD) and np.all(guard == GUARD), change
    table_bad = table.copy()                                           # a malformed history: pgb_predict's checks
    table_bad[1, 3] = 12
    rc, got, guard, _ = _call(hip, pool, table, X, 0, 130, [2, 0, 4], 2, 5, [0, 1], PRED, change=dict(fidx=table_bad.ctypes.data))
    assert rc == E_INVALID and "forest_tree_idx entry outside" in hip.lib.lib.pgb_last_error().decode()
    assert np.all(got == GUARD) and np.all(guard == GUARD)


# ------------------------------------------------------------------ 5. end to end
N_FIT, M_FIT = 300, 10


@pytest.fixture(scope="module")
def fit(hip):
    """Two chains of 12 draws behind one sampler; only columns 0 and 1 carry signal."""
    rng = np.random.default_rng(61)
    X = rng.uniform(-1, 1, size=(N_FIT, 6))
    y = 2.0 * X[:, 0] + np.where(X[:, 1] > 0, 1.5, -1.5) + rng.normal(0, 0.3, N_FIT)
    op = BARTOp(X, y, m=M_FIT)
    attach_history(op, [sample_chain(op, 30, 12, random_seed=4, chain=c, backend=hip, keep_draws=False) for c in (0, 1)])
    return X, y, _get_posterior_sampler(op, backend=hip)


def _history(s):
    pool, table = s.pooled_history() if hasattr(s, "pooled_history") else (s.pool, s.forest_idx)
    return (pool.decoded() if hasattr(pool, "decoded") else pool), np.asarray(table)


def test_end_to_end_against_bayes_r2(hip, oracle, fit, monkeypatch):
    """``mse_base`` has ``bayes_r2``'s bits; ``mse_permuted`` has the bits of the row reduce of the reference's ``fperm``
    and lies within a derived bound of ``bayes_r2`` on the host-permuted ``X``:

    * per row, ``fperm`` and the direct prediction are roundings of the same exact number, each within ``gamma_N`` times
      the absolute leaf contributions of its walks, ``N = 2 m + 2`` (``test_permimp.py``); the walks over a use list
      add a subset of the forest's leaves, so ``|fperm - direct| <= e = 2 gamma_N (S(x) + S(x'))``;
    * ``|(y - v - d)^2 - (y - v)^2| <= |d| (2 |y - v| + |d|)``, so the means differ by at most the weighted mean of
      ``e (2 |r| + e)``;
    * each reduce rounds a term three times, adds at most ``t = ceil(n / 64) + 64`` of them and divides once: a relative
      ``gamma_(t + 4)`` of a sum of non-negative terms, for each of the two.
    """
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    X, y, s = fit
    pool, table = _history(s)
    D = s.n_draws
    assert D == 24
    res = permutation_importance(s, X, y, n_repeats=2, random_seed=11)
    base = bayes_r2(s, X, y)
    assert np.array_equal(bits(res["mse_base"]), bits(base["mse"][:, 0]))
    assert res["mse_permuted"].shape == (D, 6, 2) and res["importance"].shape == (D, 6) and res["n_nonfinite"] == 0
    ref = host.reference(oracle, pool, table, X, 0, N_FIT, list(range(6)), 2, 11, np.arange(D), PRED)
    want = rowred.public(ref.reshape(-1, 1, N_FIT), y=y)
    assert np.array_equal(bits(res["mse_permuted"]), bits(want["mse"][:, 0].reshape(D, 6, 2)))
    assert np.array_equal(bits(res["importance"]), bits(res["mse_permuted"].mean(axis=2) - res["mse_base"][:, None]))
    # the signal columns matter, the noise columns do not
    mean = res["importance_mean"]
    print("importance_mean:", np.array2string(mean, precision=4))
    assert mean[:2].min() > mean[2:].max()
    # (draw, column) pairs whose use list is empty: exactly 0.0
    off, _ = host.use_lists(pool, table, 6, list(range(6)))
    empty = np.diff(off).reshape(D, 6) == 0
    f = s.sample_posterior(X, list(range(D)), None)
    assert empty.any() and not np.any((f == 0.0) & np.signbit(f))
    assert np.all(res["importance"][empty] == 0.0) and np.all(res["r2_drop"][empty] == 0.0)
    # against bayes_r2 of the explicitly permuted matrix, two draws and two columns
    draws = [0, 17]
    N = 2 * M_FIT + 2
    gamma = N * ex.U / (1 - N * ex.U)
    t = math.ceil(N_FIT / 64) + 64
    g_sum = (t + 4) * ex.U / (1 - (t + 4) * ex.U)
    S_x = ex.walk(pool, table[draws], X).S[:, 0, :]
    worst = 0.0
    for c in (0, 3):
        Xp = host.permuted_matrix(X, c, 11, 1)
        direct = bayes_r2(s, Xp, y, draws=draws)["mse"][:, 0]
        pred = s.sample_posterior(Xp, draws, None)[:, 0, :]
        S_p = ex.walk(pool, table[draws], Xp).S[:, 0, :]
        for j, d in enumerate(draws):
            e = [2 * gamma * (S_x[j, i] + S_p[j, i]) for i in range(N_FIT)]
            r = [abs(Fraction(float(y[i])) - Fraction(float(pred[j, i]))) for i in range(N_FIT)]
            bound = sum(e[i] * (2 * r[i] + e[i]) for i in range(N_FIT)) / N_FIT
            bound += g_sum * (Fraction(float(direct[j])) + Fraction(float(res["mse_permuted"][d, c, 1])))
            err = abs(Fraction(float(direct[j])) - Fraction(float(res["mse_permuted"][d, c, 1])))
            assert err <= bound, (c, d, float(err), float(bound))
            worst = max(worst, float(err / bound))
    print(f"max |mse_permuted - bayes_r2(permuted X)| / bound = {worst:.3f}")


def test_blocks_chunks_groups_and_no_y(hip, fit, monkeypatch):
    X, y, s = fit
    draws = [1, 8, 13, 22]
    halves = np.arange(N_FIT) >= 150
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    whole = permutation_importance(s, X, y, n_repeats=2, draws=draws, groups=halves, random_seed=3)
    free = permutation_importance(s, X, n_repeats=2, draws=draws, groups=halves, random_seed=3)
    keys = ("mse_permuted", "mse_base", "importance", "importance_mean", "importance_sd", "importance_hdi", "r2_drop", "weight")
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")                 # chunks of columns, blocks of 64 rows
    small = permutation_importance(s, X, y, n_repeats=2, draws=draws, groups=halves, random_seed=3)
    for key in keys:
        assert np.array_equal(bits(small[key]), bits(whole[key])), key
    small_free = permutation_importance(s, X, n_repeats=2, draws=draws, groups=halves, random_seed=3)
    for key in ("shift", "sensitivity"):
        assert free[key].shape == (4, 6, 2) and np.array_equal(bits(small_free[key]), bits(free[key])), key
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    # two halves as groups, or as two calls whose weights zero the other half: a term of weight 0 adds 0.0
    for g in (0, 1):
        one = permutation_importance(s, X, y, n_repeats=2, draws=draws, weights=(halves == bool(g)).astype(float), random_seed=3)
        for key in ("mse_permuted", "mse_base", "importance", "r2_drop"):
            assert np.array_equal(bits(one[key]), bits(whole[key][..., g])), (g, key)
        assert one["weight"].tolist() == [150.0]
    # a subset of the columns gives the slices
    some = permutation_importance(s, X, y, cols=[3, 1], n_repeats=2, draws=draws, groups=halves, random_seed=3)
    assert np.array_equal(bits(some["mse_permuted"]), bits(whole["mse_permuted"][:, [3, 1]]))
    assert np.all(free["sensitivity"] >= 0.0) and free["sensitivity"][:, :2].mean() > free["sensitivity"][:, 2:].mean()
