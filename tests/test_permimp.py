"""Permutation importance, the parts that need no GPU: the permutation of ``include/pgbart_permimp.h`` (pins, bijection,
a uniformity condition), the packer of the use lists against a NumPy recount, the host reference of the value against
the oracle's ``pgb_predict`` of the explicitly permuted matrix, and the Python layer -- its refusals and argument order
on the recording backend, its chunking and its subset rule on a backend made of the host references
(``_permimp_host.HostBackend``)."""
from fractions import Fraction

import numpy as np
import pytest

import _ice_host as ice_host
import _permimp_host as host
import _predict_exact as ex
import _rowreduce_host as rowred
from _recording_backend import Recorder
from pymc_bart_amd import _abi, permutation_importance
from pymc_bart_amd import permutation as perm_mod
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays

# ------------------------------------------------------------------ 1. the permutation
PINS = [((5, 12345, 3, 0), [1, 3, 2, 0, 4]),
        ((10, 1, 0, 0), [6, 4, 5, 1, 7, 8, 9, 3, 0, 2]),
        ((10, 1, 0, 1), [9, 3, 5, 1, 2, 4, 8, 6, 0, 7]),
        ((10, 2 ** 63 + 5, 7, 2), [8, 2, 3, 5, 4, 9, 6, 1, 7, 0]),
        ((100000, 42, 49, 4), [95270, 3459, 22238, 46649, 55169, 83341])]


@pytest.mark.parametrize("key,want", PINS)
def test_the_pinned_permutations(key, want):
    n, seed, col, rep = key
    assert host.perm(seed, col, rep, n)[:len(want)].tolist() == want


def test_the_purpose_lies_outside_the_samplers_and_the_ppcs():
    assert host.lib().permimp_rng() == 0xFFF0 and host.lib().permimp_max_repeats() == perm_mod.MAX_REPEATS == 65535


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 4097, 100000])
def test_it_is_a_bijection(n):
    for seed, col, rep in ((0, 0, 0), (7, 3, 1), (2 ** 64 - 1, 2 ** 31, 65535)):
        got = host.perm(seed, col, rep, n)
        assert np.array_equal(np.sort(got), np.arange(n)), (n, seed, col, rep)
        # a row's donor does not depend on where the range of rows starts
        assert np.array_equal(host.perm(seed, col, rep, n, n // 2, n - n // 2), got[n // 2:])


def test_columns_and_repeats_have_permutations_of_their_own():
    seen = {tuple(host.perm(11, col, rep, 65)) for col in range(6) for rep in range(5)}
    assert len(seen) == 30
    assert tuple(host.perm(12, 0, 0, 65)) not in seen


def test_the_position_table_is_even():
    """A condition, not a measurement: at n = 64 over 6400 keys every (row, donor) cell expects 100; chi-square stays
    below dof + 5 sqrt(2 dof) with dof = 63^2 (4414.5)."""
    table = np.zeros((64, 64))
    rows = np.arange(64)
    for key in range(6400):
        table[rows, host.perm(99, key % 40, key // 40, 64)] += 1
    chi2 = float(((table - 100.0) ** 2 / 100.0).sum())
    dof = 63 ** 2
    print(f"chi-square of the position table: {chi2:.1f}")
    assert chi2 < dof + 5 * np.sqrt(2 * dof)


# ------------------------------------------------------------------ 2. the packer
def _same_lists(pool, fidx, p, cols, picks=None):
    off, lst = host.use_lists(pool, fidx, p, cols, picks)
    woff, wlst = host.recount(pool, fidx, p, cols, picks)
    assert np.array_equal(off, woff) and np.array_equal(lst, wlst)
    return off, lst


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_packer_on_random_histories(seed):
    rng = np.random.default_rng(seed)
    p = 7
    pool = ice_host.random_pool(rng, 30, p, K=2, depth=5, linear=[1, 6] if seed else None, split_cols=[0, 1, 2, 3, 4])
    fidx = np.stack([rng.choice(30, size=9, replace=False) for _ in range(5)]).astype(np.int32)
    _same_lists(pool, fidx, p, list(range(p)))
    _same_lists(pool, fidx, p, [4, 0, 6], picks=[3, 0, 3])


def test_a_regressor_alone_is_a_use_and_an_unused_column_has_an_empty_list():
    rng = np.random.default_rng(5)
    pool = ice_host.random_pool(rng, 12, 6, split_cols=[0, 1, 2], linear=[4])
    fidx = np.arange(12, dtype=np.int32).reshape(2, 6)
    off, lst = _same_lists(pool, fidx, 6, [4, 5, 3])
    lens = np.diff(off).reshape(2, 3)
    assert np.all(lens[:, 0] > 0) and np.all(lens[:, 1:] == 0)
    assert not any(4 in set(pool.var[pool.node_off[t]:pool.node_off[t + 1]].tolist()) for t in range(12))


def test_a_split_that_cannot_be_reached_is_not_a_use_and_a_tree_named_twice_is_listed_twice():
    pool = TreeArrays.empty(2, 7, 1)
    pool.tree_id[:] = [0, 1]
    pool.node_off[:] = [0, 6, 7]
    pool.var[:] = [0, -1, -1, 3, -1, -1, -1]      # tree 0: a split on 0 at the root; a split on 3 nobody points at
    pool.left[0], pool.right[0], pool.left[3], pool.right[3] = 1, 2, 4, 5
    pool.count[:] = 4
    fidx = np.array([[0, 1, 0]], np.int32)
    off, lst = _same_lists(pool, fidx, 4, [3, 0])
    assert off.tolist() == [0, 0, 2] and lst.tolist() == [0, 0]


# ------------------------------------------------------------------ 3. the host reference of the value
def _bound_check(oracle, pool, fidx, X, cols, R, seed):
    """max over the entries of |fperm - pgb_predict(X permuted)| / (gamma_N S): both are roundings of the same exact
    number, N = 2 m + 2, S the sum of the absolute leaf contributions of the four walks (f, A, A', the direct one)."""
    n, p = X.shape
    D, m = fidx.shape
    N = 2 * m + 2
    gamma = N * ex.U / (1 - N * ex.U)
    ref = host.reference(oracle, pool, fidx, X, 0, n, cols, R, seed, np.arange(D), host.PRED)
    off, lst = host.use_lists(pool, fidx, p, cols)
    S_f = ex.walk(pool, fidx, X).S
    worst, differ = Fraction(0), 0
    for s, c in enumerate(cols):
        for r in range(R):
            Xp = host.permuted_matrix(X, c, seed, r)
            direct = host.predict(oracle, pool, fidx, Xp)
            S_d = ex.walk(pool, fidx, Xp).S
            for d in range(D):
                mine = lst[off[d * len(cols) + s]:off[d * len(cols) + s + 1]]
                S_a = ex.walk(pool, mine[None, :], X).S[0] if mine.size else np.full(S_f[d].shape, Fraction(0), object)
                S_ap = ex.walk(pool, mine[None, :], Xp).S[0] if mine.size else S_a
                for k in range(direct.shape[1]):
                    for i in range(n):
                        err = abs(Fraction(float(ref[d, s, r, k, i])) - Fraction(float(direct[d, k, i])))
                        if err == 0:
                            continue
                        differ += 1
                        bound = gamma * (S_f[d, k, i] + S_a[k, i] + S_ap[k, i] + S_d[d, k, i])
                        assert err <= bound, (d, s, r, k, i)
                        worst = max(worst, err / bound)
    return float(worst), differ


def test_the_reference_is_the_prediction_of_the_permuted_matrix_within_the_derived_bound(oracle):
    rng = np.random.default_rng(31)
    pool = ice_host.random_pool(rng, 30, 5, K=2, depth=4, linear=[2])
    fidx = np.stack([rng.choice(30, size=12, replace=False) for _ in range(2)]).astype(np.int32)
    X = rng.normal(size=(40, 5))
    worst, differ = _bound_check(oracle, pool, fidx, X, [0, 2, 4], 2, 77)
    print(f"max |reference - direct| / bound = {worst:.3f} over {differ} entries that differ")


def test_on_dyadic_pools_the_reference_has_the_bits_of_the_direct_prediction(oracle):
    rng = np.random.default_rng(8)
    cols = [0, 1, 2, 3]
    roots = [ex.dyadic_tree(rng, 2, 4, cols, lambda r, j: float(ex.dyadic(r, 2, 1.0)), linear=(1, 4)) for _ in range(10)]
    pool = ex.build_pool(roots, 2)
    fidx = np.stack([rng.choice(10, size=6, replace=False) for _ in range(3)]).astype(np.int32)
    X = ex.dyadic(rng, 2, 1.5, size=(33, 5)).astype(np.float64)
    ex.walk(pool, fidx, X).exact_class()
    ref = host.reference(oracle, pool, fidx, X, 0, 33, [1, 4, 0], 2, 5, np.arange(3), host.PRED)
    delta = host.reference(oracle, pool, fidx, X, 0, 33, [1, 4, 0], 2, 5, np.arange(3), host.DELTA)
    f = host.predict(oracle, pool, fidx, X)
    for s, c in enumerate([1, 4, 0]):
        for r in range(2):
            direct = host.predict(oracle, pool, fidx, host.permuted_matrix(X, c, 5, r))
            assert np.array_equal(ref[:, s, r], direct) and np.array_equal(delta[:, s, r], direct - f)
    assert np.count_nonzero(delta) > 0


# ------------------------------------------------------------------ 4. the Python layer: refusals, order
def _stumps(K, n_trees=3):
    pool = TreeArrays.empty(n_trees, n_trees, K)
    pool.tree_id[:] = np.arange(n_trees)
    pool.node_off[:] = np.arange(n_trees + 1)
    pool.var[:] = -1
    pool.count[:] = 10
    return pool


def _recorded(K=1, draws=5):
    rec = Recorder()
    rec.lib.predict_permuted_entry_point = lambda fn=rec.function("pgb_predict_permuted"): fn
    names = ("pgb_row_reduce", "pgb_row_reduce_finish", "pgb_row_reduce_workspace_bytes")
    rec.lib.rowreduce_entry_points = lambda fns=tuple(rec.function(nm) for nm in names): fns
    s = PosteriorSampler(_stumps(K), np.tile(np.arange(3, dtype=np.int32), (draws, 1)), 3, K, backend=rec)
    return rec, s


def test_argument_errors_are_raised_in_order_before_a_backend_is_touched(monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rec, s = _recorded()
    _, s2 = _recorded(K=2)
    X, y = np.zeros((8, 3)), np.zeros(8)
    cases = [
        (dict(X=np.zeros((2, 2, 2)), transform="cube"), "X must be a matrix"),
        (dict(transform="cube", offset=np.zeros(3)), "unknown transform"),
        (dict(offset=np.zeros(3), draws=[9]), "offset must have shape"),
        (dict(draws=[9], cols=[3]), "draws must index"),
        (dict(draws=[], cols=[3]), "at least 1 draw"),
        (dict(cols=[3], random_seed=-1), "cols must index"),
        (dict(cols=[1, 1], random_seed=-1), "cols must not name a column twice"),
        (dict(cols=[], random_seed=-1), "non-empty vector"),
        (dict(random_seed=-1, n_repeats=0), "random_seed"),
        (dict(n_repeats=0, weights=np.ones(3)), "n_repeats must lie in"),
        (dict(n_repeats=65536), "n_repeats must lie in"),
        (dict(weights=np.ones(3), groups=np.zeros(3)), "weights must hold one value per row"),
        (dict(groups=np.zeros(3), y=np.zeros(3)), "groups must hold one label per row"),
        (dict(y=np.zeros(3)), "y must hold one value per row"),
        (dict(y=None, transform="logistic"), "transform must be 'identity'"),
        (dict(y=None, offset=np.zeros(8)), "without y an offset"),
    ]
    for kw, msg in cases:
        args = dict(X=X, y=y)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            permutation_importance(s, **args)
    with pytest.raises(ValueError, match="y takes a fit with one output"):
        permutation_importance(s2, X, y)
    with pytest.raises(TypeError):
        permutation_importance(object(), X, y)
    assert rec.trace == []


def test_a_column_that_does_not_fit_a_block_is_refused_naming_what_to_cut(monkeypatch):
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")
    rec, s = _recorded(draws=5)
    X = np.zeros((4000, 3))
    with pytest.raises(ValueError, match=r"one column of 5 draws x 7 repeats x 2 groups .* does not fit"):
        permutation_importance(s, X, np.zeros(4000), n_repeats=7, groups=np.arange(4000) % 2)
    assert rec.trace == []


def test_hip_backend_only():
    rec, s = _recorded()
    rec.lib.backend_name = "cpu-oracle"
    with pytest.raises(_abi.PGBError, match="permutation importance runs on the HIP backend only, not on cpu-oracle"):
        permutation_importance(s, np.zeros((8, 3)), np.zeros(8))
    assert rec.trace == []


def test_a_library_without_the_symbol_is_named(oracle):
    with pytest.raises(NotImplementedError, match="pgb_predict_permuted"):
        oracle.lib.predict_permuted_entry_point()


def test_the_calls_and_their_arguments_on_the_recording_backend(monkeypatch):
    """One block of 70 rows, two columns, three repeats, five draws: predict, permute, reduce the fit, reduce the permuted
    predictions, finish both -- with the arguments in the order of the header."""
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rec, s = _recorded()
    with np.errstate(all="ignore"):
        res = permutation_importance(s, np.zeros((70, 4)), np.zeros(70), cols=[3, 1], n_repeats=3, random_seed=9)
    calls = [line for line in rec.trace if line.startswith("pgb_")]
    assert [c.split()[0] for c in calls] == ["pgb_predict", "pgb_predict_permuted", "pgb_row_reduce", "pgb_row_reduce",
                                             "pgb_row_reduce_finish", "pgb_row_reduce_finish"]
    # trees fidx D m X nb p ldx xcols n_total first_row cols q R seed picks n_picks f mode out stream
    assert calls[1].split()[1:] == ["trees:3", "host", "5", "3", "dev:280+0", "70", "4", "4", "dev:140+0", "70", "0", "host",
                                    "2", "3", "9", "host", "5", "dev:350+0", "0", "dev:2100+0", "-"]
    # a b D K nb ld ...: the fit's 5 draws, then the 5 x 2 x 3 permuted ones
    assert calls[2].split()[1:7] == ["dev:350+0", "-", "5", "1", "70", "70"]
    assert calls[3].split()[1:7] == ["dev:2100+0", "-", "30", "1", "70", "70"]
    assert res["mse_permuted"].shape == (5, 2, 3) and res["importance"].shape == (5, 2) and res["cols"].tolist() == [3, 1]
    rec2, s2 = _recorded(K=2)
    with np.errstate(all="ignore"):
        res = permutation_importance(s2, np.zeros((70, 4)), cols=[2], n_repeats=2, groups=np.arange(70) % 3)
    calls = [line for line in rec2.trace if line.startswith("pgb_")]
    assert [c.split()[0] for c in calls] == ["pgb_predict_permuted", "pgb_row_reduce", "pgb_row_reduce_finish"]
    assert calls[0].split()[-4:] == ["-", "1", "dev:1400+0", "-"]          # no f, delta mode
    assert res["shift"].shape == res["sensitivity"].shape == (5, 2, 1, 3)


# ------------------------------------------------------------------ 5. the Python layer: values, chunking, subsets
@pytest.fixture(scope="module")
def small(oracle):
    rng = np.random.default_rng(17)
    pool = ice_host.random_pool(rng, 16, 5, depth=3, split_cols=[0, 1, 3], linear=[3])
    be = host.HostBackend(oracle, pool)
    s = ice_host.pool_sampler(rng, pool, 4, 3, be)
    X = rng.normal(size=(150, 5))
    X[rng.random(X.shape) < 0.05] = np.nan
    y = np.nan_to_num(X[:, 0]) + rng.normal(0, 0.3, 150)
    return be, s, pool, X, y


def test_the_results_against_the_row_reduce_of_the_reference(small, oracle, monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    be, s, pool, X, y = small
    w = np.random.default_rng(2).uniform(0.5, 2.0, 150)
    res = permutation_importance(s, X, y, n_repeats=2, weights=w, random_seed=4)
    f = host.predict(oracle, pool, s.forest_idx, X)
    base = rowred.public(f, w, None, y=y)
    assert np.array_equal(res["mse_base"], base["mse"][:, 0])
    ref = host.reference(oracle, pool, s.forest_idx, X, 0, 150, list(range(5)), 2, 4, np.arange(3), host.PRED)
    want = rowred.public(ref.reshape(-1, 1, 150), w, None, y=y)
    assert np.array_equal(res["mse_permuted"], want["mse"][:, 0].reshape(3, 5, 2))
    assert np.array_equal(res["importance"], res["mse_permuted"].mean(axis=2) - res["mse_base"][:, None])
    assert np.array_equal(res["r2_drop"], base["r2"][:, 0][:, None] - want["r2"][:, 0].reshape(3, 5, 2).mean(axis=2))
    assert np.array_equal(res["importance_mean"], res["importance"].mean(axis=0)) and res["importance_hdi"].shape == (5, 2)
    assert np.all(res["importance"][:, [2, 4]] == 0.0)                    # no tree uses columns 2 and 4
    assert np.any(res["importance"][:, 0] != 0.0) and res["n_nonfinite"] == 0
    assert res["weight"].shape == (1,) and res["group_labels"].tolist() == [0]
    # without y: the shift of the prediction and its second moment
    res = permutation_importance(s, X, n_repeats=2, weights=w, random_seed=4)
    delta = host.reference(oracle, pool, s.forest_idx, X, 0, 150, list(range(5)), 2, 4, np.arange(3), host.DELTA)
    want = rowred.public(delta.reshape(-1, 1, 150), w, None)["mean"][:, 0, 0].reshape(3, 5, 2)
    assert np.array_equal(res["shift"], want.mean(axis=2)) and res["sensitivity"].shape == (3, 5)
    assert np.all(res["shift"][:, [2, 4]] == 0.0) and np.all(res["sensitivity"][:, [2, 4]] == 0.0)


def test_chunks_of_columns_blocks_of_rows_and_subsets_change_no_bit(small, monkeypatch):
    be, s, pool, X, y = small
    groups = np.arange(150) // 75
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    del be.calls[:]
    whole = permutation_importance(s, X, y, n_repeats=3, groups=groups, random_seed=4)
    assert be.calls == [(150, 5)] and whole["mse_permuted"].shape == (3, 5, 3, 2)
    keys = ("mse_permuted", "mse_base", "importance", "importance_mean", "importance_sd", "importance_hdi", "r2_drop")
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")
    del be.calls[:]
    small_blocks = permutation_importance(s, X, y, n_repeats=3, groups=groups, random_seed=4)
    assert max(q for _, q in be.calls) < 5 and max(nb for nb, _ in be.calls) < 150   # chunks of columns, blocks of rows
    for key in keys:
        assert np.array_equal(small_blocks[key], whole[key]), key
    assert small_blocks["n_nonfinite"] == whole["n_nonfinite"]
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    some = permutation_importance(s, X, y, cols=[3, 1], n_repeats=3, groups=groups, random_seed=4)
    assert some["cols"].tolist() == [3, 1]
    for key in keys:
        a = whole[key]
        want = a[[3, 1]] if key in ("importance_mean", "importance_sd", "importance_hdi") else (
            a if key == "mse_base" else a[:, [3, 1]])
        assert np.array_equal(some[key], want), key


# ------------------------------------------------------------------ 6. the timing tool
def test_the_timing_tool_answers_help_and_restates_the_permutation():
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "timing_permimp.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--baseline-root" in r.stdout and "--baseline-cols" in r.stdout
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        import timing_permimp
    finally:
        sys.path.pop(0)
    for key, _ in PINS:                                               # the baseline's NumPy restatement is the header's
        n, seed, col, rep = key
        assert np.array_equal(timing_permimp.perm_index(seed, col, rep, n), host.perm(seed, col, rep, n))
    assert timing_permimp.PERMIMP_RNG == host.lib().permimp_rng()
