"""ICE curves on the MI355X: ``pgb_predict_ice`` (``k_ice``) against the same backend's ``sample_posterior`` on the
explicitly built probe matrix, summed in pick order in a Python loop and divided once (``_ice_host.yardstick``).  The
walk is shared with ``k_predict``, so the comparison is ``np.array_equal``, not a tolerance."""
import numpy as np
import pytest

import _ice_host as host
from pymc_bart_amd import BARTOp, _abi, individual_conditional_expectation
from pymc_bart_amd.chains import sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler, _MultiChainSampler

pytestmark = pytest.mark.gpu

LDS_MAXP = 1024  # PGB_ICE_LDS_MAXP (include/pgbart_ice.h)


# ------------------------------------------------------------------ 1. a short fit
@pytest.fixture(scope="module")
def fits(hip, oracle):
    rng = np.random.default_rng(31)
    X = rng.uniform(-1, 1, size=(130, 4))                        # tiles of 64 + 64 + 2 rows
    Y = 2.0 * X[:, 0] - X[:, 1] ** 2 + rng.normal(0, 0.1, 130)
    ops = {}
    for name, be in (("hip", hip), ("oracle", oracle)):
        ops[name] = BARTOp(X, Y, m=15)
        sample_chain(ops[name], tune=20, draws=10, num_particles=10, random_seed=6, sigma=0.2, backend=be)
    return X, ops


KW = dict(var_idx=[0, 1], instances=4, samples=8, random_seed=2)


def test_a_short_fit(fits, hip, oracle):
    X, ops = fits
    s = _get_posterior_sampler(ops["hip"], backend=hip)
    rng = np.random.default_rng(5)
    inst = X[rng.choice(130, 4, replace=False)]
    picks = rng.integers(0, s.n_draws, size=(2, 4, 8))
    got = s.ice_mean(X, inst, [0, 1], picks)
    assert got.shape == (2, 4, 1, 130) and np.array_equal(got, host.yardstick(s, X, inst, [0, 1], picks))
    # the public function: the curves of its own picks, centred; and the oracle backend's numbers
    pub = individual_conditional_expectation(ops["hip"], X, backend=hip, **KW)
    r2 = np.random.default_rng(2)
    chosen = r2.choice(130, replace=False, size=4)
    pk = np.array([[r2.integers(0, s.n_draws, size=8) for _ in range(4)] for _ in range(2)])
    want = host.yardstick(s, X, X[chosen], [0, 1], pk)
    assert np.array_equal(pub["instances"], chosen)
    for c, j in enumerate((0, 1)):
        raw = np.moveaxis(want[c], 1, 2)
        assert pub["ice"][j].shape == (4, 130, 1) and np.array_equal(pub["ice"][j], raw - raw[:, :1, :])
    ref = individual_conditional_expectation(ops["oracle"], X, backend=oracle, **KW)
    for j in (0, 1):
        np.testing.assert_allclose(pub["ice"][j], ref["ice"][j], rtol=0, atol=1e-12)


def test_the_public_call_does_not_predict_probe_matrices(fits, hip, monkeypatch):
    X, ops = fits
    want = individual_conditional_expectation(ops["hip"], X, backend=hip, **KW)

    def refuse(self, *a, **k):
        raise AssertionError("sample_posterior was called")

    monkeypatch.setattr(PosteriorSampler, "sample_posterior", refuse)
    monkeypatch.setattr(_MultiChainSampler, "sample_posterior", refuse)
    got = individual_conditional_expectation(ops["hip"], X, backend=hip, **KW)
    for j in (0, 1):
        assert np.array_equal(got["ice"][j], want["ice"][j])


def test_against_the_probe_matrix_implementation(fits, hip):
    """The implementation the fused call replaced takes ``np.mean`` over the draws: two summation orders differ by at
    most samples * 2^-52 * max |sum| in the sum, that is by samples * 2^-52 * max |mean| in the mean compared here (an
    axis-0 mean of a C-contiguous array adds in order, so equality is what to expect)."""
    X, ops = fits
    kw = dict(KW, centered=False)
    got = individual_conditional_expectation(ops["hip"], X, backend=hip, **kw)
    old = host.ice_by_probe_matrices(ops["hip"], X, backend=hip, **kw)
    assert np.array_equal(got["instances"], old["instances"])
    for j in (0, 1):
        bound = kw["samples"] * 2.0 ** -52 * float(np.max(np.abs(old["ice"][j])))
        diff = float(np.max(np.abs(got["ice"][j] - old["ice"][j])))
        print(f"column {j}: max |new - old| = {diff:.3e} (bound {bound:.3e})")
        assert diff <= bound


# ------------------------------------------------------------------ 2. hand-built pools: every path of the walk
def _data(rng, n, p, rules=None):
    X = rng.normal(size=(n, p))
    for j, r in enumerate([] if rules is None else rules):
        if r == _abi.RULE_ONEHOT:
            X[:, j] = rng.integers(0, 4, n)
        elif r == _abi.RULE_SUBSET:
            X[:, j] = rng.integers(0, 8, n)
    return X


def _check(s, X, inst, cols, picks):
    got = s.ice_mean(X, inst, cols, picks)
    want = host.yardstick(s, X, inst, cols, picks)
    assert got.shape == want.shape == (len(cols), inst.shape[0], s.n_outputs, X.shape[0])
    assert np.array_equal(got, want, equal_nan=True) and not np.isnan(got).any()
    return got


CASES = ["cont", "rules", "nan_sweep", "nan_inst", "nan_both", "rules_nan", "linear", "k3", "deep", "never_meets"]


@pytest.mark.parametrize("m", [5, 7])        # the grouped walk (4 trees at a time) and its tail
@pytest.mark.parametrize("case", CASES)
def test_hand_built_pools(hip, case, m):
    rng = np.random.default_rng(1000 + 10 * m + CASES.index(case))
    p, n, K = 5, 130, 1
    rules = None
    kw = {}
    if case in ("rules", "rules_nan"):
        rules = [0, _abi.RULE_ONEHOT, _abi.RULE_SUBSET, 0, 0]    # CONT false
    if case == "linear":
        kw["linear"] = [0, 3]                                    # the swept column 0 and another one
    if case == "nan_both":
        kw["linear"] = [0, 1]                                    # regressors that are missing: the leaf's mean
    if case == "k3":
        K, kw["linear"] = 3, [1]
    if case == "deep":
        kw.update(depth=12, chain=True)
    if case == "never_meets":
        kw["split_cols"] = [1, 2, 3]                             # column 0 and 4 are swept, no tree splits on them
    pool = host.random_pool(rng, 24, p, K=K, rules=rules, **kw)
    if case == "deep":
        sizes = np.diff(pool.node_off)
        assert sizes.max() >= 2 * 9 + 1                          # a chain deeper than 8 levels
    s = host.pool_sampler(rng, pool, m, 6, hip)
    X = _data(rng, n, p, rules)
    inst = X[rng.choice(n, 3, replace=False)].copy()
    cols = [0, 2, 4]
    if case in ("nan_sweep", "nan_both", "rules_nan"):
        X[rng.random(n) < 0.2, 0] = np.nan
        X[7, 2] = np.nan                                         # one lane of one wave
    if case in ("nan_inst", "nan_both", "rules_nan"):
        inst[0, 1] = np.nan
        inst[1, [0, 3]] = np.nan                                 # (column 0 is replaced when it is the swept one)
    picks = rng.integers(0, s.n_draws, size=(3, 3, 4))
    got = _check(s, X, inst, cols, picks)
    if case == "never_meets":                                    # nothing on any path tests the swept column
        assert np.all(got[0] == got[0][..., :1]) and np.all(got[2] == got[2][..., :1])
        assert not np.all(got[1] == got[1][..., :1])


def test_pick_and_row_counts(hip):
    rng = np.random.default_rng(77)
    pool = host.random_pool(rng, 20, 4, linear=[2])
    s = host.pool_sampler(rng, pool, 7, 5, hip)
    X = _data(rng, 65, 4)
    inst = X[[3, 60]].copy()
    _check(s, X, inst, [1, 2], rng.integers(0, 5, size=(2, 2, 1)))                # n_picks = 1, 65 rows
    rep = np.tile(np.array([2, 2, 4, 2, 2, 2, 4, 4, 2]), (2, 2, 1))              # repeated picks
    _check(s, X, inst, [1, 2], rep)
    _check(s, X[:1], inst, [0, 3], rng.integers(0, 5, size=(2, 2, 3)))            # n_rows = 1
    nine = _check(s, X, inst, [1], np.full((1, 2, 9), 3))                          # nine times the same draw ...
    once = _check(s, X, inst, [1], np.full((1, 2, 1), 3))
    # ... is that draw, up to the roundings of eight additions and one division
    np.testing.assert_allclose(nine, once, rtol=10 * 2.0 ** -53, atol=0)


@pytest.mark.parametrize("cont", [True, False])
def test_instance_rows_wider_than_the_lds_cap(hip, cont):
    """p = PGB_ICE_LDS_MAXP + 6: the instances that read the instance row from global memory."""
    rng = np.random.default_rng(9 + cont)
    p, n = LDS_MAXP + 6, 70
    rules = np.zeros(p, np.int32)
    if not cont:
        rules[3], rules[p - 2] = _abi.RULE_ONEHOT, _abi.RULE_SUBSET
    used = [0, 3, 500, LDS_MAXP - 1, LDS_MAXP, p - 2, p - 1]
    pool = host.random_pool(rng, 16, p, rules=rules, split_cols=used, linear=[p - 1, 0])
    s = host.pool_sampler(rng, pool, 7, 4, hip)
    X = _data(rng, n, p, rules)
    inst = X[[1, 69]].copy()
    inst[1, 500] = np.nan
    X[5, p - 1] = np.nan
    _check(s, X, inst, [p - 1, 0, 3], rng.integers(0, 4, size=(3, 2, 3)))


def test_three_outputs_without_linear_leaves(hip):
    rng = np.random.default_rng(12)
    pool = host.random_pool(rng, 12, 3, K=3)
    s = host.pool_sampler(rng, pool, 5, 4, hip)
    X = _data(rng, 70, 3)
    _check(s, X, X[[0, 69]].copy(), [2, 1], rng.integers(0, 4, size=(2, 2, 5)))


# ------------------------------------------------------------------ 3. two chains, one pool
def test_two_chains_pooled(hip):
    rng = np.random.default_rng(21)
    a = host.pool_sampler(rng, host.random_pool(rng, 14, 4), 7, 5, hip)
    b = host.pool_sampler(rng, host.random_pool(rng, 18, 4, depth=6), 7, 3, hip)
    s = _MultiChainSampler([a, b])
    assert s.n_draws == 8
    X = _data(rng, 100, 4)
    inst = X[[4, 50, 99]].copy()
    picks = np.empty((2, 3, 6), np.int64)
    picks[:, :, 0::2] = rng.integers(0, 5, size=(2, 3, 3))       # chain a ...
    picks[:, :, 1::2] = rng.integers(5, 8, size=(2, 3, 3))       # ... and chain b, alternating
    got = _check(s, X, inst, [3, 0], picks)
    assert s.pooled_history() is s.pooled_history()              # built once
    only_b = _check(s, X, inst, [3, 0], picks[:, :, 1::2])
    assert np.array_equal(only_b, b.ice_mean(X, inst, [3, 0], picks[:, :, 1::2] - 5)) and not np.array_equal(got, only_b)


# ------------------------------------------------------------------ 4. blocks of columns
def test_results_do_not_depend_on_the_blocking(hip, monkeypatch):
    rng = np.random.default_rng(33)
    pool = host.random_pool(rng, 12, 4, K=2)
    s = host.pool_sampler(rng, pool, 5, 4, hip)
    X = _data(rng, 1500, 4)                                      # 8 * 3 * 2 * 1500 = 72 000 bytes per column
    inst = X[[0, 700, 1499]].copy()
    picks = rng.integers(0, 4, size=(3, 3, 4))
    monkeypatch.delenv("PGB_ICE_BLOCK_BYTES", raising=False)
    whole = s.ice_mean(X, inst, [0, 1, 3], picks)
    monkeypatch.setenv("PGB_ICE_BLOCK_BYTES", "65536")
    calls = []
    real = hip.lib.ice_entry_point

    def counting():
        f = real()
        return lambda *a: (calls.append(a[12]), f(*a))[1]

    monkeypatch.setattr(hip.lib, "ice_entry_point", counting)
    blocked = s.ice_mean(X, inst, [0, 1, 3], picks)
    assert calls == [1, 1, 1] and np.array_equal(whole, blocked)
    assert np.array_equal(whole[:, :, :, :130], host.yardstick(s, X[:130], inst, [0, 1, 3], picks))


# ------------------------------------------------------------------ 5. more curves than a grid dimension holds
def test_more_instances_and_columns_than_the_grid_dimensions(hip):
    """The grid's y (instances) and z (columns) hold 65535 each; the kernel strides over the rest, restaging the
    instance row.  One sweep row, the same picks for every curve: one ``sample_posterior`` call on the matrix of all
    probe rows is the yardstick."""
    rng = np.random.default_rng(55)
    pool = host.random_pool(rng, 10, 3, linear=[1])
    s = host.pool_sampler(rng, pool, 5, 4, hip)
    many = 65535 + 5
    x = rng.normal(size=(1, 3))
    pk = np.array([3, 0, 3])

    def want(probe):                                             # (n_picks, 1, many) -> the pick-order mean per probe row
        pred = s.sample_posterior(probe, pk.tolist(), None)
        return ((pred[0] + pred[1]) + pred[2]) / 3.0

    inst = rng.normal(size=(many, 3))
    inst[::1000, 2] = np.nan
    probe = inst.copy()
    probe[:, 1] = x[0, 1]
    got = s.ice_mean(x, inst, [1], np.tile(pk, (1, many, 1)))
    assert got.shape == (1, many, 1, 1) and np.array_equal(got[0, :, 0, 0], want(probe)[0])
    one = rng.normal(size=(1, 3))                                # ... and as many curve families of one instance
    got = s.ice_mean(x, one, [1] * many, np.tile(pk, (many, 1, 1)))
    probe = one.copy()
    probe[:, 1] = x[0, 1]
    assert got.shape == (many, 1, 1, 1) and np.all(got[:, 0, 0, 0] == want(probe)[0, 0])
