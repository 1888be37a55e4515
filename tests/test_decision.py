"""Optimal arm and policy value, the parts that need no GPU: the packer of the union use lists of
``include/pgbart_arms.h`` against a NumPy recount, the whole of ``optimal_arm`` on a pool whose sums are exact against
NumPy computed from plain oracle predictions on copies of ``X`` (bit for bit: the check that the definition is the right
one), the argmax rule at its edges, and the Python layer on a backend made of the host references
(``_arms_host.HostBackend``) -- its blocking, its refusals, its counters."""
import json
import os

import numpy as np
import pytest

import _arms_host as host
import _ice_host as ice_host
import _permimp_host as permimp
import _predict_exact as ex
from pymc_bart_amd import _abi, arm_predictions, optimal_arm
from pymc_bart_amd import decision as dec
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_ROW = ("p_best", "mean_utility", "expected_regret", "bayes_arm")
PER_DRAW = ("value_optimal", "value_bayes", "regret_bayes", "value_arm", "share_best")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same(got, want, keys):
    for key in keys:
        assert np.array_equal(bits(got[key]), bits(want[key])), (key, got[key], want[key])


def _sampler(oracle, pool, table):
    table = np.ascontiguousarray(table, np.int32)
    be = host.HostBackend(oracle, pool)
    return be, PosteriorSampler(pool, table, table.shape[1], pool.n_outputs, backend=be)


# ------------------------------------------------------------------ 1. the header's constants and the packer
def test_the_constants_of_the_header_are_the_modules():
    L = host.lib()
    assert L.arms_max_cols() == dec.MAX_COLS == 16 and L.arms_max() == dec.MAX_ARMS == 64
    for D, G, A in ((1, 1, 1), (3, 2, 5), (1, 4096, 2), (7, 3, 64)):
        assert 8 * host.ws_doubles(D, G, A) == dec.workspace_bytes(D, G, A)


def _same_lists(pool, fidx, p, cols, picks=None):
    off, lst = host.union_lists(pool, fidx, p, cols, picks)
    woff, wlst = host.recount(pool, fidx, p, cols, picks)
    assert np.array_equal(off, woff) and np.array_equal(lst, wlst)
    return off, lst


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_packer_on_random_histories_with_linear_leaves(seed):
    rng = np.random.default_rng(seed)
    p = 7
    pool = ice_host.random_pool(rng, 30, p, K=2, depth=4, linear=[1, 6] if seed else None, split_cols=[0, 1, 2, 3, 4])
    fidx = np.stack([rng.choice(30, size=9, replace=False) for _ in range(5)]).astype(np.int32)
    off, _ = _same_lists(pool, fidx, p, [4, 6], picks=[3, 0, 3])
    assert 0 < off[-1] < 27 and off[1] - off[0] == off[3] - off[2]
    _same_lists(pool, fidx, p, list(range(p)))
    assert np.diff(_same_lists(pool, fidx, p, [5])[0]).tolist() == [0] * 5   # nobody splits or regresses on column 5
    for c in range(p):                                                       # s = 1: pgb_permimp_pack_build's list
        off1, lst1 = host.union_lists(pool, fidx, p, [c])
        poff, plst = permimp.use_lists(pool, fidx, p, [c])
        assert np.array_equal(off1, poff) and np.array_equal(lst1, plst)
    if seed:                                                                 # a regressor alone is a use
        only = _same_lists(pool, fidx, p, [6])[0]
        assert only[-1] > 0 and not np.any(np.asarray(pool.var) == 6)


def test_a_split_that_cannot_be_reached_is_not_a_use_and_a_tree_named_twice_is_listed_twice():
    pool = TreeArrays.empty(2, 7, 1)
    pool.tree_id[:] = [0, 1]
    pool.node_off[:] = [0, 6, 7]
    pool.var[:] = [0, -1, -1, 3, -1, -1, -1]      # tree 0: a split on 0 at the root; a split on 3 nobody points at
    pool.left[0], pool.right[0], pool.left[3], pool.right[3] = 1, 2, 4, 5
    pool.count[:] = 4
    fidx = np.array([[0, 1, 0], [1, 1, 0]], np.int32)
    off, lst = _same_lists(pool, fidx, 4, [3])
    assert off.tolist() == [0, 0, 0]
    off, lst = _same_lists(pool, fidx, 4, [3, 0], picks=[0, 1, 0])
    assert off.tolist() == [0, 2, 3, 5] and lst.tolist() == [0, 0, 0, 0, 0]


# ------------------------------------------------------------------ 2. the exact pool
def _exact_tree(rng, K, depth, cols, level=0):
    """Leaf values that are integers times 2^-8 within +-4; continuous splits."""
    if level >= depth or (level > 0 and rng.random() > 0.8):
        return ex.Leaf(ex.dyadic(rng, 8, 4.0, K))
    j = int(rng.choice(cols))
    return ex.Split(j, float(rng.normal(0, 0.7)), _exact_tree(rng, K, depth, cols, level + 1),
                    _exact_tree(rng, K, depth, cols, level + 1))


@pytest.fixture(scope="module")
def exact(oracle):
    rng = np.random.default_rng(11)
    K, p = 2, 5
    pool = ex.build_pool([_exact_tree(rng, K, 4, [0, 1, 2, 3]) for _ in range(20)], K)
    table = np.stack([rng.choice(20, size=8, replace=False) for _ in range(5)]).astype(np.int32)
    be, s = _sampler(oracle, pool, table)
    X = rng.normal(size=(150, p))
    return be, s, pool, table, X


@pytest.mark.parametrize("maximize", [True, False])
def test_the_exact_pool_equals_numpy_on_plain_predictions_of_copies_bit_for_bit(oracle, exact, maximize, monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    be, s, pool, table, X = exact
    rng = np.random.default_rng(12)
    cols = [2, 0]
    arms = np.array([[-1.0, 0.5], [0.25, -0.75], [1.5, 1.5], [0.25, -0.75]])
    n = X.shape[0]
    w = rng.integers(0, 17, n) / 4.0                                     # dyadic weights, some of them 0
    groups = rng.integers(0, 3, n)
    policy = rng.integers(0, 4, n)
    cost = np.array([0.0, 0.125, -0.5, 0.125])
    plain = np.stack([permimp.predict(oracle, pool, table, host.arm_copy(X, cols, a)) for a in arms])   # (A, D, K, n)
    got = arm_predictions(s, X, cols, arms)
    assert got.shape == (4, 5, 2, n) and np.array_equal(bits(got), bits(plain))
    assert len({tuple(r) for r in np.argmax(plain[:, :, 1], axis=0).T.tolist()}) > 3   # the arms do compete
    for output in (0, 1):
        res = optimal_arm(s, X, cols, arms, output=output, cost=cost, maximize=maximize, weights=w, groups=groups, policy=policy)
        want = host.numpy_decision(plain[:, :, output], w, groups, 3, policy, cost, 1.0 if maximize else -1.0)
        same(res, want, PER_ROW + PER_DRAW + ("value_policy", "group_weight"))
        assert res["n_nonfinite"] == 0 and res["bayes_arm"].dtype == np.int32 and res["group_labels"].tolist() == [0, 1, 2]
        off, _ = host.union_lists(pool, table, 5, cols)
        assert res["n_list_trees"].tolist() == np.diff(off).tolist() and 0 < res["n_list_trees"].max() <= 8
        assert np.all(res["p_best"][:, 3] == 0.0)                        # arm 3 repeats arm 1: the lower index wins every tie
        for key in PER_DRAW + ("value_policy",):
            assert np.array_equal(bits(res[key + "_mean"]), bits(res[key].mean(axis=0)))
            assert res[key + "_hdi"].shape == res[key].shape[1:] + (2,) and res[key + "_sd"].shape == res[key].shape[1:]
    assert np.allclose(res["p_best"].sum(axis=1), 1.0) and np.all(res["expected_regret"] >= 0.0)
    assert np.all(res["regret_bayes"] >= 0.0) and np.allclose(res["share_best"].sum(axis=-1), 1.0)


def test_one_output_drops_the_k_axis_and_defaults_are_ones_one_group_no_policy(oracle, monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rng = np.random.default_rng(13)
    pool = ex.build_pool([_exact_tree(rng, 1, 3, [0, 1]) for _ in range(6)], 1)
    table = np.arange(6, dtype=np.int32).reshape(2, 3)
    be, s = _sampler(oracle, pool, table)
    X = rng.normal(size=(70, 2))
    arms = [-0.5, 0.5, 2.0]
    plain = np.stack([permimp.predict(oracle, pool, table, host.arm_copy(X, [1], [a]))[:, 0] for a in arms])
    got = arm_predictions(s, X, 1, arms)
    assert got.shape == (3, 2, 70) and np.array_equal(bits(got), bits(plain))
    res = optimal_arm(s, X, 1, arms)
    want = host.numpy_decision(plain, np.ones(70), np.zeros(70, np.int64), 1)
    same(res, want, PER_ROW + PER_DRAW)
    assert "value_policy" not in res and res["value_arm"].shape == (2, 1, 3) and res["group_weight"].tolist() == [70.0]
    some = optimal_arm(s, X, 1, arms, draws=[1])
    assert np.array_equal(bits(some["value_arm"]), bits(res["value_arm"][[1]]))


# ------------------------------------------------------------------ 3. the argmax rule
def _rule(u):
    """The best arm of one vector of utilities, from the header's words."""
    best = 0
    for a in range(1, len(u)):
        if u[a] > u[best] or (np.isnan(u[best]) and not np.isnan(u[a])):
            best = a
    return best


def test_better_is_the_headers_rule():
    L = host.lib()
    inf, nan = np.inf, np.nan
    for a, b, want in ((1.0, 0.0, 1), (0.0, 1.0, 0), (1.0, 1.0, 0), (inf, inf, 0), (nan, 1.0, 0), (1.0, nan, 1), (nan, nan, 0),
                       (-inf, nan, 1), (0.0, -0.0, 0), (-inf, -inf, 0)):
        assert L.arms_better(a, b) == want, (a, b)


def test_ties_nan_and_infinities_in_the_decide_step():
    rng = np.random.default_rng(21)
    A, D, n = 5, 4, 70
    f = rng.integers(-2, 3, (A, D, n)) / 2.0                             # many ties
    f[4] = f[1]                                                          # two identical arms
    f[:, 0, 3], f[:, 2, 5], f[2, 1, 7], f[0, :, 9] = np.nan, np.nan, np.nan, np.nan   # all-NaN (d, i); single NaN; NaN arm 0
    f[1, 3, 11], f[3, 3, 11], f[2, 0, 12], f[0, 0, 13] = np.inf, np.inf, -np.inf, np.inf
    w, g = np.ones(n), np.zeros(n, np.int32)
    r = host.decide(f, w, g, 1)
    best = np.array([[_rule(f[:, d, i]) for i in range(n)] for d in range(D)])
    assert np.array_equal(r["nbest"], np.stack([(best == a).sum(axis=0) for a in range(A)]).astype(np.int32))
    assert np.all(r["nbest"][4] == 0) and best[0, 3] == 0 and best[2, 5] == 0 and best[3, 11] == 1 and best[0, 9] != 0
    assert r["counts"].tolist() == [int((~np.isfinite(f)).sum()), 0, 0]
    assert np.isnan(r["mean"][:, 3]).all() and np.isnan(r["regret"][:, 3]).all() and r["bayes"][3] == 0
    assert r["bayes"][9] != 0 and np.isnan(r["mean"][0, 9]) and not np.isnan(r["mean"][r["bayes"][9], 9])
    clean = [i for i in range(n) if np.all(np.isfinite(f[:, :, i]))]
    su = f.sum(axis=1)
    assert r["bayes"][clean].tolist() == [_rule(su[:, i]) for i in clean]
    whole = host.decide(f, w, g, 1, whole_call=True)
    for key in ("nbest", "mean", "regret", "bayes", "out", "W"):
        assert np.array_equal(r[key], whole[key], equal_nan=True), key


def test_exp_overflow_gives_infinities_on_several_arms_and_the_lowest_index_wins():
    f = np.zeros((3, 2, 64))
    f[1], f[2] = 800.0, 900.0                                            # exp overflows on both
    r = host.decide(f, np.ones(64), np.zeros(64, np.int32), 1, transform="exp")
    assert np.all(r["nbest"][1] == 2) and np.all(r["nbest"][[0, 2]] == 0) and np.all(r["bayes"] == 1)
    assert r["counts"].tolist() == [2 * 2 * 64, 0, 0] and np.all(np.isinf(r["mean"][1:])) and np.all(r["mean"][0] == 1.0)
    assert np.all(r["regret"][0] == np.inf) and np.all(np.isnan(r["regret"][1:]))   # inf - inf
    assert np.all(r["out"][0] == np.inf) and np.all(r["out"][4 + 3 + 1] == 1.0)    # value_optimal; share_best[1]


def test_an_arm_on_an_unused_column_changes_nothing_and_arm_0_wins_everywhere(oracle, monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rng = np.random.default_rng(22)
    pool = ice_host.random_pool(rng, 10, 4, depth=3, split_cols=[0, 1, 2])
    table = np.stack([rng.choice(10, size=4, replace=False) for _ in range(3)]).astype(np.int32)
    be, s = _sampler(oracle, pool, table)
    X = rng.normal(size=(66, 4))
    X[3::7, 0] = np.nan
    res = optimal_arm(s, X, [3], [[-1.0], [np.nan], [np.inf]])
    assert res["n_list_trees"].tolist() == [0, 0, 0] and np.all(res["p_best"][:, 0] == 1.0) and np.all(res["bayes_arm"] == 0)
    assert np.all(bits(res["expected_regret"]) == 0) and np.all(res["share_best"][..., 0] == 1.0)
    f = permimp.predict(oracle, pool, table, X)[:, 0]
    assert np.array_equal(bits(arm_predictions(s, X, [3], [[7.0]])[0]), bits(f + 0.0))


def test_an_arm_equal_to_the_rows_own_values_returns_f_and_minus_zero_becomes_plus_zero(oracle):
    rng = np.random.default_rng(23)
    pool = ice_host.random_pool(rng, 10, 4, K=2, depth=4, linear=[1])
    table = np.stack([rng.choice(10, size=5, replace=False) for _ in range(2)]).astype(np.int32)
    X = np.tile(rng.normal(size=(1, 4)), (40, 1))                        # every row the same: an arm can equal all of them
    X[:, 3] = rng.normal(size=40)
    got, lens = host.reference_block(oracle, pool, table, X, [0, 1], [X[0, :2], [0.3, -0.2]], [0, 1])
    f = permimp.predict(oracle, pool, table, X)
    assert lens.min() > 0 and np.array_equal(bits(got[0]), bits(f)) and not np.array_equal(got[1], f)
    # f itself is never -0.0 (a sum that starts from +0.0); handed in by a caller it comes out as +0.0
    got, _ = host.reference_block(oracle, pool, table, X, [0, 1], [X[0, :2]], [0, 1], f=np.full(f.shape, -0.0))
    assert np.all(bits(got) == 0)


# ------------------------------------------------------------------ 4. blocking, scaling, counters
@pytest.fixture(scope="module")
def small(oracle):
    rng = np.random.default_rng(31)
    rules = [0, _abi.RULE_ONEHOT, 0, _abi.RULE_SUBSET, 0]
    pool = ice_host.random_pool(rng, 16, 5, K=2, depth=4, rules=rules, linear=[2])
    be = host.HostBackend(oracle, pool)
    s = ice_host.pool_sampler(rng, pool, 6, 4, be)
    X = rng.normal(size=(300, 5))
    X[:, 1], X[:, 3] = rng.integers(0, 4, 300), rng.integers(0, 8, 300)
    X[rng.random((300, 5)) < 0.04] = np.nan
    kw = dict(cols=[1, 3, 2], arms=[[0, 1, -0.5], [2, 5, 0.25], [3, np.nan, 1.5], [np.nan, 7, -2.0]], output=1,
              transform="logistic", offset=rng.normal(0, 0.3, 300), cost=[0.0, 0.01, 0.02, 0.005],
              weights=rng.uniform(0.5, 2.0, 300), groups=rng.integers(0, 2, 300), policy=rng.integers(0, 4, 300))
    return be, s, X, kw


def test_the_blocking_at_its_floor_changes_no_bit(small, monkeypatch):
    be, s, X, kw = small
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    del be.calls[:]
    whole = optimal_arm(s, X, **kw)
    preds = arm_predictions(s, X, kw["cols"], kw["arms"])
    assert be.calls == [300, 300] and whole["n_nonfinite"] == 0
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")
    del be.calls[:]
    blocked = optimal_arm(s, X, **kw)
    assert len(be.calls) >= 3 and all(nb % 64 == 0 for nb in be.calls[:-1]) and sum(be.calls) == 300
    same(blocked, whole, PER_ROW + PER_DRAW + ("value_policy", "group_weight"))
    for key in PER_DRAW + ("value_policy",):
        same(blocked, whole, [key + "_mean", key + "_sd", key + "_hdi"])
    assert np.array_equal(bits(arm_predictions(s, X, kw["cols"], kw["arms"])), bits(preds))
    assert len(set(whole["bayes_arm"].tolist())) > 1


def test_a_power_of_two_scaling_of_the_weights_changes_no_bit(small, monkeypatch):
    be, s, X, kw = small
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    whole = optimal_arm(s, X, **kw)
    scaled = optimal_arm(s, X, **dict(kw, weights=kw["weights"] * 2.0 ** -7))
    same(scaled, whole, PER_ROW + PER_DRAW + ("value_policy",))
    assert np.array_equal(bits(scaled["group_weight"]), bits(whole["group_weight"] * 2.0 ** -7))


def test_a_bad_group_and_a_bad_policy_are_counted_left_out_and_refused_at_the_finish():
    rng = np.random.default_rng(41)
    A, D, n, G = 3, 3, 140, 2
    f = rng.normal(size=(A, D, n))
    w = rng.uniform(0.5, 2.0, n)
    g, pi = rng.integers(0, G, n).astype(np.int32), rng.integers(0, A, n).astype(np.int32)
    bad_g, bad_pi = [3, 64, 70, 139], [5, 70, 100]
    g2, pi2 = g.copy(), pi.copy()
    g2[bad_g], pi2[bad_pi] = [-1, G, 7, -5], [A, -1, 99]
    r = host.decide(f, w, g2, G, policy=pi2, chunk=64)
    assert r["counts"].tolist() == [0, 4, 3]
    w0 = w.copy()
    w0[sorted(set(bad_g + bad_pi))] = 0.0                                # the same sums: a term of weight 0 adds +0.0
    ok = host.decide(f, w0, g, G, policy=pi, chunk=64)
    assert ok["counts"].tolist() == [0, 0, 0]
    for key in ("nbest", "bayes"):
        assert np.array_equal(r[key], ok[key]), key
    same(r, ok, ("mean", "regret", "out", "W"))
    for pol, counts in ((pi2, [0, 4, 3]), (None, [0, 4, 0])):
        r = host.decide(f, w, g2, G, policy=pol)
        assert r["counts"].tolist() == counts
    r = host.decide(f, w, g, G, policy=pi2, chunk=128)
    assert r["counts"].tolist() == [0, 0, 3]


# ------------------------------------------------------------------ 5. the refusals of the Python layer
def test_every_refusal_of_the_python_layer(small, monkeypatch):
    be, s, X, kw = small
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    del be.calls[:]
    n = X.shape[0]
    zero_group = kw["weights"].copy()
    zero_group[kw["groups"] == 1] = 0.0
    cases = [
        (dict(cols=[1, 5, 2]), "cols must index the 5 columns"), (dict(cols=[1, 3, 1]), "cols must not name a column twice"),
        (dict(cols=[]), "cols must be a non-empty vector"),
        (dict(arms=[[0, 1], [2, 3]]), r"arms must have shape \(n_arms, 3\)"), (dict(arms=np.zeros((0, 3))), "arms must have shape"),
        (dict(arms=np.zeros((65, 3))), "at most 64 arms"), (dict(arms=[["a", "b", "c"]]), "arms must be a matrix of numbers"),
        (dict(output=2), r"output must be an integer in \[0, 2\)"), (dict(output=-1), "output must be an integer"),
        (dict(output=0.0), "output must be an integer"), (dict(transform="log"), "unknown transform 'log'"),
        (dict(offset=np.zeros(n - 1)), "offset must hold one value per row"), (dict(offset=np.full(n, np.nan)), "offset must be finite"),
        (dict(cost=[0.0, 1.0]), r"cost must hold one value per arm: shape \(4,\)"), (dict(cost=[0, 1, np.inf, 2]), "cost must be finite"),
        (dict(weights=np.ones(n - 1)), "weights must hold one value per row"), (dict(weights=-np.ones(n)), "weights must be finite and >= 0"),
        (dict(weights=zero_group), "group 1 has total weight 0"), (dict(groups=np.zeros(n + 1)), "groups must hold one label per row"),
        (dict(policy=np.full(n, 4)), "policy must index the 4 arms"), (dict(policy=np.full(n, -1)), "policy must index the 4 arms"),
        (dict(policy=np.zeros(n)), "policy must hold one arm index per row"), (dict(policy=np.zeros(n - 1, int)), "policy must hold one arm"),
        (dict(draws=[4]), "draws must index the 4 stored draws"), (dict(draws=[]), "a decision needs at least 1 draw"),
        (dict(hdi_prob=1.0), "hdi_prob must lie in"),
    ]
    for change, msg in cases:
        with pytest.raises(ValueError, match=msg):
            optimal_arm(s, X, **dict(kw, **change))
    with pytest.raises(ValueError, match="at most 16 columns per arm"):
        optimal_arm(s, np.zeros((4, 20)), list(range(17)), np.zeros((2, 17)))
    with pytest.raises(ValueError, match=r"X must be a matrix"):
        arm_predictions(s, np.zeros((3, 2, 2)), [0], [0.0])
    with pytest.raises(ValueError, match="arms must have shape"):
        arm_predictions(s, X, [0, 1], [0.0, 1.0])
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")
    with pytest.raises(ValueError, match=r"the partial sums of 4 draws x 300 groups x 4 arms take \d+ bytes"):
        optimal_arm(s, X, **dict(kw, groups=np.arange(n)))
    assert be.calls == []


def test_the_cpu_oracle_is_refused_naming_the_entry_point(oracle, small):
    be, s, X, kw = small
    with pytest.raises(NotImplementedError, match="pgb_predict_arms"):
        optimal_arm(s, X, backend=oracle, **kw)
    with pytest.raises(NotImplementedError, match="pgb_predict_arms"):
        arm_predictions(s, X, [0], [1.0], backend=oracle)
    with pytest.raises(NotImplementedError, match="pgb_arms_kernel_ms"):
        oracle.lib.arms_kernel_ms()


# ------------------------------------------------------------------ 6. the budget and the timing tool
def test_the_instances_are_in_the_occupancy_budget_with_no_scratch_beyond_the_walks():
    budget = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    walk = budget["k_ale<true, true>"]["max_scratch_bytes"]            # the walk's two stacks
    for name in ("k_arms<false, false>", "k_arms<false, true>", "k_arms<true, false>", "k_arms<true, true>"):
        assert budget[name]["max_scratch_bytes"] == walk and budget[name]["max_vgpr_spills"] == 0, name
    for name in ("k_arms_best", "k_arms_rows", "k_arms_bayes", "k_arms_reduce", "k_arms_finish"):
        assert budget[name]["max_scratch_bytes"] == 0 and budget[name]["max_vgpr_spills"] == 0, name


def test_the_timing_tool_answers_help():
    import subprocess
    import sys

    tool = os.path.join(ROOT, "tools", "timing_decision.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--baseline-root" in r.stdout
