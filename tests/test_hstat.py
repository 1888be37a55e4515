"""Friedman's H-statistic without a GPU: ``include/pgbart_hstat.h`` compiled for the host (``tests/_hstat_host.py``)
against a brute-force reference written from the definition -- the ``n_e x n_b`` hybrid rows predicted by the exact
rational walk of ``_predict_exact`` -- the facts the header promises exactly, a hand-built forest with a closed-form
answer, and the Python layer on a backend made of the host references.

The one tolerance is derived in :func:`test_header_against_the_definition`'s docstring; everything else is
``np.array_equal`` on the bits."""
from fractions import Fraction

import numpy as np
import pytest

import _hstat_host as host
import _ice_host as ice_host
import _predict_exact as ex
import _rowreduce_host as rr
from _recording_backend import Recorder
from pymc_bart_amd import _abi, friedman_h
from pymc_bart_amd import hstat as hstat_mod
from pymc_bart_amd.trees import PosteriorSampler

ONEHOT, SUBSET = _abi.RULE_ONEHOT, _abi.RULE_SUBSET


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _rows(rng, n, p, nan_rate=0.05):
    X = rng.normal(size=(n, p))
    X[:, 3] = rng.integers(0, 4, n)                                     # the codes of a one-hot column
    X[:, 4] = rng.integers(0, 8, n)                                     # ... and of a subset column
    X[rng.random((n, p)) < nan_rate] = np.nan
    return X


def _named_cases(K):
    """One tree that holds every regressor case for the pair (0, 1): a leaf that regresses on a = 0 below a split on 0
    (a column the path also splits on), one on b = 1, one on the third column 2, and a constant leaf."""
    lf = lambda s, v: ex.Leaf(np.full(K, v) + np.arange(K), count=5 + s, svar=s, slope=np.full(K, 0.75) - np.arange(K), xbar=0.25)  # noqa: E731
    return ex.Split(0, 0.1, lf(0, 1.5), ex.Split(1, -0.2, lf(1, -2.0), ex.Split(5, 0.3, lf(2, 0.5), ex.Leaf(np.full(K, 3.0), count=4),
                                                                                 count=9), count=11), count=30)


def _mixed_pool(rng, K, kind):
    """m = 12 of 14 trees over p = 6 columns: continuous, one-hot (column 3) and subset (column 4) rules; ``kind`` in
    constant / linear / mix decides the leaves.  No tree uses both 3 and 4."""
    rules = {3: ONEHOT, 4: SUBSET}
    linear = {"constant": (), "linear": (0, 1, 2, 5), "mix": (0, 1, 2, 5)}[kind]

    def split_of(r, j):
        return float(r.integers(0, 4)) if j == 3 else float(r.integers(1, 255)) if j == 4 else float(r.normal())

    roots = [] if kind == "constant" else [_named_cases(K)]
    while len(roots) < 14:
        cols = list(rng.choice(6, size=int(rng.integers(1, 4)), replace=False))
        if 3 in cols and 4 in cols:                                     # no tree uses 3 and 4: L_34 is empty
            cols.remove(4)
        root = ex.dyadic_tree(rng, K, 3, cols, split_of, linear=linear if kind != "mix" or len(roots) % 2 else (),
                              counts="free", rules=rules)
        roots.append(root)
    return ex.build_pool(roots, K)


def _gamma(N):
    return Fraction(N) * ex.U / (1 - Fraction(N) * ex.U)


# ------------------------------------------------------------------ 1. the header against the definition
@pytest.mark.parametrize("K,kind", [(1, "constant"), (1, "mix"), (3, "linear")])
def test_header_against_the_definition(oracle, K, kind):
    """Every per-row ``J``, ``T`` and ``I`` of the header against the exact value, within ``4 gamma_N S``.

    The exact value is a combination of four partial dependences (for ``T``: three and the walk's sum), each a sum
    of terms ``in * e * B0`` (``+ in * slope * B1``) whose absolute values add up to at most ``S``, the largest
    ``sum |w| (|value| + |slope| |x - xbar|)`` of any hybrid row (``_predict_exact``'s ``S``, taken over all hybrid rows
    of the job: a weighted mean of sums below ``S`` is below ``S``).  The roundings on the longest chain of one term,
    counted in ``include/pgbart_hstat.h`` and ``pgbart_shap.h``: the factors -- one quotient per split of the path, one
    product per further member of a group and one per group on either side, at most ``3 depth``; ``v * out`` and
    ``out * d`` with ``d = x - xbar``, 3; the lane sum of the moment, at most ``n_b + 64`` additions, and as many for
    ``V``; the division by ``V``, 1; ``pgb_leaf_pred``, 3; ``e * B0``, ``slope * B1`` and their sum, 3; ``in * t``, 1; the
    accumulation of ``pd``, one addition per leaf of the job's trees; the combination, 3.  (The walk's own chain,
    ``2 L + 4 + T``, is shorter.)  So ``N = 3 depth + 2 (n_b + 64) + n_leaves + 14`` and every one of the four
    quantities is within ``gamma_N S`` (Higham, lemma 3.1).  Nothing in it is measured.

    The pools hold constant, linear and mixed leaves, all three split rules, 5 % NaN in both row sets, a tree named
    twice, a regressor on ``a``, on ``b``, on a third column and on a column the path also splits on, and pairs
    without a common tree."""
    rng = np.random.default_rng(100 + K + len(kind))
    p, n_e, n_b = 6, 10, 9
    pool = _mixed_pool(rng, K, kind)
    table = np.stack([rng.permutation(14)[:12] for _ in range(2)]).astype(np.int32)
    if kind != "constant":
        table[:, 0] = 0                                                 # the tree of the named cases is in every forest
    table[1, 7] = table[1, 3]                                           # a tree named twice
    Xe, Xb = _rows(rng, n_e, p), _rows(rng, n_b, p)
    v, w = rng.uniform(0.5, 2.0, n_b), rng.uniform(0.5, 2.0, n_e)
    cols, pairs = [0, 1, 2, 3, 4], [(0, 1), (0, 2), (1, 4), (3, 4), (2, 3)]
    ref, _ = host.whole_call(oracle, pool, table, cols, pairs, [0, 1], Xb, v, Xe, w)
    sizes, common, plan = ref.jobs.sizes(plan=True)
    assert np.array_equal(common, ref.n_common) and common.min() >= 0
    depth = max(ex.tree_depth(pool, t) for t in range(pool.n_trees))
    J, T, I = ref.J, ref.T, ref.I  # noqa: E741
    per, worst = len(cols) + len(pairs), 0.0
    exact_of = lambda x: Fraction(float(x))  # noqa: E731

    def bound_of(e, S):
        n_leaves = int(plan["slot_off"][e + 1] - plan["slot_off"][e])
        return 4 * _gamma(3 * depth + 2 * (n_b + 64) + n_leaves + 14) * S

    for d in range(2):
        for s, a in enumerate(cols):
            e = d * per + s
            trees = plan["tree"][plan["tree_off"][e]:plan["tree_off"][e + 1]]
            assert sorted(trees.tolist()) == sorted(int(t) for t in table[d] if a in host.permimp.tree_uses(pool, int(t), p))
            bf = host.brute_force(pool, trees, a, None, Xe, Xb, v)
            bound = bound_of(e, bf["abs"])
            for k in range(K):
                for i in range(n_e):
                    Jx = bf["a"][k, i] - bf["0"][k, i]
                    Tx = bf["f"][k, i] - bf["a"][k, i] - bf["-a"][k, i] + bf["0"][k, i]
                    for got, want in ((J[d, s, k, i], Jx), (T[d, s, k, i], Tx)):
                        err = abs(exact_of(got) - want)
                        assert err <= bound, (d, a, k, i, float(err), float(bound))
                        worst = max(worst, float(err / bound) if bound else 0.0)
        for j, (sa, sb) in enumerate(pairs):
            e = d * per + len(cols) + j
            trees = plan["tree"][plan["tree_off"][e]:plan["tree_off"][e + 1]]
            assert trees.size == common[d, j]
            bf = host.brute_force(pool, trees, cols[sa], cols[sb], Xe, Xb, v)
            bound = bound_of(e, bf["abs"])
            for k in range(K):
                for i in range(n_e):
                    Ix = bf["ab"][k, i] - bf["a"][k, i] - bf["b"][k, i] + bf["0"][k, i]
                    err = abs(exact_of(I[d, j, k, i]) - Ix)
                    assert err <= bound, (d, j, k, i, float(err), float(bound))
                    worst = max(worst, float(err / bound) if bound else 0.0)
    print(f"max error / bound = {worst:.3g}")
    assert (common == 0).any() and (common > 1).any()                   # an empty L_ab and a long one
    if kind != "constant":                                              # the regressor cases are all met in L_01
        e = len(cols)                                                   # (pick 0, pair (0, 1))
        assert 0 in plan["tree"][plan["tree_off"][e]:plan["tree_off"][e + 1]].tolist()


def test_no_tree_outside_the_lists_is_needed(oracle):
    """``PD_ab - PD_0`` of the FULL forest, by brute force in ``Fraction``, equals ``J_a + J_b + I_ab`` of the lists,
    within the sum of the three bounds of :func:`test_header_against_the_definition` (``2 + 2 + 4`` quantities of
    ``gamma_N S`` each, ``S`` and the leaves now those of the whole forest, which bound those of every list)."""
    rng = np.random.default_rng(7)
    p, n_e, n_b, K = 6, 8, 7, 1
    pool = _mixed_pool(rng, K, "mix")
    table = rng.permutation(14)[None, :12].astype(np.int32)
    Xe, Xb = _rows(rng, n_e, p), _rows(rng, n_b, p)
    v, w = rng.uniform(0.5, 2.0, n_b), rng.uniform(0.5, 2.0, n_e)
    cols, pairs = [0, 1, 5], [(0, 1), (1, 2)]
    ref, _ = host.whole_call(oracle, pool, table, cols, pairs, [0], Xb, v, Xe, w)
    J, I = ref.J, ref.I  # noqa: E741
    depth = max(ex.tree_depth(pool, t) for t in range(pool.n_trees))
    n_leaves = int(sum((np.asarray(pool.var)[pool.node_off[t]:pool.node_off[t + 1]] < 0).sum() for t in table[0]))
    for j, (sa, sb) in enumerate(pairs):
        bf = host.brute_force(pool, table[0], cols[sa], cols[sb], Xe, Xb, v)
        bound = 8 * _gamma(3 * depth + 2 * (n_b + 64) + n_leaves + 14) * bf["abs"]
        for i in range(n_e):
            want = bf["ab"][0, i] - bf["0"][0, i]
            got = Fraction(float(J[0, sa, 0, i])) + Fraction(float(J[0, sb, 0, i])) + Fraction(float(I[0, j, 0, i]))
            assert abs(got - want) <= bound, (j, i, float(abs(got - want)), float(bound))
        assert any(abs(bf["ab"][0, i] - bf["0"][0, i]) > 0 for i in range(n_e))


# ------------------------------------------------------------------ 2. exact facts
@pytest.fixture(scope="module")
def facts(oracle):
    """Column 3 is used by trees that split (and regress) on nothing else; column 5 by one tree of its own; columns 0, 1,
    2 share trees.  K = 2, linear leaves, NaN in both row sets."""
    rng = np.random.default_rng(11)
    K = 2
    own = lambda j, lin: ex.dyadic_tree(rng, K, 3, [j], lambda r, c: float(r.normal()), grow=1.0, linear=lin, counts="free")  # noqa: E731
    roots = [own(3, (3,)), own(3, ()), own(3, (3,)), own(5, ())]
    roots += [ex.dyadic_tree(rng, K, 3, [0, 1, 2], lambda r, c: float(r.normal()), grow=0.9, linear=(0, 2), counts="free")
              for _ in range(6)]
    pool = ex.build_pool(roots, K)
    table = np.stack([rng.permutation(10), rng.permutation(10)]).astype(np.int32)
    Xe, Xb = rng.normal(size=(200, 6)), rng.normal(size=(150, 6))
    Xe[rng.random(Xe.shape) < 0.05] = np.nan
    Xb[rng.random(Xb.shape) < 0.05] = np.nan
    v, w = rng.uniform(0.5, 2.0, 150), rng.uniform(0.5, 2.0, 200)
    cols, pairs = [0, 1, 2, 3, 5], [(0, 1), (3, 4), (0, 3), (1, 2)]
    var_fit = rng.uniform(1.0, 2.0, (2, K))
    ref, out = host.whole_call(oracle, pool, table, cols, pairs, [0, 1], Xb, v, Xe, w, var_fit)
    return dict(pool=pool, table=table, Xe=Xe, Xb=Xb, v=v, w=w, cols=cols, pairs=pairs, var_fit=var_fit, ref=ref, out=out)


def test_a_column_whose_trees_use_nothing_else_has_no_interaction_at_all(facts):
    T, out = facts["ref"].T, facts["out"]
    assert np.all(bits(T[:, 3]) == 0) and np.all(bits(T[:, 4]) == 0)    # +0.0 at every row, NaN rows included
    assert np.all(bits(out["total_var"][:, 3:]) == 0) and np.all(bits(out["h2_total"][:, 3:]) == 0)
    assert np.count_nonzero(T[:, :3]) > 0 and np.all(out["h2_total"][:, :3] > 0.0)
    assert np.all(out["main_var"] > 0.0)


def test_a_pair_without_a_common_tree_has_h2_zero(facts):
    ref, out = facts["ref"], facts["out"]
    assert ref.n_common[:, 1].tolist() == [0, 0] and ref.n_common[:, 2].tolist() == [0, 0] and ref.n_common[:, 0].min() > 0
    assert np.all(bits(ref.I[:, 1:3]) == 0)
    assert np.all(bits(out["inter_var"][:, 1:3]) == 0) and np.all(bits(out["h2"][:, 1:3]) == 0)
    assert np.all(out["h2"][:, [0, 3]] > 0.0) and out["n_nonfinite"] == 0


def test_b0_is_one_where_no_group_lies_outside_the_subset(facts):
    ref = facts["ref"]
    sizes, _, plan = ref.jobs.sizes(plan=True)
    B, V = ref.B()
    lane_sum = 0.0                                                      # V is a lane sum: 64 partials, added in lane order
    for lane in range(64):
        part = 0.0
        for x in facts["v"][lane::64]:
            part = part + float(x)
        lane_sum = lane_sum + part
    assert V == lane_sum
    per = len(facts["cols"]) + len(facts["pairs"])
    for d in range(2):
        for s in (3, 4):                                                # the jobs of columns 3 and 5: every group is on a
            e = d * per + s
            mine = B[plan["slot_off"][e]:plan["slot_off"][e + 1]]
            assert mine.shape[0] > 0 and np.all(mine[:, 1] == 1.0)
            assert np.array_equal(bits(mine[:, 0]), bits(mine[:, 2]))   # subset {} and "everything but a": the same sums
            assert np.array_equal(bits(mine[:, 4]), bits(mine[:, 6]))
    e = 0 * per + len(facts["cols"])                                    # pair (0, 1): leaves whose groups are on 0 and 1 only
    mine = B[plan["slot_off"][e]:plan["slot_off"][e + 1]]
    assert np.any(mine[:, 3] == 1.0) and np.all(mine[:, :4] <= 1.0 + 2.0 ** -40) and np.all(mine[:, :4] >= 0.0)


@pytest.mark.parametrize("block", [64, 128])
def test_blocking_the_rows_changes_no_bit(oracle, facts, block):
    f = facts
    ref, out = host.whole_call(oracle, f["pool"], f["table"], f["cols"], f["pairs"], [0, 1], f["Xb"], f["v"], f["Xe"], f["w"],
                               f["var_fit"], block=block)
    for a, b in ((ref.J, f["ref"].J), (ref.T, f["ref"].T), (ref.I, f["ref"].I)):
        assert np.array_equal(bits(a), bits(b))
    for key in ("main_var", "total_var", "h2_total", "inter_var", "h2"):
        assert np.array_equal(bits(out[key]), bits(f["out"][key])), key
    assert np.array_equal(bits(ref.B()[0]), bits(f["ref"].B()[0]))


@pytest.mark.parametrize("k", [-3, 5])
def test_scaling_all_weights_by_a_power_of_two_changes_no_bit(oracle, facts, k):
    f = facts
    s = 2.0 ** k
    ref, out = host.whole_call(oracle, f["pool"], f["table"], f["cols"], f["pairs"], [0, 1], f["Xb"], f["v"] * s, f["Xe"],
                               f["w"] * s, f["var_fit"])
    assert np.array_equal(bits(ref.I), bits(f["ref"].I)) and np.array_equal(bits(ref.T), bits(f["ref"].T))
    for key in ("main_var", "total_var", "h2_total", "inter_var", "h2"):
        assert np.array_equal(bits(out[key]), bits(f["out"][key])), key


def test_other_pairs_columns_and_picks_change_no_bit(oracle, facts):
    f = facts
    ref, out = host.whole_call(oracle, f["pool"], f["table"], [2, 1], [(1, 0)], [1], f["Xb"], f["v"], f["Xe"], f["w"],
                               f["var_fit"][1:])
    # the pair of columns (1, 2), asked for alone, through other slots, for the second pick only
    assert np.array_equal(bits(ref.I[0, 0]), bits(f["ref"].I[1, 3]))
    assert np.array_equal(bits(out["h2"][0, 0]), bits(f["out"]["h2"][1, 3]))
    assert np.array_equal(bits(out["h2_total"][0]), bits(f["out"]["h2_total"][1, [2, 1]]))
    assert np.array_equal(bits(out["main_var"][0]), bits(f["out"]["main_var"][1, [2, 1]]))


# ------------------------------------------------------------------ 3. a forest with a known answer
def test_a_hand_built_forest_has_its_closed_form_values(oracle):
    """``f = u v + s`` with ``u = 1[x0 <= 0]``, ``v = 1[x1 <= 0]``, ``s = 1 - 2 * 1[x2 <= 0]`` on the balanced design
    ``{-1, +1}^3`` (8 rows, weights one; the rows are their own background).  ``u`` and ``v`` are independent and 0 / 1
    with probability 1/2 each, so ``PD_0 = u / 2``, ``PD_1 = v / 2``, ``PD_01 = u v``, ``PD_{} = 1/4`` over the one tree
    that uses 0 and 1, and

    * ``J_0 = u / 2 - 1/4``: variance ``1/16``, ``main_sd[0] = 1/4``; ``J_2 = s``: ``main_sd[2] = 1``;
    * ``I_01 = (u - 1/2)(v - 1/2) = +-1/4``: ``inter_var = 1/16``; ``U_01 = u v - 1/4``: variance ``3/16``; so
      ``h2[0, 1] = 1/3``;
    * no tree uses 0 and 2: ``h2[0, 2] = 0``;
    * ``T_0 = u v - u / 2 - v / 2 + 1/4 = I_01``: variance ``1/16``; ``var_fit = var(u v) + var(s) = 3/16 + 1``:
      ``h2_total[0] = h2_total[1] = 1/19``; the tree of column 2 splits on nothing else: ``h2_total[2] = 0``.

    Every quantity but the two quotients is dyadic, and a quotient of two exact values is correctly rounded, so the
    comparison is ``==``."""
    K = 1
    t1 = ex.Split(0, 0.0, ex.Split(1, 0.0, ex.Leaf([1.0], 2), ex.Leaf([0.0], 2), count=4), ex.Leaf([0.0], 4), count=8)
    t2 = ex.Split(2, 0.0, ex.Leaf([-1.0], 4), ex.Leaf([1.0], 4), count=8)
    pool = ex.build_pool([t1, t2], K)
    table = np.array([[0, 1]], np.int32)
    X = np.array([[a, b, c] for a in (-1.0, 1.0) for b in (-1.0, 1.0) for c in (-1.0, 1.0)])
    w = np.ones(8)
    be = host.HostBackend(oracle, pool)
    s = PosteriorSampler(pool, table, 2, K, backend=be)
    res = friedman_h(s, X)
    assert res["pairs"].tolist() == [[0, 1], [0, 2], [1, 2]] and res["n_common_trees"].tolist() == [[1, 0, 0]]
    assert res["var_fit"].tolist() == [19.0 / 16.0]
    assert res["h2"][0].tolist() == [1.0 / 3.0, 0.0, 0.0]
    assert res["inter_sd"][0].tolist() == [0.25, 0.0, 0.0]
    assert res["h2_total"][0].tolist() == [1.0 / 19.0, 1.0 / 19.0, 0.0]
    assert res["main_sd"][0].tolist() == [0.25, 0.25, 1.0]
    assert res["total_inter_sd"][0].tolist() == [0.25, 0.25, 0.0]
    assert np.array_equal(res["h"], np.sqrt(res["h2"])) and res["n_nonfinite"] == 0
    # the same through the reference itself
    _, out = host.whole_call(oracle, pool, table, [0, 1, 2], [(0, 1), (0, 2)], [0], X, w, X, w, np.array([[19.0 / 16.0]]))
    assert out["h2"].ravel().tolist() == [1.0 / 3.0, 0.0] and out["inter_var"].ravel().tolist() == [1.0 / 16.0, 0.0]


# ------------------------------------------------------------------ 4. the Python layer
N_SMALL = 130


@pytest.fixture(scope="module")
def small(oracle):
    rng = np.random.default_rng(17)
    pool = ice_host.random_pool(rng, 16, 5, depth=3, split_cols=[0, 1, 3], linear=[3])
    be = host.HostBackend(oracle, pool)
    s = ice_host.pool_sampler(rng, pool, 6, 4, be)
    X = rng.normal(size=(N_SMALL, 5))
    X[rng.random(X.shape) < 0.05] = np.nan
    X[:, 3] = rng.normal(size=N_SMALL)                                  # (column 3 is a regressor: it stays finite)
    return be, s, pool, X, rng.uniform(0.5, 2.0, N_SMALL)


@pytest.fixture(scope="module")
def whole(small):
    import os

    assert "PGB_PW_BLOCK_BYTES" not in os.environ
    be, s, _, X, w = small
    del be.calls[:]
    res = friedman_h(s, X, weights=w)
    return res, list(be.calls)


def test_shapes_and_the_sequence_of_calls_with_one_output(small, whole):
    res, calls = whole
    assert res["cols"].tolist() == [0, 1, 2, 3, 4] and res["pairs"].shape == (10, 2) and res["n_draws"] == 4
    assert np.all(res["pairs"][:, 0] < res["pairs"][:, 1])
    for key in ("h2", "h", "inter_sd"):
        assert res[key].shape == (4, 10) and res[key + "_mean"].shape == (10,) and res[key + "_hdi"].shape == (10, 2), key
    for key in ("h2_total", "total_inter_sd", "main_sd"):
        assert res[key].shape == (4, 5) and res[key + "_sd"].shape == (5,) and res[key + "_hdi"].shape == (5, 2), key
    assert res["n_common_trees"].shape == (4, 10) and res["var_fit"].shape == (4,) and "rows" not in res
    assert [c[0] for c in calls] == ["workspace_bytes", "background", "rows", "finish"]
    assert calls[1][1:] == (N_SMALL, 5, 10) and calls[2][1:] == (N_SMALL, 5, 10)
    # columns 2 and 4 are used by no tree: nothing interacts with them
    unused = [j for j, (a, b) in enumerate(res["pairs"].tolist()) if a in (2, 4) or b in (2, 4)]
    assert np.all(res["h2"][:, unused] == 0.0) and np.all(res["n_common_trees"][:, unused] == 0)
    assert np.all(res["main_sd"][:, [2, 4]] == 0.0) and np.all(res["h2"] >= 0.0)
    pred = host.permimp.predict(small[0].lib._oracle, small[2], np.asarray(small[1].forest_idx), small[3])
    want = rr.reduce(pred, small[4], np.zeros(N_SMALL, np.int32), 1)["out"][1][:, 0, 0]
    assert np.array_equal(bits(res["var_fit"]), bits(want))


def test_blocks_chunks_subsets_and_the_order_of_a_pair_change_no_bit(small, whole, monkeypatch):
    be, s, _, X, w = small
    res, _ = whole
    job = hstat_mod.HstatJob(s, X, None, None, None, w, None, None, 0.94, False, None)
    (one,) = job.chunks(be)
    assert one.n_pairs == 10 and one.ws_bytes > 1 << 16
    # a limit that holds the moments of the whole call and 64 rows: blocks of rows; one below the moments: chunks of pairs
    for limit, kind in ((one.ws_bytes + 64 * job.row_bytes(one) + 8, "rows"), (one.ws_bytes - 8, "finish")):
        monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(limit))
        del be.calls[:]
        again = friedman_h(s, X, weights=w)
        kinds = [c[0] for c in be.calls]
        assert kinds.count(kind) > 1, (kind, kinds)
        if kind == "rows":
            assert all(c[1] <= 64 for c in be.calls if c[0] == "rows") and kinds.count("finish") == 1
        else:
            assert kinds.count("background") == kinds.count("finish")   # every chunk has moments of its own
        for key in hstat_mod.PER_DRAW:
            for suffix in ("", "_mean", "_sd", "_hdi"):
                assert np.array_equal(bits(again[key + suffix]), bits(res[key + suffix])), (kind, key + suffix)
        assert np.array_equal(again["n_common_trees"], res["n_common_trees"])
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES")
    some = friedman_h(s, X, cols=[3, 0, 1], pairs=[(3, 0), (1, 0)], weights=w, draws=[2, 0])
    assert some["pairs"].tolist() == [[0, 3], [0, 1]] and some["cols"].tolist() == [3, 0, 1]
    at = [res["pairs"].tolist().index(pr) for pr in ([0, 3], [0, 1])]
    for key in ("h2", "h", "inter_sd"):
        assert np.array_equal(bits(some[key]), bits(res[key][[2, 0]][:, at])), key
    for key in ("h2_total", "total_inter_sd", "main_sd"):
        assert np.array_equal(bits(some[key]), bits(res[key][[2, 0]][:, [3, 0, 1]])), key


def test_no_pairs_another_background_and_rows(small, whole):
    be, s, _, X, w = small
    res, _ = whole
    cols_only = friedman_h(s, X, pairs=[], weights=w)
    assert cols_only["h2"].shape == (4, 0) and cols_only["pairs"].shape == (0, 2) and cols_only["h2_mean"].shape == (0,)
    for key in ("h2_total", "total_inter_sd", "main_sd"):
        assert np.array_equal(bits(cols_only[key]), bits(res[key])), key
    rng = np.random.default_rng(5)
    Xb, vb = rng.normal(size=(70, 5)), rng.uniform(0.5, 2.0, 70)
    other = friedman_h(s, X, cols=[0, 1, 3], weights=w, background=Xb, background_weights=vb, rows=True)
    assert not np.array_equal(other["h2"], res["h2"][:, [0, 2, 7]]) and np.all(np.isfinite(other["h2"]))
    same = friedman_h(s, X, cols=[0, 1, 3], weights=w, background=X, background_weights=w)   # X as its own background
    at = [res["pairs"].tolist().index(pr) for pr in ([0, 1], [0, 3], [1, 3])]
    assert np.array_equal(bits(same["h2"]), bits(res["h2"][:, at]))
    rows = other["rows"]
    assert rows["total"]["mean"].shape == (N_SMALL, 3) and rows["pair"]["hdi"].shape == (N_SMALL, 3, 2)
    assert np.all(rows["pair"]["hdi"][..., 0] <= rows["pair"]["mean"] + 1e-12) and np.all(rows["total"]["sd"] >= 0.0)
    # the per-row mean is the mean over the draws of the reference's per-row values
    ref, _ = host.whole_call(be.lib._oracle, small[2], np.asarray(s.forest_idx), [0, 1, 3], [(0, 1), (0, 2), (1, 2)],
                             [0, 1, 2, 3], Xb, vb, X, w)
    assert np.allclose(rows["pair"]["mean"], ref.I[:, :, 0].mean(axis=0).T, rtol=1e-12, atol=1e-15)
    assert np.allclose(rows["total"]["mean"], ref.T[:, :, 0].mean(axis=0).T, rtol=1e-12, atol=1e-15)


def test_three_outputs_keep_the_k_axis(oracle):
    rng = np.random.default_rng(23)
    pool = ice_host.random_pool(rng, 12, 4, K=3, depth=3)
    be = host.HostBackend(oracle, pool)
    s = ice_host.pool_sampler(rng, pool, 5, 3, be)
    X = rng.uniform(-1, 1, size=(70, 4))
    res = friedman_h(s, X, cols=[2, 0, 3], rows=True)
    assert res["h2"].shape == (3, 3, 3) and res["h2_hdi"].shape == (3, 3, 2) and res["main_sd"].shape == (3, 3, 3)
    assert res["h2_total_mean"].shape == (3, 3) and res["var_fit"].shape == (3, 3)
    assert res["rows"]["pair"]["mean"].shape == (70, 3, 3) and res["rows"]["total"]["hdi"].shape == (70, 3, 3, 2)


def _stumps(K=1):
    return ex.build_pool([ex.Split(j, 0.5 * j, ex.Leaf(np.full(K, -1.0)), ex.Leaf(np.full(K, 1.0))) for j in range(3)], K)


HSTAT_NAMES = ("pgb_hstat_workspace_bytes", "pgb_hstat_background", "pgb_hstat_rows", "pgb_hstat_finish")


def _recorded(K=1, draws=5):
    rec = Recorder()
    rec.lib.hstat_entry_points = lambda fns=tuple(rec.function(nm) for nm in HSTAT_NAMES): fns
    names = ("pgb_row_reduce", "pgb_row_reduce_finish", "pgb_row_reduce_workspace_bytes")
    rec.lib.rowreduce_entry_points = lambda fns=tuple(rec.function(nm) for nm in names): fns
    s = PosteriorSampler(_stumps(K), np.tile(np.arange(3, dtype=np.int32), (draws, 1)), 3, K, backend=rec)
    return rec, s


def _X(n=8):
    return np.arange(3.0 * n).reshape(n, 3)


def test_argument_errors_are_raised_before_a_backend_is_touched(monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rec, s = _recorded()
    cases = [
        (dict(X=np.zeros((2, 2, 2))), "X must be a matrix"),
        (dict(draws=[9]), "draws must index"), (dict(draws=[]), "at least 1 draw"),
        (dict(hdi_prob=1.0), "hdi_prob must lie in"), (dict(hdi_prob=0.0), "hdi_prob must lie in"),
        (dict(cols=[]), "cols must be a non-empty vector"), (dict(cols=[0, 3]), "cols must index the 3 columns"),
        (dict(cols=[1, 1]), "cols must not name a column twice"),
        (dict(pairs=5), "pairs must be a list of 2-tuples"), (dict(pairs=[(0, 1, 2)]), "pairs must be a list of 2-tuples"),
        (dict(pairs=[(0, 3)]), "pairs must index the 3 columns"), (dict(pairs=[(1, 1)]), "pairs must name two different columns"),
        (dict(pairs=[(0, 1), (1, 0)]), "pairs must not name a pair twice"),
        (dict(cols=[0, 1], pairs=[(0, 2)]), "pairs names column 2, which is not among cols"),
        (dict(background=np.zeros((4, 2))), "background must have the 3 columns of X"),
        (dict(background_weights=np.ones(8)), "background_weights needs a background"),
        (dict(weights=np.ones(7)), "weights must hold one value per row of X"),
        (dict(weights=-np.ones(8)), "weights must be finite and >= 0"), (dict(weights=np.zeros(8)), "weights must have a positive total"),
        (dict(background=_X(4), background_weights=np.ones(5)), "background_weights must hold one value per row of background"),
        (dict(background=_X(4), background_weights=np.zeros(4)), "background_weights must have a positive total"),
        (dict(rows=True, draws=[1]), "at least 2 draws"),
    ]
    for change, msg in cases:
        kw = dict(X=_X())
        kw.update(change)
        with pytest.raises(ValueError, match=msg):
            friedman_h(s, **kw)
    with pytest.raises(TypeError, match="sampler must be"):
        friedman_h(object(), _X())
    assert rec.trace == []


def test_hip_backend_only():
    rec, s = _recorded()
    rec.lib.backend_name = "cpu-oracle"
    with pytest.raises(_abi.PGBError, match="the H-statistic runs on the HIP backend only, not on cpu-oracle"):
        friedman_h(s, _X())
    assert rec.trace == []
    rec2, _ = _recorded()
    friedman_h(s, _X(), backend=rec2)                                   # backend= takes the place of the sampler's own
    assert rec.trace == [] and any(line.startswith("pgb_hstat_rows") for line in rec2.trace)


def test_the_recorded_sequence_of_calls_per_block(monkeypatch):
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")                  # 1024 rows of X (64 bytes each), 2048 of the background
    rec, s = _recorded(draws=2)
    friedman_h(s, _X(2100), pairs=[(0, 2)], background=_X(2054))
    calls = [line.split()[0] for line in rec.trace if line.startswith("pgb_")]
    # the pair's chunk asks for its size first (and the chunk of the column no pair names for its own); var_fit: one
    # predict and one reduce per block of X (52 bytes a row: 1216 rows); then per chunk the background blocks, the row
    # blocks (the pair's chunk: 64 bytes a row; the lone column's: 48, so 1344 rows) and the finish
    assert calls == ["pgb_hstat_workspace_bytes"] * 2 + ["pgb_predict", "pgb_row_reduce"] * 2 + ["pgb_row_reduce_finish"] + \
        ["pgb_hstat_background"] * 2 + ["pgb_hstat_rows"] * 3 + ["pgb_hstat_finish"] + \
        ["pgb_hstat_background"] * 2 + ["pgb_hstat_rows"] * 2 + ["pgb_hstat_finish"]
    rows = [line.split() for line in rec.trace if line.startswith("pgb_hstat_rows")]
    # trees fidx n_forests m X nb p ldx w first_row init cols q pairs n_pairs picks n_picks ws jscr t_rows i_rows stream
    assert [(r[6], r[10], r[11]) for r in rows[:3]] == [("1024", "0", "1"), ("1024", "1024", "0"), ("52", "2048", "0")]
    assert rows[0][13] == "2" and rows[0][15] == "1" and rows[3][13] == "1" and rows[3][15] == "0"
    assert all(r[20] == "-" and r[21] == "-" and r[19].startswith("dev:") and r[5].startswith("dev:") for r in rows)
    bg = [line.split() for line in rec.trace if line.startswith("pgb_hstat_background")]
    assert [(r[6], r[10], r[11]) for r in bg[:2]] == [("2048", "0", "1"), ("6", "2048", "0")]


def test_a_library_without_the_symbols_is_named(oracle):
    with pytest.raises(NotImplementedError, match="pgb_hstat_workspace_bytes"):
        oracle.lib.hstat_entry_points()
    with pytest.raises(NotImplementedError, match="pgb_hstat_kernel_ms"):
        oracle.lib.hstat_kernel_ms()


# ------------------------------------------------------------------ 5. the header's constants and the timing tool
def test_constants_of_the_header_and_of_the_python_layer_agree():
    assert host.lib().hstat_max_pairs() == hstat_mod.MAX_PAIRS
    assert host.lib().hstat_max_u() == _abi.MAX_DEPTH + 1              # PGB_HSTAT_MAX_U = PGB_SHAP_MAX_U


def test_the_timing_tool_answers_help():
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "timing_hstat.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--baseline-root" in r.stdout and "--baseline-pairs" in r.stdout
