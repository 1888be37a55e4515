"""Accumulated local effects, the parts that need no GPU: the bin of ``include/pgbart_ale.h`` against
``np.searchsorted``, hand-built pools whose answer is known exactly (a stump, an additive pool, a product tree), and the
Python layer on a backend made of the host references (``_ale_host.HostBackend``) -- its blocking, chunking and subset
rules, its finish restated, ``ale_edges``, and every refusal."""
from fractions import Fraction

import numpy as np
import pytest

import _ale_host as host
import _ice_host as ice_host
import _predict_exact as ex
import _rowreduce_host as rowred
from _recording_backend import Recorder
from pymc_bart_amd import _abi, accumulated_local_effects, ale_edges
from pymc_bart_amd import ale as ale_mod
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays

LIST_KEYS = ("ale", "mean", "sd", "hdi", "local_effect", "local_var", "bin_weight", "edges")
ARRAY_KEYS = ("cols", "skipped", "n_missing", "importance", "importance_mean", "importance_hdi")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_same(got, want, skip=()):
    """Every key of two results, bit for bit."""
    assert got["n_draws"] == want["n_draws"] and got["n_nonfinite"] == want["n_nonfinite"]
    for key in ARRAY_KEYS:
        if key not in skip:
            assert np.array_equal(bits(got[key]), bits(want[key])), key
    for key in LIST_KEYS:
        if key in skip:
            continue
        assert len(got[key]) == len(want[key]), key
        for s, (a, b) in enumerate(zip(got[key], want[key])):
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (key, s)


# ------------------------------------------------------------------ 1. the bin
def _probe_values(e):
    inner = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), (e[:-1] + e[1:]) / 2])
    outer = [-np.inf, np.inf, e[0] - 1.0, e[0] - 1e300, e[-1] + 1.0, e[-1] + 1e300, -0.0, 0.0]
    return np.concatenate([inner, outer])


@pytest.mark.parametrize("B", [1, 2, 3, 7, 40, 1023, 1024])
def test_the_bin_is_searchsorted_on_the_interior_edges(B):
    rng = np.random.default_rng(B)
    e = np.sort(rng.normal(size=B + 1)) if B < 1000 else np.cumsum(rng.uniform(1e-3, 1.0, B + 1)) - 300.0
    assert np.all(np.diff(e) > 0)
    x = _probe_values(e)
    got = host.bin_of(e, x)
    assert np.array_equal(got, np.searchsorted(e[1:B], x, side="left"))
    assert got.min() == 0 and got.max() == B - 1
    # a value on an edge belongs to the bin that ends there; the ends take everything beyond them
    assert np.array_equal(host.bin_of(e, e), np.clip(np.arange(B + 1) - 1, 0, B - 1))
    assert host.bin_of(e, [-np.inf, np.inf]).tolist() == [0, B - 1]
    assert host.bin_of(e, [np.nan, -np.nan]).tolist() == [B, B]


def test_the_limit_of_the_header_is_the_modules_and_fits_the_row_reduce():
    assert host.lib().ale_max_bins() == ale_mod.MAX_BINS == 1024
    assert ale_mod.MAX_BINS + 1 <= rowred.max_groups()


# ------------------------------------------------------------------ 2. hand-built pools
def _sampler(oracle, pool, table):
    table = np.ascontiguousarray(table, np.int32)
    be = host.HostBackend(oracle, pool)
    return be, PosteriorSampler(pool, table, table.shape[1], pool.n_outputs, backend=be)


def test_a_stump_has_its_step_in_the_bin_that_holds_the_split_and_zero_elsewhere(oracle, monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rng = np.random.default_rng(3)
    X = rng.normal(size=(100, 3))
    e = ale_edges(X[:, 1], 8)
    assert e.size == 9
    left, right = -1.25, 2.5
    for b, v in ((3, (e[3] + e[4]) / 2), (0, e[0]), (7, np.nextafter(e[8], -np.inf)), (5, e[5])):
        pool = ex.build_pool([ex.Split(1, float(v), ex.Leaf([left]), ex.Leaf([right]))], 1)
        assert e[b] <= v < e[b + 1]
        _, s = _sampler(oracle, pool, [[0], [0]])
        res = accumulated_local_effects(s, X, bins=8)
        assert res["cols"].tolist() == [0, 1, 2] and np.array_equal(res["edges"][1], e)
        want = np.zeros((2, 8))
        want[:, b] = right - left
        assert np.array_equal(bits(res["local_effect"][1]), bits(want))
        for c in (0, 2):                                                # nobody uses the other columns: +0.0
            assert np.all(bits(res["local_effect"][c]) == 0) and np.all(bits(res["ale"][c]) == 0)
        assert np.all(res["local_var"][1] == 0.0) and np.all(res["importance"][:, [0, 2]] == 0.0)
        assert np.all(res["importance"][:, 1] > 0.0)


def test_an_additive_pool_gives_the_exact_step_function_and_no_local_variance(oracle, monkeypatch):
    """Trees that split on one column each: the model is additive, so the local difference is the same number at
    every row and the curve is the trees' step function up to its centre.  128 rows of weight 1 and dyadic leaves: no
    operation of the reduce or of the finish rounds."""
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rng = np.random.default_rng(4)
    split_of = lambda r, j: float(ex.dyadic(r, 3, 1.5))  # noqa: E731
    roots = [ex.dyadic_tree(rng, 1, 3, [t % 3], split_of) for t in range(9)]
    pool = ex.build_pool(roots, 1)
    table = np.stack([rng.permutation(9)[:6] for _ in range(3)])
    X = rng.normal(size=(128, 4))
    _, s = _sampler(oracle, pool, table)
    res = accumulated_local_effects(s, X, cols=[0, 1, 2], bins=10)
    moved = 0
    for slot, c in enumerate([0, 1, 2]):
        e = res["edges"][slot]
        at = np.tile(X[:1], (e.size, 1))
        at[:, c] = e
        step = ex.walk(pool, table, at).R[:, 0, :]                      # (D, B + 1) Fractions: f at every edge, row 0
        for d in range(3):
            for j in range(1, e.size):
                got = Fraction(float(res["ale"][slot][d, j])) - Fraction(float(res["ale"][slot][d, j - 1]))
                assert got == step[d, j] - step[d, j - 1], (c, d, j)
                moved += step[d, j] != step[d, j - 1]
        assert np.all(bits(res["local_var"][slot]) == 0)
    assert moved > 10


def test_a_product_tree_on_correlated_columns_equals_the_definition_in_fractions(oracle, monkeypatch):
    """``local_effect`` against the definition through the exact walk: per bin the mean over its rows of
    f(row, c = upper edge) - f(row, c = lower edge).  Dyadic leaves: the sums are exact and the one division of the
    reduce is correctly rounded, as ``float(Fraction)`` is."""
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rng = np.random.default_rng(5)
    split_of = lambda r, j: float(ex.dyadic(r, 3, 0.75))  # noqa: E731
    roots = [ex.complete_tree(rng, 1, 2, [t % 2, 1 - t % 2], split_of) for t in range(4)]
    pool = ex.build_pool(roots, 1)
    table = np.array([[0, 1, 2, 3], [3, 1, 0, 2]])
    z = rng.normal(size=90)
    X = np.stack([z, 0.8 * z + 0.6 * rng.normal(size=90)], axis=1)     # correlated columns
    _, s = _sampler(oracle, pool, table)
    res = accumulated_local_effects(s, X, bins=5)
    for slot, c in enumerate([0, 1]):
        e = res["edges"][slot]
        b = host.bin_of(e, X[:, c])
        X_hi, X_lo = X.copy(), X.copy()
        X_hi[:, c], X_lo[:, c] = e[b + 1], e[b]
        diff = ex.walk(pool, table, X_hi).R[:, 0, :] - ex.walk(pool, table, X_lo).R[:, 0, :]
        for d in range(2):
            for j in range(e.size - 1):
                rows = np.flatnonzero(b == j)
                assert rows.size > 0
                want = float(sum(diff[d, i] for i in rows) / int(rows.size))
                assert bits(res["local_effect"][slot][d, j]) == bits(want), (c, d, j)
        assert np.any(res["local_var"][slot] > 0.0)                     # the local difference depends on the other column


# ------------------------------------------------------------------ 3. the Python layer: values, blocking, subsets
N_SMALL = 600


@pytest.fixture(scope="module")
def small(oracle):
    rng = np.random.default_rng(17)
    pool = ice_host.random_pool(rng, 16, 5, depth=3, split_cols=[0, 1, 3], linear=[3])
    be = host.HostBackend(oracle, pool)
    s = ice_host.pool_sampler(rng, pool, 4, 3, be)
    X = rng.normal(size=(N_SMALL, 5))
    X[rng.random(X.shape) < 0.05] = np.nan
    X[7, 0], X[8, 0], X[9, 1] = np.inf, -np.inf, np.inf                # (column 3 is a regressor: it stays finite)
    X[:, 4] = rng.integers(0, 3, N_SMALL)                               # three codes: two bins
    w = rng.uniform(0.5, 2.0, N_SMALL)
    return be, s, pool, X, w


@pytest.fixture(scope="module")
def whole(small):
    import os

    be, s, pool, X, w = small
    old = os.environ.pop("PGB_PW_BLOCK_BYTES", None)
    try:
        del be.calls[:]
        res = accumulated_local_effects(s, X, bins=6, weights=w)
        assert be.calls == [(N_SMALL, 5)]
    finally:
        if old is not None:
            os.environ["PGB_PW_BLOCK_BYTES"] = old
    return res


def test_the_results_are_the_finish_of_the_row_reduce_of_the_reference(small, whole, oracle):
    be, s, pool, X, w = small
    res = whole
    assert res["cols"].tolist() == [0, 1, 2, 3, 4] and res["skipped"].size == 0 and res["n_draws"] == 3
    assert [e.size for e in res["edges"]] == [7, 7, 7, 7, 3]
    edges = [ale_edges(X[:, c], 6) for c in range(5)]
    out, bins = host.reference_block(oracle, pool, s.forest_idx, X, list(range(5)), edges, np.arange(3))
    assert res["n_missing"].tolist() == [int(np.isnan(X[:, c]).sum()) for c in range(5)]
    assert np.array_equal((bins == np.asarray([e.size - 1 for e in edges])[:, None]).sum(axis=1), res["n_missing"])
    for c in range(5):
        e, B = edges[c], edges[c].size - 1
        assert np.array_equal(res["edges"][c], e)
        r = rowred.reduce(out[c], w, bins[c], B + 1)
        mean, var, W = r["out"][0][:, 0, :], r["out"][1][:, 0, :], r["W"]
        assert np.array_equal(bits(res["bin_weight"][c]), bits(W[:B])) and np.all(W[:B] > 0)
        assert np.array_equal(bits(res["local_effect"][c]), bits(mean[:, :B]))
        assert np.array_equal(bits(res["local_var"][c]), bits(var[:, :B]))
        # the finish, restated: plain loops in the order the module's docstring fixes
        total = 0.0
        for b in range(B):
            total = total + W[b]
        imp = np.empty(3)
        for d in range(3):
            acc = [0.0]
            for j in range(1, B + 1):
                acc.append(acc[j - 1] + mean[d, j - 1])
            num = 0.0
            for b in range(B):
                num = num + W[b] * ((acc[b] + acc[b + 1]) / 2.0)
            centre = num / total
            ale = np.array([a - centre for a in acc])
            assert np.array_equal(bits(res["ale"][c][d]), bits(ale)), (c, d)
            sq = 0.0
            for b in range(B):
                mid = (ale[b] + ale[b + 1]) / 2.0
                sq = sq + W[b] * (mid * mid)
            imp[d] = np.sqrt(sq / total)
        assert np.array_equal(bits(res["importance"][:, c]), bits(imp))
        assert np.array_equal(bits(res["mean"][c]), bits(res["ale"][c].mean(axis=0)))
        assert np.array_equal(bits(res["sd"][c]), bits(res["ale"][c].std(axis=0))) and res["hdi"][c].shape == (B + 1, 2)
        assert np.all(res["hdi"][c][:, 0] <= res["mean"][c]) and np.all(res["mean"][c] <= res["hdi"][c][:, 1])
    assert np.array_equal(bits(res["importance_mean"]), bits(res["importance"].mean(axis=0)))
    assert res["importance_hdi"].shape == (5, 2)
    # no tree uses columns 2 and 4; 0, 1 and 3 are used
    for c in (2, 4):
        assert np.all(bits(res["local_effect"][c]) == 0) and np.all(res["importance"][:, c] == 0.0)
    assert all(np.any(res["local_effect"][c] != 0.0) for c in (0, 1, 3)) and res["n_nonfinite"] == 0


def test_blocks_of_rows_change_no_bit(small, whole, monkeypatch):
    be, s, pool, X, w = small
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")                  # its floor
    del be.calls[:]
    got = accumulated_local_effects(s, X, bins=6, weights=w)
    # chunks of two columns in blocks of 128 rows; the last column, alone and with two bins, fits one block
    assert be.calls == ([(128, 2)] * 4 + [(88, 2)]) * 2 + [(N_SMALL, 1)]
    assert_same(got, whole)


def test_chunks_of_one_column_change_no_bit(small, whole, monkeypatch):
    be, s, pool, X, w = small
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    monkeypatch.setattr(ale_mod.AleJob, "columns_per_chunk", lambda self: 1)
    del be.calls[:]
    got = accumulated_local_effects(s, X, bins=6, weights=w)
    assert be.calls == [(N_SMALL, 1)] * 5
    assert_same(got, whole)


def test_a_column_alone_weights_scaled_and_a_subset_of_the_draws(small, whole, monkeypatch):
    be, s, pool, X, w = small
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    for j in (3, 0):
        one = accumulated_local_effects(s, X, cols=[j], bins=6, weights=w)
        assert one["cols"].tolist() == [j]
        for key in LIST_KEYS:
            assert np.array_equal(bits(one[key][0]), bits(whole[key][j])), (key, j)
        for key in ("importance", "importance_mean"):
            assert np.array_equal(bits(one[key][..., 0]), bits(whole[key][..., j])), key
        assert np.array_equal(bits(one["importance_hdi"][0]), bits(whole["importance_hdi"][j]))
    scaled = accumulated_local_effects(s, X, bins=6, weights=w * 2.0 ** -3)
    assert_same(scaled, whole, skip=("bin_weight",))
    for a, b in zip(scaled["bin_weight"], whole["bin_weight"]):
        assert np.array_equal(bits(a), bits(b * 2.0 ** -3))
    some = accumulated_local_effects(s, X, bins=6, weights=w, draws=[2, 0])
    assert some["n_draws"] == 2
    for key in ("ale", "local_effect", "local_var"):
        for c in range(5):
            assert np.array_equal(bits(some[key][c]), bits(whole[key][c][[2, 0]])), (key, c)
    assert np.array_equal(bits(some["importance"]), bits(whole["importance"][[2, 0]]))


def test_user_edges_an_empty_bin_and_three_outputs(oracle, monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rng = np.random.default_rng(23)
    pool = ice_host.random_pool(rng, 12, 3, K=3, depth=3)
    be = host.HostBackend(oracle, pool)
    s = ice_host.pool_sampler(rng, pool, 5, 4, be)
    X = rng.uniform(-1, 1, size=(130, 3))
    mine = np.array([-2.0, -0.5, 0.0, 0.5, 5.0, 9.0])                  # nobody lies in (5, 9]: bin 4 would be empty ...
    res = accumulated_local_effects(s, X, cols=[2, 0], edges={0: mine}, bins=4)
    assert np.array_equal(res["edges"][1], mine) and np.array_equal(res["edges"][0], ale_edges(X[:, 2], 4))
    assert res["ale"][1].shape == (4, 3, 6) and res["local_effect"][1].shape == (4, 3, 5) and res["mean"][1].shape == (3, 6)
    assert res["hdi"][1].shape == (3, 6, 2) and res["importance"].shape == (4, 3, 2) and res["importance_hdi"].shape == (3, 2, 2)
    # ... but the last bin takes everything above the last edge too, so it is bin 3 = (0.5, 5] that the rows end in
    assert res["bin_weight"][1][4] == 0.0 and np.all(res["bin_weight"][1][:4] > 0.0)
    assert np.all(bits(res["local_effect"][1][..., 4]) == 0) and np.all(np.isnan(res["local_var"][1][..., 4]))
    assert np.array_equal(bits(res["ale"][1][..., 5]), bits(res["ale"][1][..., 4])) and np.all(np.isfinite(res["ale"][1]))


# ------------------------------------------------------------------ 4. ale_edges
def test_edges_on_ties_few_values_and_non_finite_values():
    rng = np.random.default_rng(9)
    x = rng.normal(size=500)
    e = ale_edges(x, 40)
    assert e.size == 41 and e[0] == x.min() and e[-1] == x.max() and np.all(np.diff(e) > 0) and np.all(np.isin(e, x))
    assert np.array_equal(e, np.unique(np.quantile(x, np.linspace(0, 1, 41), method="inverted_cdf")))
    # ties: quantiles that coincide are one edge
    t = np.concatenate([np.zeros(400), rng.normal(size=100)])
    e = ale_edges(t, 10)
    assert 2 <= e.size < 11 and np.all(np.diff(e) > 0) and 0.0 in e
    # fewer distinct values than bins: the values themselves, one bin per step between neighbouring codes
    codes = rng.integers(0, 4, 300).astype(float)
    assert ale_edges(codes, 40).tolist() == [0.0, 1.0, 2.0, 3.0] and ale_edges(codes, 3).tolist() == [0.0, 1.0, 2.0, 3.0]
    assert ale_edges(codes, 2).size <= 3
    # infinities and NaN are left out
    y = np.array([np.nan, -np.inf, 3.0, 1.0, np.inf, 2.0, np.nan, 1.0])
    assert ale_edges(y, 5).tolist() == [1.0, 2.0, 3.0]
    assert ale_edges([np.nan, np.inf], 5).size == 0 and ale_edges([4.0, 4.0, np.nan], 5).tolist() == [4.0]
    for bad in (0, 1025, 2.5, True, None):
        with pytest.raises(ValueError, match="bins must be an integer"):
            ale_edges(x, bad)


# ------------------------------------------------------------------ 5. refusals
def _stumps(K, n_trees=3):
    pool = TreeArrays.empty(n_trees, n_trees, K)
    pool.tree_id[:] = np.arange(n_trees)
    pool.node_off[:] = np.arange(n_trees + 1)
    pool.var[:] = -1
    pool.count[:] = 10
    return pool


def _recorded(K=1, draws=5):
    rec = Recorder()
    rec.lib.predict_ale_entry_point = lambda fn=rec.function("pgb_predict_ale"): fn
    names = ("pgb_row_reduce", "pgb_row_reduce_finish", "pgb_row_reduce_workspace_bytes")
    rec.lib.rowreduce_entry_points = lambda fns=tuple(rec.function(nm) for nm in names): fns
    s = PosteriorSampler(_stumps(K), np.tile(np.arange(3, dtype=np.int32), (draws, 1)), 3, K, backend=rec)
    return rec, s


def _X():
    X = np.arange(24, dtype=np.float64).reshape(8, 3)
    X[:, 2] = 5.0                                                       # a constant column
    return X


def test_argument_errors_are_raised_before_a_backend_is_touched(monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rec, s = _recorded()
    cases = [
        (dict(X=np.zeros((2, 2, 2))), "X must be a matrix"),
        (dict(draws=[9]), "draws must index"),
        (dict(draws=[]), "at least 1 draw"),
        (dict(bins=0), "bins must be an integer"), (dict(bins=1025), "bins must be an integer"),
        (dict(bins=3.0), "bins must be an integer"), (dict(bins=None), "bins must be an integer"),
        (dict(hdi_prob=1.0), "hdi_prob must lie in"),
        (dict(cols=[3]), "cols must index"), (dict(cols=[-1]), "cols must index"),
        (dict(cols=[1, 1]), "cols must not name a column twice"), (dict(cols=[]), "non-empty vector"),
        (dict(cols=[0, 2]), "column 2 has fewer than 2 distinct finite values"),
        (dict(edges=[0.0, 1.0]), "edges must be a dict"),
        (dict(edges={5: [0.0, 1.0]}), "edges names column 5"),
        (dict(cols=[0], edges={1: [0.0, 1.0]}), "edges names column 1"),
        (dict(edges={"a": [0.0, 1.0]}), "edges names column 'a'"),
        (dict(edges={0: [1.0]}), "at least 2 values"), (dict(edges={0: [[0.0, 1.0]]}), "at least 2 values"),
        (dict(edges={0: np.arange(1026.0)}), "at most 1025 edges"),
        (dict(edges={0: [0.0, np.inf]}), "must be finite"), (dict(edges={0: [0.0, np.nan, 1.0]}), "must be finite"),
        (dict(edges={0: [0.0, 0.0, 1.0]}), "strictly increasing"), (dict(edges={0: [1.0, 0.0]}), "strictly increasing"),
        (dict(edges={0: ["x", "y"]}), "vector of numbers"),
        (dict(weights=np.ones(3)), "weights must hold one value per row"),
        (dict(weights=-np.ones(8)), "weights must be finite and >= 0"),
        (dict(weights=np.zeros(8)), "positive total"),
    ]
    for kw, msg in cases:
        args = dict(X=_X())
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            accumulated_local_effects(s, **args)
    with pytest.raises(ValueError, match="no column of X has 2 distinct finite values"):
        accumulated_local_effects(s, np.ones((8, 2)))
    with pytest.raises(TypeError):
        accumulated_local_effects(object(), _X())
    assert rec.trace == []


def test_a_constant_column_is_skipped_unless_it_is_named_or_given_edges(monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rec, s = _recorded()
    with np.errstate(all="ignore"):
        res = accumulated_local_effects(s, _X(), bins=4)
    assert res["cols"].tolist() == [0, 1] and res["skipped"].tolist() == [2] and len(res["ale"]) == 2
    with pytest.raises(ValueError, match="column 2 has fewer than 2 distinct finite values"):
        accumulated_local_effects(s, _X(), cols=[2])
    with np.errstate(all="ignore"):
        res = accumulated_local_effects(s, _X(), cols=[2], edges={2: [4.0, 6.0]})   # edges of one's own: nothing to derive
    assert res["cols"].tolist() == [2] and res["skipped"].size == 0 and res["edges"][0].tolist() == [4.0, 6.0]


def test_the_calls_and_their_arguments_on_the_recording_backend(monkeypatch):
    """One block of 70 rows, two columns of 3 and 5 edges, five draws: one pgb_predict_ale, then per column one reduce
    and one finish -- no pgb_predict, nothing of X but its rows."""
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rec, s = _recorded()
    X = np.zeros((70, 4))
    X[:, 3], X[:, 1] = np.arange(70) % 3, np.arange(70)
    with np.errstate(all="ignore"):
        res = accumulated_local_effects(s, X, cols=[3, 1], bins=4)
    calls = [line for line in rec.trace if line.startswith("pgb_")]
    assert [c.split()[0] for c in calls] == ["pgb_predict_ale", "pgb_row_reduce", "pgb_row_reduce", "pgb_row_reduce_finish",
                                             "pgb_row_reduce_finish"]
    # trees fidx D m X nb p ldx cols q edges edge_off picks n_picks out bins_out stream
    assert calls[0].split()[1:] == ["trees:3", "host", "5", "3", "dev:280+0", "70", "4", "4", "host", "2", "host", "host",
                                    "host", "5", "dev:700+0", "dev:140+0", "-"]
    # a b D K nb ld w g y off_a off_b centre G transform first_row init: the slabs of the scratch, the rows of the bins
    assert calls[1].split()[1:9] == ["dev:700+0", "-", "5", "1", "70", "70", "dev:70+0", "dev:140+0"]
    assert calls[1].split()[9:17] == ["-", "-", "-", "-", "3", "0", "0", "1"]
    assert calls[2].split()[1:9] == ["dev:700+350", "-", "5", "1", "70", "70", "dev:70+0", "dev:140+70"]
    assert calls[2].split()[13] == "5"
    assert not any(line.startswith("to_host") and int(line.split()[1]) >= 5 * 70 for line in rec.trace)
    assert [a.shape for a in res["ale"]] == [(5, 3), (5, 5)] and res["importance"].shape == (5, 2)


def test_a_column_that_does_not_fit_a_block_is_refused_naming_what_to_cut(monkeypatch):
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")
    rec, s = _recorded(draws=5)
    X = np.arange(4000.0).reshape(2000, 2)
    with pytest.raises(ValueError, match=r"one column of 5 draws x 40 bins does not fit a block"):
        accumulated_local_effects(s, X)
    assert rec.trace == []


def test_hip_backend_only():
    rec, s = _recorded()
    rec.lib.backend_name = "cpu-oracle"
    with pytest.raises(_abi.PGBError, match="accumulated local effects run on the HIP backend only, not on cpu-oracle"):
        accumulated_local_effects(s, _X())
    assert rec.trace == []


def test_a_library_without_the_symbol_is_named(oracle):
    with pytest.raises(NotImplementedError, match="pgb_predict_ale"):
        oracle.lib.predict_ale_entry_point()


# ------------------------------------------------------------------ 6. the timing tool
def test_the_timing_tool_answers_help():
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "timing_ale.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--baseline-root" in r.stdout and "--baseline-cols" in r.stdout
