"""Partial dependence sweeps on the MI355X: ``pgb_predict_pdp`` (``k_pdp_walk``, ``k_pdp_lookup``) under ``route=1``
(direct), ``route=2`` (profile where eligible) and ``route=0`` (auto) against the same device's ``sample_posterior``
with every other column excluded.  The walk is ``pred_walk_forest`` and a slot's rows run its representative's
instructions on its operands, so the comparison is ``np.array_equal``, not a tolerance.

Once per pool the device is also held to the CPU oracle.  Both sum the same terms ``w (value + slope (x - xbar))``; each
is within ``gamma_N S`` of the exact sum (``_predict_exact``: ``N = 2 L + 4 + T`` roundings on a term, ``S`` the sum of
the terms' magnitudes), so they differ by at most ``2 gamma_N S``.  ``_oracle_bound`` takes ``L <= PGB_MAX_DEPTH``, ``T
<=`` the nodes of the forest's largest tree times ``m`` and ``S <= m max |leaf term|`` (the weights of one tree's leaves
add up to at most 1): nothing in it is measured."""
import ctypes as C
import math

import numpy as np
import pytest

import _ice_host as ice_host
import _pdp_host as host
import _predict_exact as ex
from pymc_bart_amd import BARTOp, _abi, partial_dependence
from pymc_bart_amd.chains import sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler, _MultiChainSampler

pytestmark = pytest.mark.gpu

MAXB = _abi.PDP_LDS_MAXB
DIRECT, PROFILE = 1, 2


def _oracle_bound(pool, m: int, xmax: float) -> float:
    leaf = pool.var < 0
    term = np.abs(pool.value).max(axis=1) + np.abs(pool.slope).max(axis=1) * (xmax + np.abs(pool.xbar))
    S = m * float(term[leaf].max())
    N = 2 * _abi.MAX_DEPTH + 4 + m * int(np.diff(pool.node_off).max())
    u = 2.0 ** -53
    return 2.0 * (N * u / (1.0 - N * u)) * S


def _eligible(s, cols, picks):
    """Per column: whether every picked forest leaves it eligible, and its slots summed over the picks."""
    pool, table = s.pooled_history() if hasattr(s, "pooled_history") else (s.pool, s.forest_idx)
    out = []
    for c, j in enumerate(cols):
        got = [host.breakpoints(pool, np.asarray(table)[d], j) for d in np.asarray(picks)[c].tolist()]
        out.append((all(ok for ok, _ in got), sum(b.size + 2 for ok, b in got if ok)))
    return out


def _check(s, X, cols, picks, oracle=None):
    """The three routes against the yardstick; the routes each column took are what the contract says.  Returns the
    sweep and the routes taken under ``route=2``."""
    X = np.ascontiguousarray(X, np.float64)
    picks = np.asarray(picks)
    want = host.yardstick(s, X, cols, picks)
    assert want.shape == (len(cols), picks.shape[1], s.n_outputs, X.shape[0]) and not np.isnan(want).any()
    elig = _eligible(s, cols, picks)
    routes = {}
    for route in (1, 2, 0):
        taken = []
        got = s.pdp_sweep(X, cols, picks, route=route, taken=taken)
        assert np.array_equal(got, want), f"route {route}"
        assert len(taken) == 1 and taken[0][:4] == (0, len(cols), 0, X.shape[0])
        routes[route] = taken[0][4]
    assert routes[1] == [DIRECT] * len(cols)
    assert routes[2] == [PROFILE if ok else DIRECT for ok, _ in elig]
    assert routes[0] == [PROFILE if ok and slots < X.shape[0] * picks.shape[1] else DIRECT for ok, slots in elig]
    if oracle is not None:
        pool, table = s.pooled_history() if hasattr(s, "pooled_history") else (s.pool, s.forest_idx)
        m = int(np.asarray(table).shape[1])
        ref = PosteriorSampler(pool, np.asarray(table), m, s.n_outputs, backend=oracle).pdp_sweep(X, cols, picks)
        reg = X[:, sorted(set(pool.svar[pool.svar >= 0].tolist()))]   # the columns some leaf regresses on
        bound = _oracle_bound(pool, m, float(np.abs(reg[np.isfinite(reg)]).max()) if np.isfinite(reg).any() else 0.0)
        diff = float(np.max(np.abs(want - ref)))
        print(f"max |device - oracle| = {diff:.3e} (bound {bound:.3e})")
        assert diff <= bound
    return want, routes[2]


def _data(rng, n, p, rules=None):
    X = rng.normal(size=(n, p))
    for j, r in enumerate([] if rules is None else rules):
        if r == _abi.RULE_ONEHOT:
            X[:, j] = rng.integers(0, 4, n)
        elif r == _abi.RULE_SUBSET:
            X[:, j] = rng.integers(0, 8, n)
    return X


# ------------------------------------------------------------------ 1. row counts, pick counts
@pytest.fixture(scope="module")
def plain(hip):
    """Continuous splits on every column; leaves regress on column 3 (so column 3 is not eligible, the others are)."""
    rng = np.random.default_rng(101)
    pool = ice_host.random_pool(rng, 24, 4, linear=[3])
    return ice_host.pool_sampler(rng, pool, 7, 6, hip), rng.normal(size=(257, 4))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_row_counts(plain, oracle, n):
    s, X = plain
    picks = np.array([[0, 5, 0], [2, 2, 2], [4, 1, 3]])           # repeated picks
    _, taken = _check(s, X[:n], [0, 1, 3], picks, oracle if n == 257 else None)
    assert taken == [PROFILE, PROFILE, DIRECT]                       # svar == 3: direct even under route=2


def test_one_pick(plain):
    s, X = plain
    _check(s, X[:65], [2, 0], np.array([[3], [5]]))


# ------------------------------------------------------------------ 2. layout
def _raw(hip, s, Xwide, p, cols, picks, route, guard=None):
    """``pgb_predict_pdp`` itself on a matrix whose rows are ``ldx = Xwide.shape[1] >= p`` apart.  ``guard``: 64 cells of
    it lie behind the output and come back third."""
    mem, lib = hip.mem, hip.lib
    n, ldx = Xwide.shape
    cols, picks = np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(picks, np.int32)
    K = s.n_outputs
    xd = mem.from_host(np.ascontiguousarray(Xwide))
    size = cols.size * picks.shape[1] * K * n
    od = mem.empty((size,), np.float64) if guard is None else mem.from_host(np.full(size + 64, guard))
    rt = np.zeros(cols.size, np.int32)
    carr = s.pool.as_c()
    rc = lib.pdp_entry_point()(C.byref(carr), s.forest_idx.ctypes.data, s.n_draws, s.m, mem.ptr(xd), n, p, ldx,
                               cols.ctypes.data, cols.size, picks.ctypes.data, picks.shape[1], route, mem.ptr(od),
                               rt.ctypes.data, mem.stream_ptr)
    lib.check(rc, "pgb_predict_pdp")
    got = mem.to_host(od)
    if guard is not None:
        return got[:size].reshape(cols.size, picks.shape[1], K, n), rt.tolist(), got[size:]
    return got.reshape(cols.size, picks.shape[1], K, n), rt.tolist()


def test_rows_further_apart_than_p(plain, hip):
    s, X = plain
    rng = np.random.default_rng(5)
    wide = np.concatenate([X[:130], rng.normal(size=(130, 3))], axis=1)     # ldx = 7 > p = 4
    picks = np.array([[1, 4], [0, 0], [5, 2]])
    want = host.yardstick(s, X[:130], [1, 3, 0], picks)
    assert all(slots < 130 * 2 for _, slots in _eligible(s, [1, 0], picks[[0, 2]]))
    for route, routes in ((1, [DIRECT] * 3), (2, [PROFILE, DIRECT, PROFILE]), (0, [PROFILE, DIRECT, PROFILE])):
        got, taken = _raw(hip, s, wide, 4, [1, 3, 0], picks, route)
        assert np.array_equal(got, want) and taken == routes, route


def test_a_single_column(hip, oracle):
    rng = np.random.default_rng(8)
    pool = ice_host.random_pool(rng, 12, 1)
    s = ice_host.pool_sampler(rng, pool, 5, 4, hip)
    X = rng.normal(size=(70, 1))
    X[3, 0] = np.nan
    want, taken = _check(s, X, [0], np.array([[0, 3, 1]]), oracle)
    assert taken == [PROFILE]
    assert np.array_equal(want[0], s.sample_posterior(X, [0, 3, 1], None))   # nothing is excluded when p = 1


# ------------------------------------------------------------------ 3. breakpoint counts
def test_no_split_one_split_and_shared_split_values(hip, oracle):
    pool = host.hand_pool()                                         # K = 2
    table = np.array([[0, 1, 2, 3], [3, 4, 5, 5], [6, 0, 2, 1], [4, 5, 5, 4]], np.int32)
    s = PosteriorSampler(pool, table, 4, 2, backend=hip)
    assert [host.breakpoints(pool, table[d], 0)[1].size for d in (0, 1, 3)] == [4, 1, 0]   # shared values; B = 1; B = 0
    b = host.breakpoints(pool, table[2], 0)[1]
    # equal to a breakpoint, the doubles on either side, below and above all, +-inf, NaN, -0.0 against 0.0, +inf a breakpoint
    xs = [x for slot in host.probes(b) for x in slot] + [5e-324, -5e-324, 0.0, -0.0, math.inf, -math.inf, math.nan]
    X = np.full((len(xs), 3), 0.375)
    X[:, 0] = xs
    assert math.inf in b and 0.0 in b
    picks = np.array([[0, 1, 2, 3, 2], [3, 3, 3, 3, 3], [2, 0, 1, 2, 0]])
    got, taken = _check(s, X, [0, 0, 0], picks, oracle)
    assert taken == [PROFILE] * 3
    assert np.all(got[1] == got[1][..., :1])                        # B = 0 in every pick: one value per (pick, output)
    _, taken = _check(s, X, [1, 2], picks[:2])
    assert taken == [DIRECT, DIRECT]                                # leaves regress on columns 1 and 2


@pytest.mark.parametrize("B", [MAXB, MAXB + 1])
def test_profiles_at_and_beyond_the_lds_cap(hip, B):
    """Eleven chain trees of 24 splits each on column 0 -- 264 splits with ``B`` distinct values -- in one forest, next
    to a forest of a few breakpoints in the same call (staged while the long one is read from global memory)."""
    rng = np.random.default_rng(B)
    values = list(np.linspace(-3.0, 3.0, B)) + [0.0 - 3.0] * (264 - B)
    rng.shuffle(values)
    it = iter(values)
    roots = [ex.chain_tree(rng, 1, 24, [0], lambda r, j: next(it), "left" if t % 2 else "right", counts="free")
             for t in range(11)]
    roots += [ex.dyadic_tree(rng, 1, 3, [0, 1], lambda r, j: float(r.normal()), counts="free") for _ in range(11)]
    pool = ex.build_pool(roots, 1)
    table = np.array([np.arange(11), np.arange(11, 22)], np.int32)
    s = PosteriorSampler(pool, table, 11, 1, backend=hip)
    assert host.breakpoints(pool, table[0], 0)[1].size == B
    X = rng.uniform(-3.5, 3.5, size=(300, 2))
    X[:40, 0] = rng.choice(np.linspace(-3.0, 3.0, B), 40)           # on a breakpoint
    X[40:60, 0] = np.nextafter(X[:20, 0], np.inf)
    X[60, 0], X[61, 0], X[62, 0] = np.nan, np.inf, -np.inf
    _, taken = _check(s, X, [0, 1], np.array([[0, 1, 0], [1, 0, 1]]))
    assert taken == [PROFILE, PROFILE]


# ------------------------------------------------------------------ 4. leaves, split rules, zero counts
def test_three_outputs_and_linear_leaves(hip, oracle):
    rng = np.random.default_rng(12)
    pool = ice_host.random_pool(rng, 16, 4, K=3, linear=[1, 2])
    s = ice_host.pool_sampler(rng, pool, 6, 5, hip)
    X = _data(rng, 130, 4)
    X[rng.random(130) < 0.1, 1] = np.nan                            # a missing regressor: the leaf's mean
    X[5, 0] = np.nan
    _, taken = _check(s, X, [0, 1, 2, 3], rng.integers(0, 5, size=(4, 3)), oracle)
    assert taken == [PROFILE, DIRECT, DIRECT, PROFILE]              # svar == j: direct; svar != j: profile, the mean


def test_one_hot_and_subset_columns_next_to_continuous_ones(hip, oracle):
    rng = np.random.default_rng(14)
    rules = [0, _abi.RULE_ONEHOT, _abi.RULE_SUBSET, 0, 0]
    pool = ice_host.random_pool(rng, 30, 5, rules=rules)
    s = ice_host.pool_sampler(rng, pool, 9, 5, hip)
    X = _data(rng, 200, 5, rules)
    X[rng.random(200) < 0.1, 1] = np.nan
    X[rng.random(200) < 0.1, 3] = np.nan
    picks = rng.integers(0, 5, size=(5, 3))
    elig = [ok for ok, _ in _eligible(s, range(5), picks)]
    assert elig[0] and elig[3] and elig[4] and not elig[1] and not elig[2]   # (every picked forest splits on 1 and on 2)
    _check(s, X, [0, 1, 2, 3, 4], picks, oracle)


def test_children_with_zero_counts(hip, oracle):
    rng = np.random.default_rng(16)
    pool = ice_host.random_pool(rng, 20, 3)
    splits = np.flatnonzero(pool.var >= 0)
    base = pool.node_off[np.searchsorted(pool.node_off, splits, side="right") - 1]
    for g, b in list(zip(splits.tolist(), base.tolist()))[::3]:     # both children of every third split: nothing is added
        pool.count[b + pool.left[g]] = pool.count[b + pool.right[g]] = 0
    for g, b in list(zip(splits.tolist(), base.tolist()))[1::3]:    # one child of every third: all the weight to the other
        pool.count[b + pool.left[g]] = 0
    s = ice_host.pool_sampler(rng, pool, 8, 5, hip)
    X = _data(rng, 100, 3)
    X[::9, 2] = np.nan
    _, taken = _check(s, X, [0, 1, 2], rng.integers(0, 5, size=(3, 4)), oracle)
    assert taken == [PROFILE] * 3


# ------------------------------------------------------------------ 5. two chains, one pool
def test_two_chains_pooled(hip):
    rng = np.random.default_rng(21)
    a = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 14, 4), 7, 5, hip)
    b = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 18, 4, depth=6), 7, 3, hip)
    s = _MultiChainSampler([a, b])
    X = _data(rng, 100, 4)
    picks = np.empty((2, 6), np.int64)
    picks[:, 0::2] = rng.integers(0, 5, size=(2, 3))                # chain a ...
    picks[:, 1::2] = rng.integers(5, 8, size=(2, 3))                # ... and chain b, alternating
    got, taken = _check(s, X, [3, 0], picks)
    assert taken == [PROFILE, PROFILE]
    assert np.array_equal(got[:, 1::2], b.pdp_sweep(X, [3, 0], picks[:, 1::2] - 5, route=2))


# ------------------------------------------------------------------ 6. blocking
def test_results_do_not_depend_on_the_blocking(plain, monkeypatch):
    s, X = plain
    rng = np.random.default_rng(33)
    X = X[:300 - 43].copy()
    X[::17, 1] = np.nan
    picks = rng.integers(0, 6, size=(3, 4))                         # 8 * 4 * 1 * 257 = 8224 bytes per column
    monkeypatch.delenv("PGB_PDP_BLOCK_BYTES", raising=False)
    whole = s.pdp_sweep(X, [0, 1, 3], picks)
    assert np.array_equal(whole, host.yardstick(s, X, [0, 1, 3], picks))
    for route in (0, 1, 2):
        monkeypatch.setenv("PGB_PDP_BLOCK_BYTES", "16384")          # blocks of one column
        taken = []
        assert np.array_equal(s.pdp_sweep(X, [0, 1, 3], picks, route=route, taken=taken), whole)
        assert [t[:4] for t in taken] == [(0, 1, 0, 257), (1, 2, 0, 257), (2, 3, 0, 257)]
        monkeypatch.setenv("PGB_PDP_BLOCK_BYTES", "4096")           # blocks of 128 rows of one column
        taken = []
        assert np.array_equal(s.pdp_sweep(X, [0, 1, 3], picks, route=route, taken=taken), whole)
        assert [t[:4] for t in taken] == [(c, c + 1, r, min(257, r + 128)) for c in range(3) for r in (0, 128, 256)]


# ------------------------------------------------------------------ 7. the public function
@pytest.fixture(scope="module")
def fits(hip, oracle):
    rng = np.random.default_rng(31)
    X = rng.uniform(-1, 1, size=(130, 4))
    Y = 2.0 * X[:, 0] - X[:, 1] ** 2 + rng.normal(0, 0.1, 130)
    ops = {}
    for name, be in (("hip", hip), ("oracle", oracle)):
        ops[name] = BARTOp(X, Y, m=15)
        sample_chain(ops[name], tune=20, draws=10, num_particles=10, random_seed=6, sigma=0.2, backend=be)
    return X, ops


def test_the_public_call_is_one_sweep_and_the_oracle_backends_numbers(fits, hip, oracle, monkeypatch):
    X, ops = fits
    kw = dict(xs_interval="insample", samples=8, random_seed=2)
    ref = partial_dependence(ops["oracle"], X, backend=oracle, **kw)
    s = _get_posterior_sampler(ops["hip"], backend=hip)
    rng = np.random.default_rng(2)
    picks = np.stack([rng.integers(0, s.n_draws, size=8) for _ in range(4)])
    want = host.yardstick(s, X, [0, 1, 2, 3], picks)

    def refuse(self, *a, **k):
        raise AssertionError("sample_posterior was called")

    calls = []
    real = hip.lib.pdp_entry_point
    monkeypatch.setattr(hip.lib, "pdp_entry_point", lambda: (lambda *a, f=real(): (calls.append(a[9]), f(*a))[1]))
    monkeypatch.setattr(PosteriorSampler, "sample_posterior", refuse)
    monkeypatch.setattr(_MultiChainSampler, "sample_posterior", refuse)
    got = partial_dependence(ops["hip"], X, backend=hip, **kw)
    assert calls == [4]                                             # ONE call for the four covariates
    pool, table = s.pooled_history()
    bound = _oracle_bound(pool, 15, 1.0)
    for c in range(4):
        assert got["pd"][c].shape == (8, 130, 1) and np.array_equal(got["pd"][c], np.moveaxis(want[c], 1, 2))
        diff = float(np.max(np.abs(got["pd"][c] - ref["pd"][c])))
        print(f"column {c}: max |hip - oracle backend| = {diff:.3e} (bound {bound:.3e})")
        assert diff <= bound
    assert abs(got["reference"] - ref["reference"]) <= bound


def test_summaries_without_the_matrix(fits, hip):
    X, ops = fits
    kw = dict(xs_interval="insample", samples=12, random_seed=4, backend=hip,
              summary={"quantiles": [0.1, 0.5, 0.9], "hdi_prob": 0.8})
    kept = partial_dependence(ops["hip"], X, var_idx=[2, 0], **kw)
    lean = partial_dependence(ops["hip"], X, var_idx=[2, 0], keep_pd=False, **kw)
    plain_ = partial_dependence(ops["hip"], X, var_idx=[2, 0], xs_interval="insample", samples=12, random_seed=4, backend=hip)
    means = []
    for j in (2, 0):
        assert lean["pd"][j] is None and np.array_equal(kept["pd"][j], plain_["pd"][j])
        for key in ("mean", "sd", "var", "quantiles", "hdi"):
            assert np.array_equal(lean["summary"][j][key], kept["summary"][j][key]), (j, key)
        assert lean["summary"][j]["mean"].shape == (130, 1) and lean["summary"][j]["n_draws"] == 12
        means.append(float(lean["summary"][j]["mean"][:, 0].mean()))
    assert lean["reference"] == float(np.mean(means)) and kept["reference"] == plain_["reference"]
