"""ROC AUC, KS and threshold counts per posterior draw (``include/pgbart_rank.h``, ``pymc_bart_amd/discrimination.py``)
without a GPU: the order of the keys, the pair-counting reference against an independent NumPy count, the Python layer on
the host backend under chunking and blocking, the invariances of the AUC, SciPy, every refusal, the occupancy budget and
the timing tool.  Every compared result is an integer and is compared with ``np.array_equal``."""
import importlib
import json
import os

import numpy as np
import pytest

import _rank_host as host
from pymc_bart_amd import BARTOp, BernoulliLikelihood, discrimination, discrimination_matrix
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler

disc = importlib.import_module("pymc_bart_amd.discrimination")   # (the package's attribute of that name is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX, TINY = np.finfo(np.float64).max, 5e-324     # the largest double, the smallest subnormal
INTEGERS = ("U2", "KSN", "tp", "fp")


def test_the_constants_of_the_header_are_the_modules():
    L = host.lib()
    assert L.rank_max_groups() == disc.MAX_GROUPS == 256 and L.rank_max_thresholds() == disc.MAX_THRESHOLDS == 64
    assert host.TRANSFORMS == disc.TRANSFORMS


# ------------------------------------------------------------------ 1. the key
def test_the_order_of_the_keys_is_the_order_of_the_doubles():
    up = np.nextafter
    ladder = [-np.inf, -DBL_MAX, up(-DBL_MAX, 0.0), -1e300, -2.0, up(-1.0, -2.0), -1.0, up(-1.0, 0.0), -2.2250738585072014e-308,
              up(-2.2250738585072014e-308, 0.0), -3 * TINY, -2 * TINY, -TINY, 0.0, TINY, 2 * TINY, 3 * TINY,
              up(2.2250738585072014e-308, 0.0), 2.2250738585072014e-308, up(1.0, 0.0), 1.0, up(1.0, 2.0), 2.0, 1e300,
              up(DBL_MAX, 0.0), DBL_MAX, np.inf]
    assert np.all(np.diff(ladder) > 0.0)
    keys = host.key(ladder)
    assert np.all(keys[1:] > keys[:-1])                                # strictly, in the unsigned order
    assert host.key(-0.0) == host.key(0.0) and np.signbit(-0.0)        # the two zeros share a key
    assert host.key(-TINY) < host.key(-0.0) < host.key(TINY)
    nans = [np.nan, -np.nan, np.float64(np.uint64(0x7FF0000000000001).view(np.float64)),
            np.float64(np.uint64(0xFFFFFFFFFFFFFFFF).view(np.float64))]
    assert np.all(host.key(nans) == np.uint64(host.NAN_KEY)) and host.NAN_KEY > int(keys[-1])   # a NaN is above everything
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.normal(size=500), rng.normal(size=100) * 1e-310, rng.integers(-3, 4, 100).astype(np.float64)])
    k = host.key(v)
    assert np.array_equal(k[:, None] < k[None, :], v[:, None] < v[None, :])
    assert np.array_equal(k[:, None] == k[None, :], v[:, None] == v[None, :])


# ------------------------------------------------------------------ 2. the reference against NumPy
def _case(name, rng):
    """-> ``(scores (D, n), cls, gid, G, thr)``"""
    if name == "two rows":
        return np.array([[0.3, 0.7], [0.7, 0.3], [0.5, 0.5]]), np.array([0, 1]), np.zeros(2, np.int32), 1, (0.5,)
    if name == "one positive":
        return rng.normal(size=(3, 41)), np.r_[1, np.zeros(40, int)], np.zeros(41, np.int32), 1, (0.0, 0.5)
    if name == "one negative":
        return rng.normal(size=(3, 41)), np.r_[np.ones(20, int), 0, np.ones(20, int)], np.zeros(41, np.int32), 1, (0.0,)
    if name == "all equal":
        return np.full((2, 30), 0.25), np.r_[0, 1, rng.integers(0, 2, 28)], np.zeros(30, np.int32), 1, (0.25, 0.3)
    if name == "perfect separation":
        cls = np.r_[np.zeros(17, int), np.ones(13, int)]
        return (np.arange(30.0) + 0.0)[None, :].repeat(2, 0), cls, np.zeros(30, np.int32), 1, (16.0, 16.5, 17.0)
    if name == "ties across the classes":
        return np.round(rng.normal(size=(4, 90)) * 2) / 2, rng.integers(0, 2, 90), np.zeros(90, np.int32), 1, (-0.5, 0.0, 0.5)
    if name == "infinities":
        s = rng.normal(size=(3, 50))
        s[:, [3, 9]], s[:, [4, 30]], s[1, 7] = np.inf, -np.inf, np.inf
        return s, rng.integers(0, 2, 50), np.zeros(50, np.int32), 1, (-np.inf, 0.0, np.inf)
    if name == "both zeros":
        s = np.where(rng.random((3, 40)) < 0.5, -0.0, 0.0)
        s[:, :6] = [-1.0, 1.0, -TINY, TINY, 0.0, -0.0]
        return s, np.arange(40) % 2, np.zeros(40, np.int32), 1, (0.0, -0.0, TINY)
    if name == "thresholds":
        s = rng.normal(size=(2, 60))
        return s, rng.integers(0, 2, 60), np.zeros(60, np.int32), 1, (s[0, 5], s[1, 7], s.min() - 1.0, s.max() + 1.0, s.min(), s.max(),
                                                                        -np.inf, np.inf)
    if name == "no thresholds":
        return rng.normal(size=(2, 60)), rng.integers(0, 2, 60), np.zeros(60, np.int32), 1, ()
    if name == "three groups":
        gid = np.r_[rng.integers(0, 2, 98) * 2, [1, 1]].astype(np.int32)       # group 1 has two rows
        cls = np.r_[rng.integers(0, 2, 98), [1, 0]]
        cls[:4], gid[:4] = [0, 1, 0, 1], [0, 0, 2, 2]
        order = rng.permutation(100)
        return np.round(rng.normal(size=(3, 100)), 1), cls[order], gid[order], 3, (0.0, 0.35)
    raise KeyError(name)


CASES = ["two rows", "one positive", "one negative", "all equal", "perfect separation", "ties across the classes", "infinities",
         "both zeros", "thresholds", "no thresholds", "three groups"]


@pytest.mark.parametrize("name", CASES)
def test_the_reference_equals_an_independent_numpy_count(name):
    scores, cls, gid, G, thr = _case(name, np.random.default_rng(len(name)))
    cls = np.asarray(cls, np.int32)
    got, n_nan = host.reference_scores(scores, cls, gid, G, thr)
    want = host.numpy_counts(scores, cls, gid, G, thr)
    assert n_nan == 0 and np.array_equal(got, want), (got, want)
    n1 = np.array([((gid == g) & (cls == 1)).sum() for g in range(G)])
    n0 = np.array([((gid == g) & (cls == 0)).sum() for g in range(G)])
    assert np.all(got[:, :, 0] <= 2 * n1 * n0) and np.all(got[:, :, 1] <= n1 * n0) and np.all(got >= 0)
    if name == "all equal":
        assert np.all(got[:, 0, 0] == n1[0] * n0[0]) and np.all(got[:, 0, 1] == 0)                  # AUC 1/2 exactly, KS 0
        assert got[0, 0, 2:].tolist() == [n1[0], 0, n0[0], 0]
    if name == "perfect separation":
        assert np.all(got[:, 0, 0] == 2 * n1[0] * n0[0]) and np.all(got[:, 0, 1] == n1[0] * n0[0])
        assert got[0, 0, 2:].tolist() == [13, 13, 13, 1, 0, 0]
    if name == "two rows":
        assert got[:, 0, 0].tolist() == [2, 0, 1] and got[:, 0, 1].tolist() == [1, 1, 0]
    if name == "thresholds":
        assert got[0, 0, 2 + 2] == n1[0] and got[0, 0, 2 + 3] == 0 and got[0, 0, 2 + 6] == n1[0] and got[0, 0, 2 + 7] == 0
    if name == "both zeros":
        assert np.array_equal(got[:, :, 2], got[:, :, 3]) and np.array_equal(got[:, :, 5], got[:, :, 6])   # thr 0.0 is thr -0.0


def test_the_layout_of_the_header_is_the_modules_and_a_nan_is_counted():
    rng = np.random.default_rng(5)
    n, G = 300, 4
    cls, gid = rng.integers(0, 2, n), rng.integers(0, G, n)
    seg_off, dest = host.layout(cls, gid, G)
    lay = disc.Layout(cls, gid, n)
    assert np.array_equal(seg_off, lay.seg_off) and np.array_equal(dest, lay.dest) and sorted(dest.tolist()) == list(range(n))
    s = 2 * gid + cls
    for seg in range(2 * G):
        rows = np.flatnonzero(s == seg)
        assert np.array_equal(dest[rows], np.arange(seg_off[seg], seg_off[seg + 1]))            # ascending row order
    a = rng.normal(size=(2, n))
    a[1, 17] = np.nan
    keys, counters = host.keys_block(a, "identity", dest, n)
    assert counters.tolist() == [1, 0] and keys[1, dest[17]] == np.uint64(host.NAN_KEY)
    assert np.array_equal(keys[0, dest], host.key(a[0]))
    keys, counters = host.keys_block(a[:, :5], "identity", [0, -1, n, 3, 4], n)                 # a dest out of range writes nothing
    assert counters.tolist() == [0, 4] and np.all(keys[:, 1:3] == 0)


def test_the_bounds_of_the_header():
    ok = np.array([0, 3, 5], np.int64)
    assert host.fault(2, 5, ok, 1, [0.5], 1) == (0, 0)
    assert host.fault(0, 5, ok, 1, None, 0)[0] == 1 and host.fault(1, 1, ok, 1, None, 0)[0] == 2
    assert host.fault(1, 5, ok, 0, None, 0)[0] == 3 and host.fault(1, 5, ok, 257, None, 0)[0] == 3
    assert host.fault(1, 5, ok, 1, None, -1)[0] == 4 and host.fault(1, 5, ok, 1, None, 65)[0] == 4
    assert host.fault(1, 5, None, 1, None, 0)[0] == 5 and host.fault(1, 5, ok, 1, None, 1)[0] == 6
    assert host.fault(1 << 16, 1 << 15, [0, 1, 1 << 15], 1, None, 0)[0] == 7 and host.fault(1, 1 << 31, ok, 1, None, 0)[0] == 7
    assert host.fault(1, 5, [1, 3, 5], 1, None, 0)[0] == 8 and host.fault(1, 6, ok, 1, None, 0)[0] == 8
    assert host.fault(1, 5, [0, 0, 5], 1, None, 0) == (9, 0) and host.fault(1, 5, [0, 2, 2, 4, 5], 2, None, 0) == (9, 1)
    assert host.fault(1, 5, [0, 4, 3, 4, 5], 2, None, 0) == (9, 1)
    big = 1 << 30
    assert host.fault(1, big, [0, 1 << 29, big], 1, None, 0) == (10, 0)                          # 2^58 pairs
    # 2^23 (2^30 - 2^23) >= 2^52 > 2^22 (2^30 - 2^22)
    assert host.fault(1, big, [0, 1 << 23, big], 1, None, 0)[0] == 10 and host.fault(1, big, [0, 1 << 22, big], 1, None, 0)[0] == 0
    assert host.fault(1, 1 << 27, [0, 1 << 26, 1 << 27], 1, None, 0)[0] == 10                      # 2^26 2^26 = 2^52 exactly
    assert host.fault(1, 5, ok, 1, [0.5, np.nan], 2) == (11, 1) and host.fault(1, 5, ok, 1, [np.inf, -np.inf], 2) == (0, 0)


# ------------------------------------------------------------------ 3. the Python layer on the host backend
N_BIG = 4300    # (one draw's keys, twice, are more than the 64 KiB floor of PGB_PW_BLOCK_BYTES)


@pytest.fixture(scope="module")
def chain(oracle):
    """A short probit chain of the oracle (80 rows, 3 covariates, m = 5, four draws), read at 4300 new rows."""
    rng = np.random.default_rng(43)
    Z = rng.normal(size=(80, 3))
    yz = (rng.random(80) < np.where(Z[:, 0] > 0, 0.8, 0.2)).astype(np.float64)
    op = BARTOp(Z, yz, m=5)
    attach_history(op, [sample_chain(op, 6, 4, num_particles=5, random_seed=3, backend=oracle, keep_draws=False,
                                     likelihood=BernoulliLikelihood("probit"))])
    s = _get_posterior_sampler(op, backend=oracle)
    pool, table = (s.pooled_history() if hasattr(s, "pooled_history") else (s.pool, s.forest_idx))
    pool = pool.decoded() if hasattr(pool, "decoded") else pool
    table = np.ascontiguousarray(np.asarray(table), np.int32)
    be = host.HostBackend(oracle, pool)
    s = PosteriorSampler(pool, table, table.shape[1], pool.n_outputs, backend=be)
    X = rng.normal(size=(N_BIG, 3))
    y = (rng.random(N_BIG) < np.where(X[:, 0] > 0, 0.8, 0.2)).astype(np.int64)
    groups = np.where(X[:, 1] > 0.5, "b", "a")
    f = np.asarray(PosteriorSampler(pool, table, table.shape[1], pool.n_outputs, backend=oracle).sample_posterior(
        X, list(range(table.shape[0])), None))[:, 0, :]
    return be, s, X, y, groups, f


def _same(got, want, draws=slice(None)):
    for key in INTEGERS:
        assert got[key].dtype == np.int64 and np.array_equal(got[key], want[key][draws]), key
    for key in ("auc", "ks", "tpr", "fpr", "precision"):
        assert np.array_equal(got[key], want[key][draws], equal_nan=True), key


def test_one_chunk_one_draw_per_chunk_with_blocks_of_64_rows_and_permuted_draws(chain, monkeypatch):
    be, s, X, y, groups, f = chain
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    thr = (0.2, 0.5)
    off = np.random.default_rng(44).normal(0, 0.2, N_BIG)
    kw = dict(groups=groups, thresholds=thr, transform="probit", offset=off)
    del be.key_calls[:], be.metric_calls[:]
    whole = discrimination(s, X, y, **kw)
    assert whole["n_chunks"] == 1 and be.metric_calls == [4] and be.key_calls == [(4, N_BIG)]
    assert whole["auc"].shape == (4, 2) and whole["tp"].shape == (4, 2, 2) and whole["group_labels"].tolist() == ["a", "b"]
    assert whole["auc_mean"].shape == (2,) and whole["auc_hdi"].shape == (2, 2) and whole["ks_sd"].shape == (2,)
    # the definition: the header's value of the oracle's predictions, counted by NumPy
    gid = (groups == "b").astype(np.int32)
    want = host.numpy_counts(host.value(f, "probit", off), y, gid, 2, thr)
    assert np.array_equal(whole["U2"], want[:, :, 0]) and np.array_equal(whole["KSN"], want[:, :, 1])
    assert np.array_equal(whole["tp"], want[:, :, 2:4]) and np.array_equal(whole["fp"], want[:, :, 4:6])
    assert np.array_equal(whole["n_pos"] + whole["n_neg"], np.bincount(gid)) and np.all(whole["auc_mean"] > 0.6)
    assert np.array_equal(whole["auc"], whole["U2"] / (2.0 * whole["n_pos"] * whole["n_neg"]))
    assert np.array_equal(whole["tpr"], whole["tp"] / whole["n_pos"][None, :, None].astype(np.float64))
    # one draw per chunk, blocks of 64 rows
    run = disc.RankRun(be, disc.Layout(y, groups, N_BIG), np.asarray(thr), 4)
    row = 8 * 3 + 8 + 8 + 8
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(run.reserved(1) + 100 * row))
    assert run.reserved(1) > 65536 and run.chunk_draws(lambda dc: 8 * 3 + 8 * dc + 16) == 1
    del be.key_calls[:], be.metric_calls[:]
    cut = discrimination(s, X, y, **kw)
    assert cut["n_chunks"] == 4 and be.metric_calls == [1] * 4 and set(be.key_calls) == {(1, 64), (1, N_BIG % 64)}
    _same(cut, whole)
    order = [2, 0, 3]
    _same(discrimination(s, X, y, draws=order, **kw), whole, order)                        # chunks of one draw still
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES")
    _same(discrimination(s, X, y, draws=order, **kw), whole, order)
    # the matrix route: the same integers from the scores themselves
    v = host.value(f, "probit", off)
    _same(discrimination_matrix(v, y, groups, thr, backend=be), whole)
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(run.reserved(1) + 100 * 16))
    _same(discrimination_matrix(v, y, groups, thr, backend=be), whole)
    one = discrimination_matrix(v[1], y, backend=be)                                     # a vector is one draw; no thresholds
    assert one["auc"].shape == (1, 1) and "tp" not in one and one["n_pos"].tolist() == [int(y.sum())]


# ------------------------------------------------------------------ 4. invariances
def test_the_auc_of_negated_scores_and_of_increasing_maps(chain):
    be = chain[0]
    rng = np.random.default_rng(45)
    v = np.round(rng.normal(size=(5, 400)), 1)                                             # with ties
    y, g = rng.integers(0, 2, 400), rng.integers(0, 3, 400)
    a = discrimination_matrix(v, y, g, backend=be)
    b = discrimination_matrix(-v, y, g, backend=be)
    assert np.array_equal(a["U2"] + b["U2"], np.broadcast_to(2 * a["n_pos"] * a["n_neg"], a["U2"].shape))
    assert np.allclose(b["auc"], 1.0 - a["auc"], rtol=0, atol=2.0 ** -52) and np.array_equal(a["KSN"], b["KSN"])
    for fn in (np.exp, lambda x: 3.0 * x - 7.0, lambda x: x ** 3, np.arctan):              # strictly increasing on these values
        c = discrimination_matrix(fn(v), y, g, backend=be)
        assert np.array_equal(c["U2"], a["U2"]) and np.array_equal(c["KSN"], a["KSN"]) and np.array_equal(c["auc"], a["auc"])


# ------------------------------------------------------------------ 5. SciPy
def test_scipy_mann_whitney_and_two_sample_ks(chain):
    """``U2 / 2`` is SciPy's Mann-Whitney statistic exactly (halves are representable); ``ks`` is ``ks_2samp``'s
    statistic WITHIN ONE ROUNDING OF THE DIVISION: SciPy subtracts two rounded quotients, ``i / n1 - j / n0``, this
    library divides the exact integer ``|i n0 - j n1|`` once."""
    stats = pytest.importorskip("scipy.stats")
    be = chain[0]
    rng = np.random.default_rng(46)
    for n, levels in ((200, None), (333, 8)):
        v = rng.normal(size=(3, n))
        v = v if levels is None else np.round(v * levels / 4) / (levels / 4)
        y = rng.integers(0, 2, n)
        r = discrimination_matrix(v, y, backend=be)
        for d in range(3):
            pos, neg = v[d, y == 1], v[d, y == 0]
            assert r["U2"][d, 0] / 2.0 == stats.mannwhitneyu(pos, neg, alternative="two-sided", method="asymptotic").statistic
            ks = stats.ks_2samp(pos, neg, method="asymp").statistic
            assert abs(r["ks"][d, 0] - ks) <= 2.0 ** -52, (r["ks"][d, 0], ks)


# ------------------------------------------------------------------ 6. refusals
def test_every_refusal_of_the_python_layer(chain, oracle, monkeypatch):
    be, s, X, y, groups, f = chain
    NR = 600
    X, y, groups = X[:NR], y[:NR], groups[:NR]
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    bad = [
        (dict(y=y[:-1]), "y must hold one value per row"), (dict(y=np.where(y == 1, 2, 0)), "y must hold 0 or 1"),
        (dict(y=y + 0.5), "y must hold 0 or 1"), (dict(y=np.where(np.arange(NR) == 3, np.nan, y)), "y must hold 0 or 1"),
        (dict(y=["a"] * NR), "y must hold 0 or 1"),
        (dict(y=np.zeros(NR)), "holds no row with y == 1"), (dict(y=np.ones(NR)), "holds no row with y == 0"),
        (dict(groups=np.where(np.arange(NR) == 0, "lonely", groups)), "group 'lonely' holds no row with y =="),
        (dict(groups=groups[:-1]), "groups must hold one label per row"),
        (dict(groups=np.arange(NR) % 300), "at most 256 groups"),
        (dict(thresholds=np.linspace(0, 1, 65)), "at most 64 thresholds"), (dict(thresholds=[0.5, np.nan]), "thresholds must not hold a NaN"),
        (dict(thresholds=[[0.5]]), "thresholds must be a vector"),
        (dict(transform="logit"), "unknown transform 'logit'"), (dict(offset=np.zeros(NR - 1)), "offset must have shape"),
        (dict(excluded=[3]), "excluded must index"), (dict(draws=[4]), "draws must index the 4 stored draws"),
        (dict(draws=[]), "discrimination needs at least 1 draw"),
    ]
    for change, msg in bad:
        kw = dict(dict(y=y, groups=groups, thresholds=(0.5,), transform="probit"), **change)
        with pytest.raises(ValueError, match=msg):
            discrimination(s, X, kw.pop("y"), **kw)
    with pytest.raises(ValueError, match="at least 2 rows"):
        discrimination(s, X[:1], y[:1])
    for change, msg in bad[:13]:
        kw = dict(dict(y=y, groups=groups, thresholds=(0.5,)), **change)
        with pytest.raises(ValueError, match=msg):
            discrimination_matrix(f[:, :NR], kw.pop("y"), backend=be, **kw)
    with pytest.raises(ValueError, match="scores must be a matrix"):
        discrimination_matrix(np.zeros((2, 3, 4)), y, backend=be)
    with pytest.raises(ValueError, match="y must hold one value per row"):
        discrimination_matrix(f[:, :NR - 1], y, backend=be)

    class Resident:                                                                       # what a device tensor looks like
        shape = (600, 3)

        def data_ptr(self):
            return 0
    with pytest.raises(ValueError, match="device-resident X"):
        discrimination(s, Resident(), y)
    # a fit with several outputs
    rng = np.random.default_rng(47)
    import _ice_host as ice_host

    pool3 = ice_host.random_pool(rng, 8, 3, K=3, depth=3)
    s3 = ice_host.pool_sampler(rng, pool3, 4, 2, host.HostBackend(oracle, pool3))
    with pytest.raises(ValueError, match="takes a fit with one output, this one has 3"):
        discrimination(s3, X, y)
    # a NaN score
    v = f[:, :NR].copy()
    v[2, 11] = v[0, 5] = np.nan
    with pytest.raises(ValueError, match="2 of the 2400 scores are NaN: the AUC of NaN scores is undefined"):
        discrimination_matrix(v, y, backend=be)
    # not even one draw fits
    big = chain[2]
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")
    with pytest.raises(ValueError, match="PGB_PW_BLOCK_BYTES"):
        discrimination(s, big, chain[3])
    with pytest.raises(ValueError, match="PGB_PW_BLOCK_BYTES"):
        discrimination_matrix(f, chain[3], backend=be)


def test_the_cpu_oracle_is_refused_naming_the_entry_point(oracle, chain):
    be, s, X, y, groups, f = chain
    with pytest.raises(NotImplementedError, match="pgb_rank_metrics"):
        discrimination(s, X[:100], y[:100], backend=oracle)
    with pytest.raises(NotImplementedError, match="pgb_rank_metrics"):
        discrimination_matrix(f[:, :100], y[:100], backend=oracle)
    with pytest.raises(NotImplementedError, match="pgb_rank_kernel_ms"):
        oracle.lib.rank_kernel_ms()


# ------------------------------------------------------------------ 7. the budget and the timing tool
def test_the_kernels_are_in_the_occupancy_budget_with_no_scratch_and_no_spills():
    budget = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    for name in ("k_rank_keys", "k_rank_count"):
        assert budget[name]["max_scratch_bytes"] == 0 and budget[name]["max_vgpr_spills"] == 0, name


def test_the_timing_tool_answers_help():
    import subprocess
    import sys

    tool = os.path.join(ROOT, "tools", "timing_discrimination.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--baseline-root" in r.stdout
