"""Accumulated local effects on the MI355X: ``pgb_predict_ale`` (``k_ale_bins``, ``k_ale``) against the host reference of
``tests/_ale_host.py`` -- the header's bin, the oracle's ``pgb_predict`` of the use lists at the two edges, one NumPy
rounding -- bit for bit, over the row counts, bin counts, widths, outputs, leaf kinds, split rules, list lengths and
NaN / infinity patterns at which the kernels take another path; every refusal; then ``accumulated_local_effects`` end
to end on a two-chain fit, against itself under blocking and against the route before it (``average_contrast`` on two
edge copies of ``X``).

The one tolerance is the issue's, derived in :func:`test_the_sampled_fit_against_the_route_before`'s docstring;
everything else is ``np.array_equal`` on the bits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _ale_host as host
import _ice_host as ice_host
import _permimp_host as permimp
import _predict_exact as ex
from pymc_bart_amd import BARTOp, _abi, accumulated_local_effects, average_contrast
from pymc_bart_amd import ale as ale_mod
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAXP = int(re.search(r"#define PRED_LDS_MAXP (\d+)", open(os.path.join(ROOT, "pymc_bart_amd", "csrc", "pgb_pred_walk.h")).read()).group(1))
ONEHOT, SUBSET = _abi.RULE_ONEHOT, _abi.RULE_SUBSET
GUARD = -7.75e300    # the outputs before a call and behind them after it: no refused call may touch it
BIN_GUARD = -77
POISON = 7.0e77      # the padding of ldx > p: no result may show it
E_INVALID = -1


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _call(hip, pool, table, block, cols, edges, picks, pad=3, change=None):
    """The entry point itself on the rows ``block`` with a leading dimension of ``p + pad`` -> ``(rc, out (q, n_picks, K,
    nb), bins (q, nb), the guards behind both)``.  ``change``: arguments replaced after everything is laid out (the
    refusals)."""
    mem, lib = hip.mem, hip.lib
    nb, p = block.shape
    K = int(pool.n_outputs)
    table = np.ascontiguousarray(table, np.int32)
    cols, picks = np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(picks, np.int32)
    flat, off = host.flat_edges(edges)
    wide = np.full((nb, p + pad), POISON)
    wide[:, :p] = block
    xd = mem.from_host(wide)
    cells, n_bins = cols.size * picks.size * K * nb, cols.size * nb
    od = mem.from_host(np.full(cells + 64, GUARD))
    bd = mem.from_host(np.full(n_bins + 64, BIN_GUARD, np.int32))
    carr = pool.as_c()
    a = dict(fidx=table.ctypes.data, n_forests=table.shape[0], m=table.shape[1], X_dev=mem.ptr(xd), nb=nb, p=p, ldx=p + pad,
             cols=cols.ctypes.data, q=cols.size, edges=flat.ctypes.data, edge_off=off.ctypes.data, picks=picks.ctypes.data,
             n_picks=picks.size, out=mem.ptr(od), bins=mem.ptr(bd))
    a.update(change or {})
    rc = lib.predict_ale_entry_point()(C.byref(carr), a["fidx"], a["n_forests"], a["m"], a["X_dev"], a["nb"], a["p"], a["ldx"],
                                       a["cols"], a["q"], a["edges"], a["edge_off"], a["picks"], a["n_picks"], a["out"],
                                       a["bins"], mem.stream_ptr)
    got, gb = mem.to_host(od), mem.to_host(bd)
    return rc, got[:cells].reshape(cols.size, picks.size, K, nb), gb[:n_bins].reshape(cols.size, nb), (got[cells:], gb[n_bins:])


def _check(hip, oracle, pool, table, block, cols, edges, picks, pad=3):
    """Against the host reference, bit for bit; the guards untouched.  -> ``(out, bins)``."""
    rc, got, gb, (g_out, g_bins) = _call(hip, pool, table, block, cols, edges, picks, pad)
    hip.lib.check(rc, "pgb_predict_ale")
    want, wb = host.reference_block(oracle, pool, table, block, list(cols), edges, picks)
    assert np.all(g_out == GUARD) and np.all(g_bins == BIN_GUARD)
    assert np.array_equal(gb, wb), int((gb != wb).sum())
    assert np.array_equal(bits(got), bits(want)), (int((bits(got) != bits(want)).sum()), got.size)
    return got, gb


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


def _edges(rng, B, lo=-2.5, hi=2.5):
    """``B + 1`` increasing edges inside the bulk of a normal column, so that rows fall below, between and above."""
    e = np.sort(rng.uniform(lo, hi, B + 1))
    assert np.all(np.diff(e) > 0)
    return e


# ------------------------------------------------------------------ 1. row counts, list lengths, bin counts, picks
BINS_OF = (1, 2, 7, 1024, 7, 2)


@pytest.fixture(scope="module")
def lengths():
    """Use lists of 1, 3, 4, 8, 9 and 0 trees: both sides of PRED_WALKS and of its prefetch; K = 1; the columns have 1,
    2, 7, 1024, 7 and 2 bins."""
    rng = np.random.default_rng(101)
    pool = permimp.lengths_pool(rng, 1)
    table = _forests(rng, 12, 12, 3)                                   # the same trees in three orders
    off, _ = permimp.use_lists(pool, table, 6, list(range(6)))
    assert np.diff(off).reshape(3, 6).tolist() == [list(permimp.LENGTHS) + [0]] * 3
    return pool, table, _rows(rng, 130, 6), [_edges(rng, B) for B in BINS_OF]


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 130])
def test_row_counts_list_lengths_and_bin_counts(hip, oracle, lengths, nb):
    pool, table, X, edges = lengths
    out, bins = _check(hip, oracle, pool, table, X[:nb], list(range(6)), edges, [0, 2, 0])      # a repeated pick
    assert np.array_equal(bits(out[:, 0]), bits(out[:, 2]))
    assert np.all(bits(out[5]) == 0)                                   # the unused column: +0.0 everywhere
    if nb >= 63:
        assert np.count_nonzero(out[:5]) > 0 and len(set(bins[3].tolist())) > 30
        missing = bins == (np.asarray(BINS_OF)[:, None])
        assert missing.any() and np.all(bits(out)[np.broadcast_to(missing[:, None, None, :], out.shape)] == 0)


def test_clean_rows_take_the_fixed_length_walk_too(hip, oracle, lengths):
    pool, table, X, edges = lengths
    clean = np.nan_to_num(X, nan=0.25)
    cols = [4, 0, 3, 5]
    out, bins = _check(hip, oracle, pool, table, clean, cols, [edges[c] for c in cols], [1])
    assert np.all(bins < np.asarray([BINS_OF[c] for c in cols])[:, None]) and np.count_nonzero(out) > 0


def test_three_outputs_and_linear_leaves_that_regress_on_the_swept_column(hip, oracle):
    rng = np.random.default_rng(102)
    pool = permimp.lengths_pool(rng, 3, linear=True)                    # tree 0: leaves regress on column 4 or 5
    table = _forests(rng, 12, 12, 2)
    X = _rows(rng, 100, 6)
    cols = [4, 5, 1]
    out, _ = _check(hip, oracle, pool, table, X, cols, [_edges(rng, 5), _edges(rng, 3), _edges(rng, 7)], [1, 0])
    assert out.shape == (3, 2, 3, 100) and all(np.count_nonzero(out[s]) > 0 for s in range(3))


def test_two_calls_are_the_slices_of_one(hip, lengths):
    pool, table, X, edges = lengths
    cols, picks = [3, 1, 4], [2, 1]
    mine = [edges[c] for c in cols]
    _, whole, wb, _ = _call(hip, pool, table, X, cols, mine, picks)
    _, a, ab, _ = _call(hip, pool, table, X[:64], cols, mine, picks)
    _, b, bb, _ = _call(hip, pool, table, X[64:], cols, mine, picks, pad=0)
    assert np.array_equal(bits(whole[..., :64]), bits(a)) and np.array_equal(bits(whole[..., 64:]), bits(b))
    assert np.array_equal(wb[:, :64], ab) and np.array_equal(wb[:, 64:], bb)


# ------------------------------------------------------------------ 2. widths, outputs, trees per forest, leaves, rules
@pytest.mark.parametrize("p,K,m,linear", [(3, 1, 1, False), (3, 3, 12, True), (LDS_MAXP + 1, 1, 12, True),
                                          (LDS_MAXP + 1, 3, 1, False)])
def test_widths_outputs_and_forest_sizes(hip, oracle, p, K, m, linear):
    """p = 3 is staged in LDS, p = 127 is the first width read from global memory; constant and linear leaves."""
    rng = np.random.default_rng(200 + p + K)
    pool = ice_host.random_pool(rng, 2 * m + 2, p, K=K, depth=5, linear=[0, p - 1] if linear else None)
    table = _forests(rng, pool.n_trees, m, 3)
    X = _rows(rng, 70, p)
    cols = [p - 1, 0, 1] if p == 3 else [p - 1, 0, 64, 5]
    _check(hip, oracle, pool, table, X, cols, [_edges(rng, B) for B in (4, 1, 9, 2)[:len(cols)]], [2, 0])


@pytest.mark.parametrize("p,K", [(5, 1), (5, 3), (LDS_MAXP + 1, 1)])
def test_one_hot_and_subset_rules(hip, oracle, p, K):
    """The instances without the continuous rule, staged and not; the code columns with one bin per step."""
    rng = np.random.default_rng(300 + p + K)
    rules = [0, ONEHOT, 0, SUBSET, 0] + [0] * (p - 5)
    pool = ice_host.random_pool(rng, 16, p, K=K, depth=5, rules=rules, linear=[2, 4], split_cols=[0, 1, 2, 3, 4])
    table = _forests(rng, 16, 8, 2)
    X = _rows(rng, 130, p, rules)
    edges = [np.arange(4.0), np.arange(8.0), _edges(rng, 6), _edges(rng, 3)]
    out, _ = _check(hip, oracle, pool, table, X[64:], [1, 3, 0, 4], edges, [0, 1])
    assert np.count_nonzero(out[0]) > 0 and np.count_nonzero(out[1]) > 0


# ------------------------------------------------------------------ 3. NaN and the infinities
def test_nan_and_infinities_in_the_swept_column_and_in_the_others_only(hip, oracle, lengths):
    pool, table, X, edges = lengths
    X = np.nan_to_num(X, nan=-0.5)
    only_swept, only_others = X.copy(), X.copy()
    only_swept[0::5, 3], only_swept[1::7, 3], only_swept[2::11, 3] = np.nan, np.inf, -np.inf
    only_others[0::5, 4], only_others[1::7, 0], only_others[2::11, 0] = np.nan, np.inf, -np.inf
    cols = [3, 2]
    mine = [edges[c] for c in cols]
    out, bins = _check(hip, oracle, pool, table, only_swept, cols, mine, [0, 1])
    x = only_swept[:, 3]
    assert np.isnan(x).sum() > 10 and (x == np.inf).sum() > 5 and (x == -np.inf).sum() > 5
    assert np.all(bins[0][np.isnan(x)] == 1024) and np.all(bins[0][x == np.inf] == 1023) and np.all(bins[0][x == -np.inf] == 0)
    assert np.all(bits(out[0][..., np.isnan(x)]) == 0) and np.all(np.isfinite(out))
    _check(hip, oracle, pool, table, only_others, cols, mine, [0, 1])


# ------------------------------------------------------------------ 4. refusals
def test_every_refusal_leaves_both_outputs_untouched(hip, lengths):
    pool, table, X, edges = lengths
    cols = [2, 0, 4]
    mine = [edges[c] for c in cols]                                     # 7, 1 and 7 bins: 8 + 2 + 8 edges
    flat, off = host.flat_edges(mine)
    i32 = lambda *v: np.array(v, np.int32)  # noqa: E731
    bad_cols, twice, bad_picks, many = i32(0, 9, 1), i32(2, 0, 2), i32(0, 3), np.zeros(1 << 22, np.int32)
    off_from_1, off_by_1, off_back = i32(1, 8, 10, 18), i32(0, 8, 9, 18), i32(0, 8, 6, 18)
    long_off, long_edges = i32(0, 1026, 1028, 1036), np.arange(1036.0)
    e_inf, e_nan, e_same, e_down = (flat.copy() for _ in range(4))
    e_inf[9], e_nan[3], e_same[12], e_down[1] = np.inf, np.nan, e_same[11], e_down[0] - 1.0
    cases = [
        (dict(X_dev=None), "X_dev is null"), (dict(cols=None), "cols_host is null"), (dict(edges=None), "edges_host is null"),
        (dict(edge_off=None), "edge_off_host is null"), (dict(picks=None), "picks_host is null"),
        (dict(fidx=None), "forest_tree_idx is null"), (dict(out=None), "out_dev is null"), (dict(bins=None), "bins_out_dev is null"),
        (dict(m=0), "n_forests, m and p must be >= 1"), (dict(n_forests=0), "n_forests, m and p must be >= 1"),
        (dict(p=0), "n_forests, m and p must be >= 1"), (dict(nb=0), "nb must be >= 1"), (dict(q=0), "q must be >= 1"),
        (dict(n_picks=0), "n_picks must be >= 1"), (dict(ldx=5), "ldx must be >= p"),
        (dict(cols=bad_cols.ctypes.data), "cols_host[1] = 9 is outside [0, p = 6)"),
        (dict(cols=twice.ctypes.data), "repeats cols_host"),
        (dict(picks=bad_picks.ctypes.data), "picks_host[1] = 3 is outside [0, n_forests = 3)"),
        (dict(edge_off=off_from_1.ctypes.data), "edge_off_host[0] = 1 must be 0"),
        (dict(edge_off=off_by_1.ctypes.data), "edge_off_host[2] = 9 must be >= edge_off_host[1] + 2"),
        (dict(edge_off=off_back.ctypes.data), "edge_off_host[2] = 6 must be >= edge_off_host[1] + 2"),
        (dict(edge_off=long_off.ctypes.data, edges=long_edges.ctypes.data), "slot 0 of edges_host holds 1026 edges"),
        (dict(edges=e_inf.ctypes.data), "edges_host[9] (slot 1) is not finite"),
        (dict(edges=e_nan.ctypes.data), "edges_host[3] (slot 0) is not finite"),
        (dict(edges=e_same.ctypes.data), "edges_host[12] (slot 2) is not above its predecessor"),
        (dict(edges=e_down.ctypes.data), "edges_host[1] (slot 0) is not above its predecessor"),
        (dict(nb=(1 << 37) - 64, picks=many.ctypes.data, n_picks=1 << 22), "overflows a 64-bit size"),
    ]
    assert off.tolist() == [0, 8, 10, 18]
    for change, msg in cases:
        rc, got, gb, (g_out, g_bins) = _call(hip, pool, table, X, cols, mine, [0, 1], change=change)
        text = hip.lib.lib.pgb_last_error().decode()
        assert rc == E_INVALID and msg in text and text.startswith("pgb_predict_ale: "), (change, rc, text)
        assert np.all(got == GUARD) and np.all(g_out == GUARD) and np.all(gb == BIN_GUARD) and np.all(g_bins == BIN_GUARD), change
    table_bad = table.copy()                                           # a malformed history: pgb_predict's checks
    table_bad[1, 3] = 12
    rc, got, gb, _ = _call(hip, pool, table, X, cols, mine, [0, 1], change=dict(fidx=table_bad.ctypes.data))
    assert rc == E_INVALID and "forest_tree_idx entry outside" in hip.lib.lib.pgb_last_error().decode()
    assert np.all(got == GUARD) and np.all(gb == BIN_GUARD)


# ------------------------------------------------------------------ 5. end to end
N_FIT, M_FIT = 300, 10
LIST_KEYS = ("ale", "mean", "sd", "hdi", "local_effect", "local_var", "bin_weight", "edges")


@pytest.fixture(scope="module")
def fit(hip):
    """Two chains of 12 draws behind one sampler; only columns 0 and 1 carry signal; columns 0 and 2 are correlated."""
    rng = np.random.default_rng(61)
    X = rng.uniform(-1, 1, size=(N_FIT, 6))
    X[:, 2] = 0.7 * X[:, 0] + 0.3 * X[:, 2]
    y = 2.0 * X[:, 0] + np.where(X[:, 1] > 0, 1.5, -1.5) + rng.normal(0, 0.3, N_FIT)
    op = BARTOp(X, y, m=M_FIT)
    attach_history(op, [sample_chain(op, 30, 12, random_seed=4, chain=c, backend=hip, keep_draws=False) for c in (0, 1)])
    Xm = X.copy()
    Xm[5::17, 1], Xm[3::29, 4] = np.nan, np.nan                         # missing values in a swept and in a noise column
    return Xm, rng.uniform(0.5, 2.0, N_FIT), _get_posterior_sampler(op, backend=hip)


def _history(s):
    pool, table = s.pooled_history() if hasattr(s, "pooled_history") else (s.pool, s.forest_idx)
    return (pool.decoded() if hasattr(pool, "decoded") else pool), np.asarray(table)


def _same_lists(got, want, keys=LIST_KEYS, pick=lambda a: a):
    for key in keys:
        assert len(got[key]) == len(want[key]), key
        for s, (a, b) in enumerate(zip(got[key], want[key])):
            assert np.array_equal(bits(a), bits(pick(b))), (key, s)


def test_blocks_chunks_subsets_of_columns_and_of_draws_change_no_bit(hip, fit, monkeypatch):
    X, w, s = fit
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    whole = accumulated_local_effects(s, X, bins=8, weights=w)
    assert whole["n_draws"] == 24 and whole["cols"].tolist() == list(range(6)) and whole["n_nonfinite"] == 0
    assert whole["n_missing"].tolist() == [0, 18, 0, 0, 11, 0] and [e.size for e in whole["edges"]] == [9] * 6
    draws = [1, 8, 13, 22]
    few = accumulated_local_effects(s, X, bins=8, weights=w, draws=draws)
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")                  # chunks of columns, blocks of 64 rows
    job = ale_mod.AleJob(s, X, None, 8, None, w, draws, 0.94)
    assert job.chunk < 6 and job.row_bytes(job.chunk) * N_FIT > 65536 - job.reserved(range(job.chunk))
    small = accumulated_local_effects(s, X, bins=8, weights=w, draws=draws)
    _same_lists(small, few)
    for key in ("importance", "importance_mean", "importance_hdi", "n_missing"):
        assert np.array_equal(bits(small[key]), bits(few[key])), key
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    monkeypatch.setattr(ale_mod.AleJob, "columns_per_chunk", lambda self: 1)
    _same_lists(accumulated_local_effects(s, X, bins=8, weights=w, draws=draws), few)
    monkeypatch.undo()
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    _same_lists(few, whole, keys=("ale", "local_effect", "local_var"), pick=lambda a: a[draws])
    some = accumulated_local_effects(s, X, cols=[3, 1], bins=8, weights=w)
    for key in LIST_KEYS:
        for j, c in enumerate([3, 1]):
            assert np.array_equal(bits(some[key][j]), bits(whole[key][c])), (key, c)
    assert np.array_equal(bits(some["importance"]), bits(whole["importance"][:, [3, 1]]))
    # the signal columns matter, the noise columns do not
    mean = whole["importance_mean"]
    print("importance_mean:", np.array2string(mean, precision=4))
    assert mean[:2].min() > mean[3:].max()


def _route_before(s, X, w, c, e, draws=None):
    """``average_contrast(X_hi, X_lo, weights=..., groups=bin)["mean"]`` of column ``c`` -> ``(D, B)``; a row with a NaN
    in the column keeps it in both copies and goes to a group of its own."""
    B = e.size - 1
    b = np.where(np.isnan(X[:, c]), B, np.searchsorted(e[1:B], X[:, c], side="left"))
    at = np.minimum(b, B - 1)
    X_hi, X_lo = X.copy(), X.copy()
    X_hi[:, c] = np.where(b == B, np.nan, e[at + 1])
    X_lo[:, c] = np.where(b == B, np.nan, e[at])
    got = average_contrast(s, X_hi, X_lo, weights=w, groups=b, draws=draws)
    assert got["group_labels"].tolist()[:B] == list(range(B))           # every bin holds rows
    return got["mean"][:, :B, 0], b


def test_where_every_tree_uses_every_column_the_route_before_has_the_same_bits(hip, monkeypatch):
    """Complete trees over all the columns asked for: the use list of every (draw, column) is the forest itself, so
    both routes add the same leaves in the same order, subtract once and reduce the same rows."""
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    rng = np.random.default_rng(71)
    cols = [0, 2, 3]
    roots = [ex.complete_tree(rng, 1, 3, list(rng.permutation(cols)), lambda r, j: float(r.normal(0, 0.6)), counts="free")
             for _ in range(14)]
    pool = ex.build_pool(roots, 1)
    table = _forests(rng, 14, 9, 5)
    off, _ = permimp.use_lists(pool, table, 4, cols)
    assert np.all(np.diff(off) == 9)
    X = rng.normal(size=(200, 4))
    X[4::23, 2] = np.nan                                               # a missing bin; NaN elsewhere is marginalised by both
    X[6::31, 1] = np.nan
    w = rng.uniform(0.5, 2.0, 200)
    s = PosteriorSampler(pool, table, 9, 1, backend=hip)
    res = accumulated_local_effects(s, X, cols=cols, bins=7, weights=w)
    for j, c in enumerate(cols):
        want, b = _route_before(s, X, w, c, res["edges"][j])
        assert np.array_equal(bits(res["local_effect"][j]), bits(want)), c
        assert np.allclose(res["bin_weight"][j], np.bincount(b, weights=w, minlength=8)[:7], rtol=1e-12, atol=0.0)
    assert res["n_missing"].tolist() == [0, int(np.isnan(X[:, 2]).sum()), 0]


def test_the_sampled_fit_against_the_route_before(hip, fit, monkeypatch):
    """``local_effect`` against ``average_contrast`` on the two edge copies of ``X``, per column, within
    ``8 m 2^-53 S``: ``S`` is the largest, over the draws, of the sum over a draw's trees of the tree's largest
    ``|leaf|`` (computed from the pool below).  Each side forms two ``m``-term sums in an order of its own -- the use
    list and then nothing, against the whole forest -- whose roundings are each within ``m 2^-53 S``; the bound is twice
    that of the two sums of either side.  The reference alone decides it; nothing is tuned on the device's output."""
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    X, w, s = fit
    pool, table = _history(s)
    K = int(pool.n_outputs)
    leaf = np.asarray(pool.var) < 0
    top = np.abs(np.asarray(pool.value, np.float64).reshape(-1, K)).max(axis=1) * leaf
    per_tree = np.array([top[pool.node_off[t]:pool.node_off[t + 1]].max() for t in range(pool.n_trees)])
    S = float(per_tree[table].sum(axis=1).max())
    bound = 8 * M_FIT * 2.0 ** -53 * S
    res = accumulated_local_effects(s, X, bins=8, weights=w)
    worst = 0.0
    for c in range(6):
        want, _ = _route_before(s, X, w, c, res["edges"][c])
        err = float(np.abs(res["local_effect"][c] - want).max())
        print(f"column {c}: max |local_effect - route before| = {err:.3e}, bound {bound:.3e}")
        worst = max(worst, err)
        assert err <= bound, (c, err, bound)
    assert S > 0.0 and np.any(res["local_effect"][0] != 0.0)
    print(f"max |local_effect - route before| / bound = {worst / bound:.3f}")
