"""Optimal arm and policy value on the MI355X: ``pgb_predict_arms`` (``k_arms``) and ``pgb_arm_decide`` +
``pgb_arm_decide_finish`` (``k_arms_best``, ``k_arms_rows``, ``k_arms_bayes``, ``k_arms_reduce``, ``k_arms_finish``)
against the host references of ``tests/_arms_host.py`` -- the header's packer, the oracle's ``pgb_predict`` of the union
lists at the row and under each arm, two NumPy roundings; the header's own ``pgb_arms_block`` / ``pgb_arms_finish`` --
bit for bit, over the row counts, arm counts, column counts, draws, outputs, groups, widths, list lengths, split rules,
leaf kinds and NaN / infinity patterns at which the kernels take another path; every refusal; then ``optimal_arm`` and
``arm_predictions`` end to end on a two-chain fit.

The one tolerance is the issue's, derived in :func:`test_arm_predictions_against_plain_predictions_of_copies`'s
docstring; everything else is ``np.array_equal`` on the bits.  "Bit for bit" is the 64-bit pattern of every output that is
a number; a NaN on both sides counts as equal (the sign and payload of a NaN an operation GENERATES -- inf - inf,
0 * inf -- are the hardware's, not the contract's: ``tests/test_rowreduce_gpu.py``)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _arms_host as host
import _ice_host as ice_host
import _permimp_host as permimp
from pymc_bart_amd import BARTOp, _abi, arm_predictions, optimal_arm
from pymc_bart_amd import decision as dec
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAXP = int(re.search(r"#define PRED_LDS_MAXP (\d+)", open(os.path.join(ROOT, "pymc_bart_amd", "csrc", "pgb_pred_walk.h")).read()).group(1))
ONEHOT, SUBSET = _abi.RULE_ONEHOT, _abi.RULE_SUBSET
GUARD = -7.75e300    # the outputs before a call and behind them after it: no refused call may touch it
INT_GUARD = -77
POISON = 7.0e77      # the padding of ldx > p: no result may show it
E_INVALID = -1
PER_ROW = ("p_best", "mean_utility", "expected_regret", "bayes_arm")
PER_DRAW = ("value_optimal", "value_bayes", "regret_bayes", "value_arm", "share_best")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_bits(got, want) -> bool:
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


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


# ------------------------------------------------------------------ pgb_predict_arms
def _arms_call(hip, oracle, pool, table, block, cols, arms, picks, pad=3, change=None, f=None):
    """The entry point itself on the rows ``block`` with a leading dimension of ``p + pad`` -> ``(rc, out (A, n_picks, K,
    nb), list lengths, the guards behind both)``.  ``f``: what is handed in as ``f_dev`` (default: the oracle's
    ``pgb_predict``, whose bits the device's has).  ``change``: arguments replaced after everything is laid out."""
    mem, lib = hip.mem, hip.lib
    nb, p = block.shape
    K = int(pool.n_outputs)
    table = np.ascontiguousarray(table, np.int32)
    cols, picks = np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(picks, np.int32)
    arms = np.ascontiguousarray(np.asarray(arms, np.float64).reshape(-1, cols.size))
    A = arms.shape[0]
    wide = np.full((nb, p + pad), POISON)
    wide[:, :p] = block
    xd = mem.from_host(wide)
    if f is None:
        f = permimp.predict(oracle, pool, table[picks], block)
    fd = mem.from_host(np.ascontiguousarray(f, np.float64).ravel())
    cells = A * picks.size * K * nb
    od = mem.from_host(np.full(cells + 64, GUARD))
    lens = np.full(picks.size + 4, INT_GUARD, np.int32)
    carr = pool.as_c()
    a = dict(fidx=table.ctypes.data, n_forests=table.shape[0], m=table.shape[1], X_dev=mem.ptr(xd), nb=nb, p=p, ldx=p + pad,
             cols=cols.ctypes.data, s=cols.size, arms=arms.ctypes.data, A=A, picks=picks.ctypes.data, n_picks=picks.size,
             f=mem.ptr(fd), out=mem.ptr(od), lens=lens.ctypes.data)
    a.update(change or {})
    rc = lib.arms_entry_points()[0](C.byref(carr), a["fidx"], a["n_forests"], a["m"], a["X_dev"], a["nb"], a["p"], a["ldx"],
                                    a["cols"], a["s"], a["arms"], a["A"], a["picks"], a["n_picks"], a["f"], a["out"], a["lens"],
                                    mem.stream_ptr)
    got = mem.to_host(od)
    return rc, got[:cells].reshape(A, picks.size, K, nb), lens[:picks.size], (got[cells:], lens[picks.size:])


def _check_arms(hip, oracle, pool, table, block, cols, arms, picks, pad=3, f=None):
    """Against the host reference, bit for bit; the guards untouched.  -> ``(out, list lengths)``."""
    rc, got, lens, (g_out, g_lens) = _arms_call(hip, oracle, pool, table, block, cols, arms, picks, pad, f=f)
    hip.lib.check(rc, "pgb_predict_arms")
    want, wl = host.reference_block(oracle, pool, table, block, list(cols), arms, picks, f=f)
    assert np.all(g_out == GUARD) and np.all(g_lens == INT_GUARD)
    assert np.array_equal(lens, wl), (lens, wl)
    assert same_bits(got, want), (int((bits(got) != bits(want)).sum()), got.size)
    return got, lens


@pytest.fixture(scope="module")
def lengths():
    """Union lists of 1, 3, 4, 8, 9 and 0 trees for the single columns 0 .. 5: both sides of PRED_WALKS and of its
    prefetch; K = 1."""
    rng = np.random.default_rng(101)
    pool = permimp.lengths_pool(rng, 1)
    table = _forests(rng, 12, 12, 3)                                   # the same trees in three orders
    return pool, table, _rows(rng, 130, 6)


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 130])
def test_row_counts_and_list_lengths(hip, oracle, lengths, nb):
    pool, table, X = lengths
    arms = [0.3, np.nan, np.inf, -np.inf, -0.4]
    for c in range(6):
        out, lens = _check_arms(hip, oracle, pool, table, X[:nb], [c], arms, [0, 2, 0])         # a repeated pick
        assert lens.tolist() == [(permimp.LENGTHS + (0,))[c]] * 3 and np.array_equal(bits(out[:, 0]), bits(out[:, 2]))
        if c == 5:                                                     # the unused column: f itself under every arm
            f = permimp.predict(oracle, pool, table[[0, 2, 0]], X[:nb])
            assert np.array_equal(bits(out), bits(np.broadcast_to(f + 0.0, out.shape)))
        elif nb >= 63:
            assert not np.array_equal(out[2], out[3])                    # +inf goes right where -inf goes left
    out, lens = _check_arms(hip, oracle, pool, table, X[:nb], [5, 0, 2], [[1.0, -1.0, 0.5], [np.nan, 0.2, np.nan]], [1])
    assert lens.tolist() == [4]                                        # the union of 0, 1 and 4 nested trees


def test_clean_tiles_take_the_fixed_length_walk_under_a_clean_arm_only(hip, oracle, lengths):
    pool, table, X = lengths
    clean = np.nan_to_num(X, nan=0.25)
    out, _ = _check_arms(hip, oracle, pool, table, clean, [4, 3], [[0.1, -0.3], [np.nan, 0.5], [1.0, np.nan], [-2.0, 2.0]], [1, 0])
    assert np.all(np.isfinite(out)) and np.count_nonzero(out[0] != out[3]) > 0
    mixed = clean.copy()
    mixed[64:, 1] = np.where(np.arange(66) % 5 == 0, np.nan, mixed[64:, 1])   # the first tile clean, the others not
    _check_arms(hip, oracle, pool, table, mixed, [4, 3], [[0.1, -0.3], [np.nan, 0.5]], [2])


@pytest.mark.parametrize("p,K,s,A,D", [(3, 1, 2, 1, 1), (3, 3, 3, 64, 3), (LDS_MAXP, 1, 16, 2, 5), (LDS_MAXP + 1, 1, 16, 3, 3),
                                       (LDS_MAXP + 1, 3, 1, 2, 1), (20, 3, 2, 3, 5)])
def test_widths_outputs_columns_arms_and_linear_leaves_on_an_arm_column(hip, oracle, p, K, s, A, D):
    """p = 126 is the last width staged in LDS, p = 127 the first read from global memory; the leaves regress on columns
    among ``cols``; ldx = p + 3 with poisoned padding."""
    rng = np.random.default_rng(200 + p + K + s)
    pool = ice_host.random_pool(rng, 14, p, K=K, depth=5, linear=[0, p - 1])
    table = _forests(rng, 14, 6, max(D, 2))
    X = _rows(rng, 70, p)
    cols = ([p - 1, 0] + [int(c) for c in rng.permutation(np.arange(1, p - 1))])[:s]
    arms = rng.normal(size=(A, s))
    if A >= 2:
        arms[1, 0] = np.nan
    if A >= 3 and s >= 3:                                               # (the infinities on a column no leaf regresses on)
        arms[2, 2], arms[0, s - 1] = np.inf, -np.inf
    out, lens = _check_arms(hip, oracle, pool, table, X, cols, arms, list(range(D)))
    assert out.shape == (A, D, K, 70) and lens.max() > 0 and not np.any(np.abs(out) == POISON)


@pytest.mark.parametrize("p,K", [(5, 1), (5, 3), (LDS_MAXP + 1, 1)])
def test_continuous_one_hot_and_subset_columns_among_the_arm_columns(hip, oracle, p, K):
    """The instances without the continuous rule, staged and not; a code on a subset column is read as pgb_predict reads
    it in a row (a code outside the trained ones and a NaN included)."""
    rng = np.random.default_rng(300 + p + K)
    rules = [0, ONEHOT, 0, SUBSET, 0] + [0] * (p - 5)
    pool = ice_host.random_pool(rng, 16, p, K=K, depth=5, rules=rules, linear=[2, 4], split_cols=[0, 1, 2, 3, 4])
    table = _forests(rng, 16, 8, 2)
    X = _rows(rng, 130, p, rules)
    arms = [[0.0, 0.0, -0.3], [1.0, 7.0, 0.8], [3.0, 2.0, np.nan], [2.0, np.nan, 0.1], [np.nan, 5.0, np.inf], [5.0, 11.0, -1.0]]
    out, _ = _check_arms(hip, oracle, pool, table, X[64:], [1, 3, 0], arms, [0, 1])
    assert len({out[a].tobytes() for a in range(6)}) >= 4


def test_an_arm_equal_to_the_rows_returns_f_and_minus_zero_becomes_plus_zero(hip, oracle, lengths):
    pool, table, X = lengths
    same = np.tile(np.nan_to_num(X[:1], nan=0.5), (70, 1))
    f = permimp.predict(oracle, pool, table[[0, 1]], same)
    out, _ = _check_arms(hip, oracle, pool, table, same, [4, 2], [same[0, [4, 2]], [0.0, 9.0]], [0, 1])
    assert np.array_equal(bits(out[0]), bits(f)) and not np.array_equal(out[1], f)
    out, _ = _check_arms(hip, oracle, pool, table, same, [4, 2], [same[0, [4, 2]]], [0, 1], f=np.full(f.shape, -0.0))
    assert np.all(bits(out) == 0)
    out, _ = _check_arms(hip, oracle, pool, table, X, [5], [3.0], [0, 1], f=np.full((2, 1, 130), -0.0))   # an empty list
    assert np.all(bits(out) == 0)


def test_every_refusal_of_predict_arms_leaves_the_outputs_untouched(hip, oracle, lengths):
    pool, table, X = lengths
    cols, arms = [2, 0, 4], np.arange(9.0).reshape(3, 3)               # (3 arms x 2^22 picks x 2^37 rows: above 2^60 cells)
    i32 = lambda *v: np.array(v, np.int32)  # noqa: E731
    bad_cols, twice, bad_picks, many = i32(0, 9, 1), i32(2, 0, 2), i32(0, 3), np.zeros(1 << 22, np.int32)
    wide_cols, many_arms = np.arange(17, dtype=np.int32), np.zeros((65, 3))
    cases = [
        (dict(X_dev=None), "X_dev is null"), (dict(cols=None), "cols_host is null"), (dict(arms=None), "arms_host is null"),
        (dict(picks=None), "picks_host is null"), (dict(fidx=None), "forest_tree_idx is null"), (dict(f=None), "f_dev is null"),
        (dict(out=None), "out_dev is null"),
        (dict(m=0), "n_forests, m and p must be >= 1"), (dict(n_forests=0), "n_forests, m and p must be >= 1"),
        (dict(p=0), "n_forests, m and p must be >= 1"), (dict(nb=0), "nb must be >= 1"), (dict(s=0), "s must be >= 1"),
        (dict(A=0), "A must be >= 1"), (dict(n_picks=0), "n_picks must be >= 1"), (dict(ldx=5), "ldx must be >= p"),
        (dict(cols=wide_cols.ctypes.data, s=17), "s must be <= PGB_ARMS_MAX_COLS = 16"),
        (dict(arms=many_arms.ctypes.data, A=65), "A must be <= PGB_ARMS_MAX = 64"),
        (dict(cols=bad_cols.ctypes.data), "cols_host[1] = 9 is outside [0, p = 6)"),
        (dict(cols=twice.ctypes.data), "repeats cols_host"),
        (dict(picks=bad_picks.ctypes.data), "picks_host[1] = 3 is outside [0, n_forests = 3)"),
        (dict(nb=(1 << 37) - 64, picks=many.ctypes.data, n_picks=1 << 22), "overflows a 64-bit size"),
    ]
    for change, msg in cases:
        rc, got, lens, (g_out, g_lens) = _arms_call(hip, oracle, pool, table, X, cols, arms, [0, 1], change=change)
        text = hip.lib.lib.pgb_last_error().decode()
        assert rc == E_INVALID and msg in text and text.startswith("pgb_predict_arms: "), (change, rc, text)
        assert np.all(got == GUARD) and np.all(g_out == GUARD) and np.all(lens == INT_GUARD) and np.all(g_lens == INT_GUARD), change
    table_bad = table.copy()                                           # a malformed history: pgb_predict's checks
    table_bad[1, 3] = 12
    rc, got, lens, _ = _arms_call(hip, oracle, pool, table, X, cols, arms, [0, 1], change=dict(fidx=table_bad.ctypes.data))
    assert rc == E_INVALID and "forest_tree_idx entry outside" in hip.lib.lib.pgb_last_error().decode()
    assert np.all(got == GUARD) and np.all(lens == INT_GUARD)


# ------------------------------------------------------------------ pgb_arm_decide and its finish
def _utilities(rng, A, D, K, n):
    """Predictions ``(A, D, K, n)`` with many ties, two identical arms, single and all-NaN (d, i) and infinities."""
    f = rng.integers(-3, 4, (A, D, K, n)) / 2.0 + rng.normal(0, 0.01, (A, D, K, n)) * (rng.random((A, D, K, n)) < 0.5)
    if A >= 3:
        f[A - 1] = f[1]
    f[:, 0, :, n // 3] = np.nan
    f[0, D - 1, :, n // 2] = np.nan
    f[A - 1, 0, :, n - 1], f[0, 0, :, n - 1], f[0, D - 1, :, 0] = np.inf, np.inf, -np.inf
    return f


def _decide(hip, f, k, w, g, G, policy=None, off=None, cost=None, sign=1.0, transform="identity", blocks=None, change=None,
            finish_change=None, do_finish=True):
    """``pgb_arm_decide`` per block of rows on output ``k`` of ``f`` ``(A, D, K, n)`` (handed over through ``lda`` /
    ``ldd``, without a copy) and ``pgb_arm_decide_finish`` -> a dict in the layout of ``_arms_host.decide`` plus the return
    codes and the guards.  ``change`` / ``finish_change``: arguments replaced after everything is laid out."""
    mem, lib = hip.mem, hip.lib
    _, decide, finish, query = lib.arms_entry_points()
    A, D, K, n = f.shape
    code = host.TRANSFORMS[transform]
    n_ws = host.ws_doubles(D, G, A)
    assert int(query(D, G, A)) == 8 * n_ws
    ws = mem.from_host(np.full(n_ws + 64, GUARD))
    cost_h = None if cost is None else np.ascontiguousarray(cost, np.float64)
    res = {"nbest": np.empty((A, n), np.int32), "mean": np.empty((A, n)), "regret": np.empty((A, n)), "bayes": np.empty(n, np.int32),
           "rc": [], "guards_ok": True}
    for r0, r1 in (blocks or [(0, n)]):
        nb = r1 - r0
        fd = mem.from_host(np.ascontiguousarray(f[..., r0:r1]).ravel())
        dev = lambda v, t: None if v is None else mem.from_host(np.ascontiguousarray(v[r0:r1], t))  # noqa: E731
        wd, gd, pd, offd = dev(w, np.float64), dev(g, np.int32), dev(policy, np.int32), dev(off, np.float64)
        nd, bd = mem.from_host(np.full(A * nb + 64, INT_GUARD, np.int32)), mem.from_host(np.full(nb + 64, INT_GUARD, np.int32))
        md, rd = mem.from_host(np.full(A * nb + 64, GUARD)), mem.from_host(np.full(A * nb + 64, GUARD))
        ptr = lambda b: None if b is None else mem.ptr(b)  # noqa: E731
        a = dict(f=mem.ptr(fd[k * nb:]), lda=D * K * nb, ldd=K * nb, D=D, A=A, nb=nb, w=ptr(wd), g=ptr(gd), policy=ptr(pd),
                 off=ptr(offd), cost=None if cost_h is None else cost_h.ctypes.data, sign=sign, transform=code, G=G, first_row=r0,
                 init=int(r0 == 0), ws=mem.ptr(ws), nbest=mem.ptr(nd), mean=mem.ptr(md), regret=mem.ptr(rd), bayes=mem.ptr(bd))
        a.update(change or {})
        res["rc"].append(decide(a["f"], a["lda"], a["ldd"], a["D"], a["A"], a["nb"], a["w"], a["g"], a["policy"], a["off"], a["cost"],
                                a["sign"], a["transform"], a["G"], a["first_row"], a["init"], a["ws"], a["nbest"], a["mean"],
                                a["regret"], a["bayes"], mem.stream_ptr))
        got = [mem.to_host(b) for b in (nd, md, rd, bd)]
        res["guards_ok"] &= bool(np.all(got[0][A * nb:] == INT_GUARD) and np.all(got[1][A * nb:] == GUARD)
                                 and np.all(got[2][A * nb:] == GUARD) and np.all(got[3][nb:] == INT_GUARD))
        res["nbest"][:, r0:r1], res["mean"][:, r0:r1] = got[0][:A * nb].reshape(A, nb), got[1][:A * nb].reshape(A, nb)
        res["regret"][:, r0:r1], res["bayes"][r0:r1] = got[2][:A * nb].reshape(A, nb), got[3][:nb]
    n_out = (4 + 2 * A) * D * G
    od, wod = mem.from_host(np.full(n_out + 64, GUARD)), mem.from_host(np.full(G + 64, GUARD))
    counts = (C.c_int64 * 3)(INT_GUARD, INT_GUARD, INT_GUARD)
    if do_finish:
        a = dict(ws=mem.ptr(ws), D=D, G=G, A=A, has_policy=int(policy is not None), out=mem.ptr(od), w_out=mem.ptr(wod), counts=counts)
        a.update(finish_change or {})
        res["rc_finish"] = finish(a["ws"], a["D"], a["G"], a["A"], a["has_policy"], a["out"], a["w_out"], a["counts"], mem.stream_ptr)
    out, W, wsh = mem.to_host(od), mem.to_host(wod), mem.to_host(ws)
    res["guards_ok"] &= bool(np.all(out[n_out:] == GUARD) and np.all(W[G:] == GUARD) and np.all(wsh[n_ws:] == GUARD))
    res.update(out=out[:n_out].reshape(4 + 2 * A, D, G), W=W[:G], counts=np.array(list(counts), np.int64), ws=wsh[:n_ws])
    return res


def _same_decision(got, want, ws=True):
    for key in ("nbest", "bayes", "counts"):
        assert np.array_equal(got[key], want[key]), (key, got[key], want[key])
    for key in ("mean", "regret", "out", "W") + (("ws",) if ws else ()):
        assert same_bits(got[key], want[key]), (key, int((bits(got[key]) != bits(want[key])).sum()))


def _inputs(rng, n, G, A, contiguous=False):
    w = rng.uniform(0.5, 2.0, n)
    w[rng.random(n) < 0.1] = 0.0
    g = np.sort(rng.integers(0, G, n)) if contiguous else rng.integers(0, G, n)
    return w, g.astype(np.int32), rng.integers(0, A, n).astype(np.int32), rng.normal(0, 0.3, n), rng.integers(-4, 5, A) / 8.0


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 130])
def test_decide_row_counts(hip, nb):
    rng = np.random.default_rng(400 + nb)
    A, D, K, G = 3, 3, 1, 3
    f = _utilities(rng, A, D, K, nb) if nb > 1 else rng.normal(size=(A, D, K, 1))
    w, g, pi, off, cost = _inputs(rng, nb, G, A)
    got = _decide(hip, f, 0, w, g, G, pi, off, cost)
    assert got["rc"] == [0] and got["rc_finish"] == 0 and got["guards_ok"]
    _same_decision(got, host.decide(f[:, :, 0], w, g, G, pi, off, cost))


@pytest.mark.parametrize("A,D,K,G,transform,sign", [(1, 1, 1, 1, "identity", 1.0), (2, 1, 1, 4096, "identity", -1.0),
                                                    (3, 5, 3, 3, "logistic", 1.0), (64, 3, 1, 3, "exp", 1.0),
                                                    (2, 3, 3, 1, "probit", -1.0), (5, 5, 1, 4, "exp", -1.0)])
def test_decide_arms_draws_outputs_groups_transforms_and_signs(hip, A, D, K, G, transform, sign):
    rng = np.random.default_rng(500 + A + D + K + G)
    n = 4200 if G == 4096 else 130
    f = _utilities(rng, A, D, K, n)
    if transform == "exp":
        f[0, 0, :, 5], f[A - 1, 0, :, 5] = 800.0, 900.0                  # exp overflows on both: +inf == +inf
    w, g, pi, off, cost = _inputs(rng, n, G, A, contiguous=G == 4096)
    k = K - 1
    for policy, offset, costs in ((pi, off, cost), (None, None, None)):
        got = _decide(hip, f, k, w, g, G, policy, offset, costs, sign, transform)
        assert got["rc"] == [0] and got["rc_finish"] == 0 and got["guards_ok"]
        want = host.decide(f[:, :, k], w, g, G, policy, offset, costs, sign, transform)
        _same_decision(got, want)
        assert got["counts"][1:].tolist() == [0, 0]
        if transform != "probit":                                        # (pgb_lphi_t maps a NaN to a number)
            assert got["counts"][0] > 0
    if A >= 3:
        assert np.all(got["nbest"][A - 1][np.isfinite(f[:, :, k]).all(axis=(0, 1))] == 0)   # the copy of arm 1 never wins


def test_a_two_block_carry_of_the_workspace(hip):
    rng = np.random.default_rng(600)
    A, D, K, G, n = 4, 3, 3, 3, 130
    f = _utilities(rng, A, D, K, n)
    w, g, pi, off, cost = _inputs(rng, n, G, A)
    whole = _decide(hip, f, 1, w, g, G, pi, off, cost, transform="logistic")
    two = _decide(hip, f, 1, w, g, G, pi, off, cost, transform="logistic", blocks=[(0, 64), (64, 130)])   # first_row = 64, init = 0
    assert two["rc"] == [0, 0] and two["rc_finish"] == 0 and two["guards_ok"] and whole["guards_ok"]
    _same_decision(two, whole)
    _same_decision(two, host.decide(f[:, :, 1], w, g, G, pi, off, cost, transform="logistic", chunk=64))


def test_bad_groups_and_bad_policies_are_counted_and_the_finish_refuses(hip):
    rng = np.random.default_rng(700)
    A, D, K, G, n = 3, 3, 1, 2, 140
    f = rng.normal(size=(A, D, K, n))
    w, g, pi, _, _ = _inputs(rng, n, G, A)
    g[[3, 64, 70, 139]], pi[[5, 70, 100]] = [-1, G, 7, -5], [A, -1, 99]
    got = _decide(hip, f, 0, w, g, G, pi)
    text = hip.lib.lib.pgb_last_error().decode()
    assert got["rc"] == [0] and got["rc_finish"] == E_INVALID and "4 rows have a group outside [0, 2)" in text and got["guards_ok"]
    _same_decision(got, host.decide(f[:, :, 0], w, g, G, pi))
    assert got["counts"].tolist() == [0, 4, 3]
    g = np.clip(g, 0, G - 1)
    got = _decide(hip, f, 0, w, g, G, pi)
    assert got["rc_finish"] == E_INVALID and "3 rows have a policy outside [0, 3)" in hip.lib.lib.pgb_last_error().decode()
    _same_decision(got, host.decide(f[:, :, 0], w, g, G, pi))


def test_every_refusal_of_decide_and_of_the_finish_leaves_the_outputs_and_the_workspace_untouched(hip):
    rng = np.random.default_rng(800)
    A, D, K, G, n = 3, 2, 2, 2, 70
    f = rng.normal(size=(A, D, K, n))
    w, g, pi, off, cost = _inputs(rng, n, G, A)
    bad_cost = np.array([0.0, np.inf, 1.0])
    cases = [
        (dict(f=None), "f_dev is null"), (dict(w=None), "w_dev is null"), (dict(g=None), "g_dev is null"),
        (dict(ws=None), "ws_dev is null"), (dict(nbest=None), "nbest_dev is null"), (dict(mean=None), "mean_dev is null"),
        (dict(regret=None), "regret_dev is null"), (dict(bayes=None), "bayes_dev is null"),
        (dict(D=0), "D must be >= 1"), (dict(A=0), "A must be >= 1"), (dict(A=65), "A must be <= PGB_ARMS_MAX = 64"),
        (dict(nb=0), "nb must be >= 1"), (dict(G=0), "G must be in [1, PGB_ROWRED_MAX_GROUPS = 4096]"),
        (dict(G=4097), "G must be in [1, PGB_ROWRED_MAX_GROUPS = 4096]"), (dict(ldd=n - 1), "ldd must be >= nb"),
        (dict(lda=K * n + n - 1), "lda must be >= (D - 1) ldd + nb"),
        (dict(first_row=-64), "first_row must be a multiple of 64"), (dict(first_row=32), "first_row must be a multiple of 64"),
        (dict(transform=4), "unknown transform"), (dict(transform=-1), "unknown transform"),
        (dict(sign=0.5), "sign must be +1.0 or -1.0"), (dict(sign=float("nan")), "sign must be +1.0 or -1.0"),
        (dict(cost=bad_cost.ctypes.data), "cost_host[1] is not finite"),
    ]
    for change, msg in cases:
        got = _decide(hip, f, 1, w, g, G, pi, off, cost, change=change, do_finish=False)
        text = hip.lib.lib.pgb_last_error().decode()
        assert got["rc"] == [E_INVALID] and msg in text and text.startswith("pgb_arm_decide: "), (change, got["rc"], text)
        assert got["guards_ok"] and np.all(got["ws"] == GUARD) and np.all(got["nbest"] == INT_GUARD) and np.all(got["bayes"] == INT_GUARD)
        assert np.all(got["mean"] == GUARD) and np.all(got["regret"] == GUARD), change
    cases = [(dict(ws=None), "ws_dev is null"), (dict(out=None), "out_dev is null"), (dict(w_out=None), "w_out_dev is null"),
             (dict(counts=None), "counts_out is null"), (dict(D=0), "D must be >= 1"), (dict(A=65), "A must be <= PGB_ARMS_MAX"),
             (dict(G=4097), "G must be in [1, PGB_ROWRED_MAX_GROUPS = 4096]"), (dict(has_policy=2), "has_policy must be 0 or 1")]
    for change, msg in cases:
        got = _decide(hip, f, 1, w, g, G, pi, off, cost, finish_change=change)
        text = hip.lib.lib.pgb_last_error().decode()
        assert got["rc_finish"] == E_INVALID and msg in text and text.startswith("pgb_arm_decide_finish: "), (change, text)
        assert got["guards_ok"] and np.all(got["out"] == GUARD) and np.all(got["W"] == GUARD), change
        assert got["counts"].tolist() == [INT_GUARD] * 3
    assert [int(hip.lib.arms_entry_points()[3](*a)) for a in ((0, 1, 1), (1, 0, 1), (1, 4097, 1), (1, 1, 0), (1, 1, 65))] == [0] * 5


# ------------------------------------------------------------------ end to end
N_FIT, M_FIT = 300, 20


@pytest.fixture(scope="module")
def fit(hip):
    """Two chains of 12 draws behind one sampler; column 1 is the treatment (three levels) whose effect depends on
    column 0; rows with missing values in the treatment and in a noise column."""
    rng = np.random.default_rng(61)
    X = rng.uniform(-1, 1, size=(N_FIT, 6))
    X[:, 1] = rng.integers(0, 3, N_FIT)
    y = X[:, 1] * X[:, 0] + 0.5 * X[:, 2] + rng.normal(0, 0.2, N_FIT)
    op = BARTOp(X, y, m=M_FIT)
    attach_history(op, [sample_chain(op, 30, 12, random_seed=4, chain=c, backend=hip, keep_draws=False) for c in (0, 1)])
    Xm = X.copy()
    Xm[5::17, 1], Xm[3::29, 4] = np.nan, np.nan
    kw = dict(cols=[1], arms=[0.0, 1.0, 2.0], cost=[0.0, 0.05, 0.1], weights=rng.uniform(0.5, 2.0, N_FIT),
              groups=np.where(X[:, 0] > 0, "right", "left"), policy=(X[:, 0] > 0).astype(np.int64) * 2)
    return Xm, kw, _get_posterior_sampler(op, backend=hip)


def _history(s):
    pool, table = s.pooled_history() if hasattr(s, "pooled_history") else (s.pool, s.forest_idx)
    return (pool.decoded() if hasattr(pool, "decoded") else pool), np.asarray(table)


def _same_results(got, want):
    for key in PER_ROW + PER_DRAW + ("value_policy", "group_weight", "n_list_trees"):
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    for key in PER_DRAW + ("value_policy",):
        for tail in ("_mean", "_sd", "_hdi"):
            assert np.array_equal(bits(got[key + tail]), bits(want[key + tail])), key + tail
    assert got["n_nonfinite"] == want["n_nonfinite"] and got["group_labels"].tolist() == want["group_labels"].tolist()


def test_optimal_arm_under_blocking_and_against_the_host_backend(hip, oracle, fit, monkeypatch):
    X, kw, s = fit
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    whole = optimal_arm(s, X, **kw)
    assert whole["n_draws"] == 24 and whole["n_nonfinite"] == 0 and whole["group_labels"].tolist() == ["left", "right"]
    assert 0 < whole["n_list_trees"].min() and whole["n_list_trees"].max() <= M_FIT
    draws = [1, 8, 13, 22]
    few = optimal_arm(s, X, draws=draws, **kw)
    for key in ("value_optimal", "value_arm", "share_best", "value_policy"):   # (bayes_arm depends on the draws asked for)
        assert np.array_equal(bits(few[key]), bits(whole[key][draws])), key
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")                  # blocks of 64 rows
    job = dec.ArmsJob(s, X, kw["cols"], kw["arms"], draws, None)
    job.take_decision(0, None, None, kw["cost"], True, kw["weights"], kw["groups"], kw["policy"], 0.94)
    assert job.decide_row_bytes() * 128 > 65536 - job.ws_bytes
    _same_results(optimal_arm(s, X, draws=draws, **kw), few)
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    pool, table = _history(s)
    on_host = PosteriorSampler(pool, np.ascontiguousarray(table, np.int32), M_FIT, 1, backend=host.HostBackend(oracle, pool))
    _same_results(optimal_arm(on_host, X, draws=draws, **kw), few)
    # the treatment helps on the right and hurts on the left: the rule that knows it beats every single arm
    mean = whole["value_arm_mean"]
    print("value_arm_mean:", np.array2string(mean, precision=3), "value_bayes_mean:", whole["value_bayes_mean"])
    assert mean[0].argmax() == 0 and mean[1].argmax() == 2 and np.all(whole["value_policy_mean"] >= mean.max(axis=1) - 0.05)


def test_arm_predictions_against_plain_predictions_of_copies(hip, fit, monkeypatch):
    """``arm_predictions`` against ``Job.predict`` on copies of ``X`` within ``4 (m + 1) 2^-53 S``: ``S`` is the largest,
    over the draws, of the sum over a draw's trees of the tree's largest ``|leaf|`` (computed from the pool below).

    Both routes add the same per-tree terms -- the walk of a tree at a row is one text -- in different orders.  With
    ``u = 2^-53`` and to first order: the plain prediction of the copy is a recursive sum of ``m`` terms, off by at most
    ``(m - 1) u S``; the fused value is ``fl(f + fl(A_a - A_self))``, where ``f`` (``m`` terms), ``A_a`` and ``A_self``
    (at most ``m`` terms each) are recursive sums off by at most ``(m - 1) u S`` each, the rounding of the difference is
    at most ``u |A_a - A_self| <= 2 u S`` and that of the last addition at most ``u S``.  Together
    ``(4 (m - 1) + 3) u S < 4 (m + 1) u S``.  The reference alone decides it; nothing is tuned on the device's output."""
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    X, kw, s = fit
    pool, table = _history(s)
    leaf = np.asarray(pool.var) < 0
    top = np.abs(np.asarray(pool.value, np.float64).reshape(-1, 1)).max(axis=1) * leaf
    per_tree = np.array([top[pool.node_off[t]:pool.node_off[t + 1]].max() for t in range(pool.n_trees)])
    S = float(per_tree[table].sum(axis=1).max())
    bound = 4 * (M_FIT + 1) * 2.0 ** -53 * S
    cols, arms = [1, 0], [[0.0, -0.5], [2.0, 0.5], [np.nan, 0.0]]
    got = arm_predictions(s, X, cols, arms)
    assert got.shape == (3, 24, N_FIT)
    job = dec.ArmsJob(s, X, cols, arms, None, None)
    job.take_history()
    worst = 0.0
    for a, arm in enumerate(arms):
        Xa = host.arm_copy(X, cols, arm)
        want = hip.mem.to_host(job.predict(hip, hip.mem.from_host(Xa), N_FIT)).reshape(24, N_FIT)
        err = float(np.abs(got[a] - want).max())
        print(f"arm {a}: max |arm_predictions - plain prediction of the copy| = {err:.3e}, bound {bound:.3e}")
        worst = max(worst, err)
        assert err <= bound, (a, err, bound)
    assert S > 0.0 and not np.array_equal(got[0], got[1])
    print(f"max |arm_predictions - plain| / bound = {worst / bound:.3f}")
    assert optimal_arm(s, X, cols, arms)["n_nonfinite"] == 0
