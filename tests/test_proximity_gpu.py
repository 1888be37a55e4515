"""Posterior proximity on the MI355X: ``k_leaf_codes``, ``k_prox_count`` and ``k_prox_topk`` through
``pgb_predict_leaf_codes``, ``pgb_prox_count`` and ``pgb_prox_topk`` against the independent NumPy recount of
``tests/_proximity_host.py`` -- on hand-built pools at every tile regime, row path, split rule and walk, on synthetic code
matrices at the edges of the count's query tile and row tile, in one block and in successive blocks and chunks -- the
refusals of the entry points, and the public calls of ``pymc_bart_amd.proximity`` on short real chains.

Every comparison is an exact integer equality."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import _predict_exact as px
import _proximity_host as host
from pymc_bart_amd import BARTOp, CategoricalLikelihood, _abi, _stored, leaf_ids, nearest_rows, proximity
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays
from pymc_bart_amd.utils import _get_posterior_sampler

prox_mod = sys.modules["pymc_bart_amd.proximity"]

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADX = 7.0e77            # what the columns of X beyond p hold: no code may depend on it
GUARD = 0x5A5A5A5A       # what every output buffer holds before a call, and keeps wherever nothing is written
QT, BT = 16, 256         # k_prox_count's query tile and row tile (PROX_QT, PROX_BT)


def _define(header: str, name: str) -> int:
    text = open(os.path.join(ROOT, "pymc_bart_amd", "csrc", header)).read()
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


LDS_MAXP = _define("pgb_pred_walk.h", "PRED_LDS_MAXP")
assert (_define("k_proximity.h", "PROX_QT"), _define("k_proximity.h", "PROX_BT")) == (QT, BT)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)


def up32(mem, a):
    """A uint32 host array on the device (as int32: the same bits)."""
    return mem.from_host(np.ascontiguousarray(a, np.uint32).view(np.int32))


def down32(mem, t) -> np.ndarray:
    return mem.to_host(t).view(np.uint32)


# ------------------------------------------------------------------ the three entry points on device buffers
def dev_codes(hip, pool, fidx, X, excluded=(), pad_x=0, pad_c=0) -> np.ndarray:
    """``pgb_predict_leaf_codes`` with ``ldx = p + pad_x`` and ``ldc = n + pad_c`` -> the words ``(W, n)``."""
    mem, lib = hip.mem, hip.lib
    entry = lib.proximity_entry_points()[0]
    X = np.asarray(X, np.float64)
    fidx = np.ascontiguousarray(fidx, np.int32)
    (D, m), (n, p) = fidx.shape, X.shape
    Xp = np.full((n, p + pad_x), PADX)
    Xp[:, :p] = X
    W, ldc = -(-D * m // 4), n + pad_c
    xd, cd = mem.from_host(Xp), up32(mem, np.full(W * ldc + 8, GUARD))
    excl = np.ascontiguousarray(excluded, np.int32)
    carr = pool.as_c()
    rc = entry(C.byref(carr), fidx.ctypes.data, D, m, mem.ptr(xd), n, p, p + pad_x, excl.ctypes.data if excl.size else None,
               int(excl.size), mem.ptr(cd), ldc, mem.stream_ptr)
    lib.check(rc, "pgb_predict_leaf_codes")
    got = down32(mem, cd)
    assert np.all(got[-8:] == GUARD)
    got = got[:-8].reshape(W, ldc)
    assert np.all(got[:, n:] == GUARD)                                  # nothing written beyond the rows
    return got[:, :n].copy()


def check_codes(hip, pool, fidx, X, excluded=(), what=None, **pads):
    want = host.stop_nodes(pool, fidx, X, excluded)
    got = dev_codes(hip, pool, fidx, X, excluded, **pads)
    D, m = np.asarray(fidx).shape
    assert np.array_equal(got, host.pack(want.reshape(D * m, -1))), what
    return want, got


def dev_count(hip, cq, cr, pads=(0, 0, 0), dist=None) -> np.ndarray:
    """``pgb_prox_count`` of the words ``cq (W, q)`` and ``cr (W, nb)`` with ``ldq``, ``ldr`` and ``ldo`` padded;
    ``dist``: the distances to continue from (``None``: init) -> ``uint32 (q, nb)``."""
    mem, lib = hip.mem, hip.lib
    count = lib.proximity_entry_points()[1]
    (W, q), nb = cq.shape, cr.shape[1]
    ldq, ldr, ldo = q + pads[0], nb + pads[1], nb + pads[2]
    cqp, crp = np.full((W, ldq), GUARD, np.uint32), np.full((W, ldr), GUARD, np.uint32)
    cqp[:, :q], crp[:, :nb] = cq, cr
    out = np.full(q * ldo + 8, GUARD, np.uint32)
    if dist is not None:
        out[:q * ldo].reshape(q, ldo)[:, :nb] = dist
    qd, rd, dd = up32(mem, cqp), up32(mem, crp), up32(mem, out)         # (held: a dropped buffer's memory is handed out again)
    rc = count(mem.ptr(qd), ldq, q, mem.ptr(rd), ldr, nb, W, mem.ptr(dd), ldo, int(dist is None), mem.stream_ptr)
    lib.check(rc, "pgb_prox_count")
    got = down32(mem, dd)
    assert np.all(got[-8:] == GUARD)
    got = got[:-8].reshape(q, ldo)
    assert np.all(got[:, nb:] == GUARD)
    return got[:, :nb].copy()


def dev_topk(hip, dist, k, cuts=None, self_row0=-1, pad=0) -> np.ndarray:
    """``pgb_prox_topk`` of ``dist (q, n)``, block by block along ``cuts`` (``None``: one block) -> the workspace."""
    mem, lib = hip.mem, hip.lib
    _, _, topk, query = lib.proximity_entry_points()
    q, n = dist.shape
    words = int(host.lib().prox_topk_ws_words(q, k))
    assert query(q, k) == 8 * words
    ws = mem.from_host(np.full(words + 4, 0x7777777777777777, np.uint64).view(np.float64))
    cuts = (0, n) if cuts is None else cuts
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        blk = np.full((q, r1 - r0 + pad), GUARD, np.uint32)
        blk[:, :r1 - r0] = dist[:, r0:r1]
        bd = up32(mem, blk)
        rc = topk(mem.ptr(bd), r1 - r0 + pad, q, r1 - r0, r0, self_row0, k, mem.ptr(ws), int(r0 == 0), mem.stream_ptr)
        lib.check(rc, "pgb_prox_topk")
    got = mem.to_host(ws).view(np.uint64)
    assert np.all(got[-4:] == 0x7777777777777777)
    return got[:-4].copy()


# ------------------------------------------------------------------ pools
def grid_split(r, j):
    return r.integers(-8, 9) / 8.0


def mixed_pool(seed: int, p: int, K: int = 1):
    rng = np.random.default_rng(seed)
    cols = list(range(p))
    roots = [px.complete_tree(rng, K, 3, cols, grid_split), px.chain_tree(rng, K, 6, cols, grid_split, "left"),
             px.chain_tree(rng, K, 5, cols, grid_split, "right"), px.Leaf([0.5] * K)]
    roots += [px.dyadic_tree(rng, K, 5, cols, grid_split) for _ in range(6)]
    return px.build_pool(roots, K), rng


def grid_rows(rng, n: int, p: int) -> np.ndarray:
    return rng.integers(-10, 11, (n, p)) / 8.0                          # (rows hit split values exactly)


# ------------------------------------------------------------------ 1. codes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_codes_at_every_shape(n, hip):
    p = 5
    pool, rng = mixed_pool(n, p)
    X = grid_rows(rng, n, p)
    i = 0
    for D in (1, 3):
        for m in (1, 3, 4, 5, 9):                                       # T = 1 .. 27: words straddle draws, tails pad
            fidx = rng.integers(0, pool.n_trees, (D, m)).astype(np.int32)
            check_codes(hip, pool, fidx, X, what=(n, D, m), pad_x=(0, 3)[i % 2], pad_c=(0, 5)[(i // 2) % 2])
            i += 1


def test_codes_of_a_wide_matrix_take_the_global_row_path(hip):
    p = LDS_MAXP + 4
    pool, rng = mixed_pool(7, p)
    X = grid_rows(rng, 65, p)
    fidx = rng.integers(0, pool.n_trees, (3, 5)).astype(np.int32)
    check_codes(hip, pool, fidx, X, pad_x=2, pad_c=3)
    X[17, 9] = np.nan                                                   # ... and the stop rule on that path
    check_codes(hip, pool, fidx, X, excluded=(p - 1, 0))


def test_stumps_only_every_distance_is_zero(hip):
    pool = px.build_pool([px.Leaf([float(t)]) for t in range(5)], 1)
    rng = np.random.default_rng(0)
    X = rng.normal(size=(70, 3))
    X[3, 1] = np.nan
    fidx = rng.integers(0, 5, (3, 3)).astype(np.int32)
    want, words = check_codes(hip, pool, fidx, X)
    assert not want.any() and np.all(words[:2] == 0) and np.all(words[2] == 0xFFFFFF00)
    assert not dev_count(hip, words[:, :17].copy(), words).any()


def test_a_255_node_tree_puts_code_254_next_to_the_pad(hip):
    rng = np.random.default_rng(1)
    pool = px.build_pool([px.complete_tree(rng, 1, 7, [0, 1, 2], grid_split)], 1)
    assert pool.total_nodes == 255
    X = grid_rows(rng, 66, 3)
    X[0], X[65] = 9.0, -9.0                                             # always right: the last node; always left
    want, words = check_codes(hip, pool, np.zeros((1, 1), np.int32), X)
    assert want[0, 0, 0] == 254 and words[0, 0] == 0xFFFFFFFE and want[0, 0, 65] == 127
    want, words = check_codes(hip, pool, np.zeros((1, 5), np.int32), X)  # a full word of 254s, then 254 and three pads
    assert words[0, 0] == 0xFEFEFEFE and words[1, 0] == 0xFFFFFFFE
    dist = dev_count(hip, words[:, :2].copy(), words)
    assert np.array_equal(dist, host.distances(want.reshape(5, -1)[:, :2], want.reshape(5, -1)))


def test_depth_64_chains(hip):
    rng = np.random.default_rng(2)
    cols = [0, 1, 2, 3]
    pool = px.build_pool([px.chain_tree(rng, 1, 64, cols, grid_split, "left"), px.chain_tree(rng, 1, 64, cols, grid_split, "right"),
                          px.Leaf([1.0])], 1)
    assert px.tree_depth(pool, 0) == px.tree_depth(pool, 1) == 64
    X = grid_rows(rng, 67, 4)
    X[0], X[1] = -9.0, 9.0                                              # to the end of the left chain / of the right one
    fidx = np.array([[0, 1, 2, 1, 0], [1, 1, 0, 2, 0]], np.int32)
    want, _ = check_codes(hip, pool, fidx, X)
    assert want[0, 0, 0] == 127 and want[0, 1, 1] == 128                # (breadth-first: the deepest split's children)
    X[5, 2] = np.nan
    check_codes(hip, pool, fidx, X, excluded=(3,))


def test_general_and_fixed_length_trees_in_one_forest(hip):
    rng = np.random.default_rng(3)
    cols = [0, 1, 2]
    roots = [px.dyadic_tree(rng, 1, 5, cols, grid_split, grow=0.9) for _ in range(4)]
    pool = TreeArrays.concat([px.build_pool(roots[:2], 1), px.build_pool(roots[2:], 1, order="reversed")])
    X = grid_rows(rng, 130, 3)
    fidx = np.array([[0, 2, 1, 3], [2, 3, 2, 3], [0, 1, 0, 1], [3, 0, 0, 0]], np.int32)   # mixed, general, fixed, mixed words
    check_codes(hip, pool, fidx, X, pad_c=1)


@pytest.mark.parametrize("where", ["one lane", "every lane"])
def test_rows_with_a_missing_value_stop_at_the_split(where, hip):
    pool, rng = mixed_pool(4, 5)
    X = grid_rows(rng, 130, 5)
    if where == "one lane":
        X[69, 0] = X[69, 2] = np.nan                                    # one lane of the second wave; the first is clean
    else:
        X[:, 1] = np.nan
        X[::3, 4] = np.nan
    fidx = rng.integers(0, pool.n_trees, (3, 5)).astype(np.int32)
    want, _ = check_codes(hip, pool, fidx, X)
    node = pool.node_off[fidx][:, :, None] + want
    assert (pool.var[node] >= 0).any()                                  # rows do stop at split nodes


def test_excluded_columns_stop_the_walk(hip):
    pool, rng = mixed_pool(5, 5)
    X = grid_rows(rng, 65, 5)
    fidx = rng.integers(0, pool.n_trees, (3, 4)).astype(np.int32)
    free, _ = check_codes(hip, pool, fidx, X)
    want, _ = check_codes(hip, pool, fidx, X, excluded=(0, 3, 9, -1))   # (outside [0, p): ignored, as pgb_predict does)
    assert (want != free).any()
    everything, _ = check_codes(hip, pool, fidx, X, excluded=tuple(range(5)))
    assert not everything.any()                                         # every row stops at every root


def test_onehot_and_subset_rules(hip):
    rng = np.random.default_rng(6)
    rules = {0: px.ONEHOT, 1: px.SUBSET}
    split_of = lambda r, j: float(r.integers(0, 4)) if j == 0 else (float(r.integers(1, 64)) if j == 1 else r.integers(-8, 9) / 8.0)  # noqa: E731
    pool = px.build_pool([px.dyadic_tree(rng, 1, 5, [0, 1, 2], split_of, grow=0.9, rules=rules) for _ in range(8)], 1)
    assert set(pool.rule[pool.var >= 0]) == {px.CONT, px.ONEHOT, px.SUBSET}
    X = grid_rows(rng, 70, 3)
    X[:, 0], X[:, 1] = rng.integers(0, 4, 70), rng.integers(0, 6, 70)
    X[3, 2], X[5, 2], X[7, 1] = np.inf, -np.inf, np.nan
    fidx = rng.integers(0, pool.n_trees, (3, 5)).astype(np.int32)
    check_codes(hip, pool, fidx, X)
    check_codes(hip, pool, fidx, X, excluded=(1,))


# ------------------------------------------------------------------ 2. the count
def random_codes(rng, T: int, n: int) -> np.ndarray:
    codes = rng.integers(0, 4, (T, n))                                  # few values: many matches
    codes[rng.random((T, n)) < 0.1] = 254
    codes[rng.random((T, n)) < 0.1] = 128
    return codes


@pytest.mark.parametrize("q", [1, QT - 1, QT, QT + 1, 65])
def test_count_at_every_tile_edge(q, hip):
    rng = np.random.default_rng(q)
    T = 26                                                              # 7 words, two pads
    cq = random_codes(rng, T, q)
    for i, nb in enumerate((1, 63, 64, 65, 130, BT - 1, BT, BT + 1, 2 * BT + 88)):
        cr = random_codes(rng, T, nb)
        cr[:, : min(q, nb)] = np.where(rng.random((T, min(q, nb))) < 0.5, cq[:, : min(q, nb)], cr[:, : min(q, nb)])
        pads = ((0, 0, 0), (3, 0, 0), (0, 5, 0), (0, 0, 7), (1, 2, 3))[i % 5]
        got = dev_count(hip, host.pack(cq), host.pack(cr), pads)
        assert np.array_equal(got, host.distances(cq, cr)), (q, nb)


def test_count_adds_over_draw_chunks_that_end_inside_a_word(hip):
    rng = np.random.default_rng(8)
    q, nb = 17, 70
    cq, cr = random_codes(rng, 10, q), random_codes(rng, 10, nb)
    want = host.distances(cq, cr)
    first = dev_count(hip, host.pack(cq[:5]), host.pack(cr[:5]))       # 5 slots: two words, three pads
    assert np.array_equal(first, host.distances(cq[:5], cr[:5]))
    both = dev_count(hip, host.pack(cq[5:]), host.pack(cr[5:]), pads=(0, 0, 2), dist=first)
    assert np.array_equal(both, want)
    assert np.array_equal(dev_count(hip, host.pack(cq), host.pack(cr)), want)
    assert np.array_equal(host.header_count(host.pack(cq), host.pack(cr)), want)


# ------------------------------------------------------------------ 3. the top-k
@pytest.mark.parametrize("k", [1, 10, 100, 128])
def test_topk_equals_the_recount(k, hip):
    rng = np.random.default_rng(k)
    q, n = 5, 100 if k == 100 else 300                                  # (k = n; and more rows than the workgroup has threads)
    dist = rng.integers(0, 9, (q, n)).astype(np.uint32)                 # ties everywhere
    dist[1] = 4                                                         # all equal: the first k rows in order
    dist[2] = rng.integers(3, 9, n)
    dist[2, n - 1] = 0                                                  # the best neighbour lies in the last block
    for ex in (False, True):
        if ex and k == n:
            continue
        want = host.topk(dist, k, ex)
        for cuts, pad in ((None, 0), ((0, 64, n - 10, n), 3), ((0, n - 1, n), 0)):
            ws = dev_topk(hip, dist, k, cuts, self_row0=0 if ex else -1, pad=pad)
            got = host.split_ws(ws, q, k)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (k, ex, cuts)
            assert np.array_equal(ws, host.header_topk(dist, k, self_row0=0 if ex else -1))
    assert np.array_equal(host.split_ws(dev_topk(hip, dist, k), q, k)[0][1], np.arange(k))
    assert host.split_ws(dev_topk(hip, dist, k, (0, 64, n)), q, k)[0][2, 0] == n - 1


def test_topk_with_queries_that_are_later_rows_and_with_few_candidates(hip):
    rng = np.random.default_rng(9)
    dist = rng.integers(0, 5, (4, 40)).astype(np.uint32)
    for cuts in (None, (0, 3, 5, 40)):
        assert np.array_equal(dev_topk(hip, dist, 6, cuts, self_row0=3), host.header_topk(dist, 6, self_row0=3))
    ws = dev_topk(hip, dist[:, :3].copy(), 5)                           # three candidates for five places
    assert np.array_equal(ws, host.header_topk(dist[:, :3], 5))
    assert np.all(ws[:20].reshape(4, 5)[:, 3:] == host.KEY_NONE)


# ------------------------------------------------------------------ 4. refusals: nothing is launched
def refused(lib, rc, name, message, prefixed=True):
    """The call returned PGB_E_INVALID with ``message``, which carries the entry point's name."""
    assert rc == -1
    with pytest.raises(_abi.PGBError, match=message) as err:
        lib.check(rc, "call")
    assert (name + ": " in str(err.value)) == prefixed


def test_refusals_of_leaf_codes(hip):
    mem, lib = hip.mem, hip.lib
    entry = lib.proximity_entry_points()[0]
    pool, rng = mixed_pool(1, 3)
    carr, fidx = pool.as_c(), np.zeros((2, 3), np.int32)
    xd, cd = mem.from_host(np.zeros((8, 3))), up32(mem, np.full(64, GUARD))
    excl = np.zeros(1, np.int32)
    ok = dict(trees=C.byref(carr), fidx=fidx.ctypes.data, D=2, m=3, X=mem.ptr(xd), n=8, p=3, ldx=3, excl=None, n_excl=0,
              codes=mem.ptr(cd), ldc=8)

    def call(**kw):
        a = {**ok, **kw}
        return entry(a["trees"], a["fidx"], a["D"], a["m"], a["X"], a["n"], a["p"], a["ldx"], a["excl"], a["n_excl"], a["codes"],
                     a["ldc"], mem.stream_ptr)

    name = "pgb_predict_leaf_codes"
    for kw, message in ((dict(trees=None), "trees is null"), (dict(fidx=None), "forest_tree_idx is null"),
                        (dict(X=None), "X_dev is null"), (dict(codes=None), "codes_dev is null"),
                        (dict(D=0), "n_forests, m and p must be >= 1"), (dict(n=0), "n_rows must be >= 1"),
                        (dict(ldx=2), "ldx must be >= p"), (dict(ldc=7), "ldc must be >= n_rows"),
                        (dict(n_excl=1), "excluded_host is null"), (dict(D=1 << 16, m=1 << 16), r"2\^31 - 1 slots"),
                        (dict(n=1 << 38, ldc=1 << 38), r"n_rows exceeds 2\^31 - 1 tiles of 64 rows")):
        refused(lib, call(**kw), name, message)
    # the history's own faults keep the sentences of pgb_predict; the 255-node rule is this entry point's
    bad = np.array([[0, 1, pool.n_trees]] * 2, np.int32)
    refused(lib, call(fidx=bad.ctypes.data), name, "forest_tree_idx entry outside", prefixed=False)
    rng2 = np.random.default_rng(0)
    big = px.build_pool([px.Split(0, 0.0, px.complete_tree(rng2, 1, 7, [0, 1, 2], grid_split), px.Leaf([0.0])), px.Leaf([1.0])], 1)
    assert big.node_off[1] == 257
    cbig = big.as_c()
    refused(lib, call(trees=C.byref(cbig), fidx=np.ones((2, 3), np.int32).ctypes.data), name,
            "tree 0 has 257 nodes: a leaf code is one byte, at most 255 nodes per tree")
    assert np.all(down32(mem, cd) == GUARD)
    assert call(excl=excl.ctypes.data, n_excl=1) == 0                  # (the call, accepted: 2 words of 8 rows)
    got = down32(mem, cd)
    assert not np.any(got[:16] == GUARD) and np.all(got[16:] == GUARD)


def test_refusals_of_the_count(hip):
    mem, lib = hip.mem, hip.lib
    count = lib.proximity_entry_points()[1]
    cq, cr, dd = up32(mem, np.zeros(64)), up32(mem, np.zeros(64)), up32(mem, np.full(64, GUARD))
    ok = dict(cq=mem.ptr(cq), ldq=4, q=4, cr=mem.ptr(cr), ldr=8, nb=8, W=2, dist=mem.ptr(dd), ldo=8)

    def call(**kw):
        a = {**ok, **kw}
        return count(a["cq"], a["ldq"], a["q"], a["cr"], a["ldr"], a["nb"], a["W"], a["dist"], a["ldo"], 1, mem.stream_ptr)

    huge = 1 << 40
    for kw, message in ((dict(cq=None), "cq_dev is null"), (dict(cr=None), "cr_dev is null"), (dict(dist=None), "dist_dev is null"),
                        (dict(q=0), "q must be >= 1"), (dict(nb=0), "nb must be >= 1"), (dict(W=0), "W must be >= 1"),
                        (dict(ldq=3), "ldq must be >= q"), (dict(ldr=7), "ldr must be >= nb"), (dict(ldo=7), "ldo must be >= nb"),
                        (dict(W=(1 << 29) + 1), r"W exceeds the words of 2\^31 - 1 slots"),
                        (dict(q=huge, ldq=huge, nb=huge, ldr=huge, ldo=huge), r"q nb exceeds 2\^31 - 1 tiles")):
        refused(lib, call(**kw), "pgb_prox_count", message)
    assert np.all(down32(mem, dd) == GUARD)
    assert call() == 0
    assert not down32(mem, dd)[:32].any() and np.all(down32(mem, dd)[32:] == GUARD)


def test_refusals_of_the_topk(hip):
    mem, lib = hip.mem, hip.lib
    _, _, topk, query = lib.proximity_entry_points()
    dd = up32(mem, np.zeros(64))
    ws = mem.from_host(np.full(64, 0x7777777777777777, np.uint64).view(np.float64))
    ok = dict(dist=mem.ptr(dd), ldo=8, q=4, nb=8, first=0, self0=-1, k=3, ws=mem.ptr(ws))

    def call(**kw):
        a = {**ok, **kw}
        return topk(a["dist"], a["ldo"], a["q"], a["nb"], a["first"], a["self0"], a["k"], a["ws"], 1, mem.stream_ptr)

    for kw, message in ((dict(dist=None), "dist_dev is null"), (dict(ws=None), "ws_dev is null"), (dict(q=0), "q must be >= 1"),
                        (dict(nb=0), "nb must be >= 1"), (dict(ldo=7), "ldo must be >= nb"),
                        (dict(k=0), r"k must be in \[1, 128\]"), (dict(k=129), r"k must be in \[1, 128\]"),
                        (dict(q=1 << 31), r"q exceeds 2\^31 - 1 queries"), (dict(first=-1), "first_row must be >= 0"),
                        (dict(first=(1 << 32) - 8), r"first_row \+ nb <= 2\^32 - 1")):
        refused(lib, call(**kw), "pgb_prox_topk", message)
    assert np.all(mem.to_host(ws).view(np.uint64) == 0x7777777777777777)
    assert (query(0, 3), query(4, 0), query(4, 129), query(4, 3)) == (0, 0, 0, 8 * 16)
    assert call(first=(1 << 32) - 9) == 0
    got = mem.to_host(ws).view(np.uint64)
    assert np.all(got[:3] == np.arange((1 << 32) - 9, (1 << 32) - 6, dtype=np.uint64)) and not got[12:16].any()


# ------------------------------------------------------------------ 5. the public calls on short real chains
N, P, M_TREES = 200, 5, 9


def _data(seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, P))
    f = 2.0 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 1.5 * (X[:, 2] - 0.5) + X[:, 3]
    return rng, X, f


@pytest.fixture(scope="module")
def one_chain(hip):
    rng, X, f = _data(51)
    op = BARTOp(X, f + rng.normal(0, 0.5, N), m=M_TREES)
    attach_history(op, [sample_chain(op, 5, 8, random_seed=4, chain=0, backend=hip, keep_draws=False)])
    return X, _get_posterior_sampler(op, backend=hip)


@pytest.fixture(scope="module")
def two_chains(hip):
    """Two chains behind one sampler: 2 x 8 pooled draws of 9 trees, and everything the tests below compare against."""
    rng, X, f = _data(52)
    op = BARTOp(X, f + rng.normal(0, 0.5, N), m=M_TREES)
    attach_history(op, [sample_chain(op, 5, 8, random_seed=5, chain=c, backend=hip, keep_draws=False) for c in (0, 1)])
    s = _get_posterior_sampler(op, backend=hip)
    Xq = rng.uniform(0, 1, (65, P))
    Xq[0] = X[N - 1]                                                    # the nearest row of query 0 is the LAST reference row
    Xq[1] = X[7]
    Xq[2, 1] = np.nan
    _, pool, fidx = _stored.history(s)
    codes = host.stop_nodes(pool, fidx, np.vstack([X, Xq])).reshape(-1, N + 65)
    return {"X": X, "Xq": Xq, "s": s, "T": codes.shape[0], "ref": codes[:, :N], "qry": codes[:, N:],
            "dist": host.distances(codes[:, N:], codes[:, :N])}


def test_leaf_ids_on_a_real_chain(one_chain, monkeypatch):
    X, s = one_chain
    _, pool, fidx = _stored.history(s)
    want = host.stop_nodes(pool, fidx, X)
    got = leaf_ids(s, X)
    assert got.dtype == np.uint8 and got.shape == (8, M_TREES, N) and np.array_equal(got, want)
    assert (pool.var[pool.node_off[np.asarray(fidx)][:, :, None] + want] < 0).all()      # no NaN, nothing excluded: leaves
    assert len({tuple(c) for c in want.reshape(-1, N).T}) > 1
    draws = [5, 0, 5]
    assert np.array_equal(leaf_ids(s, X[:70], draws=draws, excluded=[0]), host.stop_nodes(pool, np.asarray(fidx)[draws], X[:70], [0]))
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "1")                       # the floor: blocks of 64 rows
    assert np.array_equal(leaf_ids(s, X), want)


def test_leaf_ids_on_two_pooled_chains(two_chains):
    f = two_chains
    got = leaf_ids(f["s"], f["X"])
    assert got.shape == (16, M_TREES, N) and np.array_equal(got.reshape(-1, N), f["ref"])
    assert np.array_equal(leaf_ids(f["s"], f["Xq"]).reshape(-1, 65), f["qry"])


def test_leaf_ids_of_a_categorical_fit(hip):
    rng, X, f = _data(53)
    y = np.digitize(f + rng.normal(0, 0.5, N), [1.0, 2.0]).astype(np.float64)
    op = BARTOp(X, y, m=M_TREES)
    res = sample_chain(op, 5, 8, num_particles=10, random_seed=6, chain=0, backend=hip, keep_draws=False,
                       likelihood=CategoricalLikelihood(3))
    base, batches = res["history"]
    s = PosteriorSampler.from_history(batches, base, M_TREES, 3, backend=hip)
    _, pool, fidx = _stored.history(s)
    assert pool.n_outputs == 3
    assert np.array_equal(leaf_ids(s, X[:130]), host.stop_nodes(pool, fidx, X[:130]))


def test_proximity_of_rows_to_themselves(two_chains):
    f = two_chains
    res = proximity(f["s"], f["X"][:70])
    T = f["T"]
    assert res["n_slots"] == T == 16 * M_TREES and res["matches"].dtype == np.uint32
    assert np.array_equal(res["matches"], res["matches"].T) and np.all(np.diag(res["matches"]) == T)
    assert np.array_equal(res["matches"], T - host.distances(f["ref"][:, :70], f["ref"][:, :70]))
    assert np.array_equal(res["similarity"], res["matches"] / float(T))


@pytest.fixture
def row_blocks(monkeypatch):
    """-> the lists of row blocks the calls of a test make."""
    seen = []
    real = _stored.row_blocks

    def recording(n, bytes_per_row, limit):
        seen.append(real(n, bytes_per_row, limit))
        return seen[-1]

    monkeypatch.setattr(_stored, "row_blocks", recording)
    return seen


def test_proximity_does_not_depend_on_the_blocking(two_chains, row_blocks, monkeypatch):
    f = two_chains
    Xq = np.vstack([f["Xq"], f["X"][:135]])                             # 200 queries: at the floor the draws go in two chunks
    want = f["T"] - np.vstack([f["dist"], host.distances(f["ref"][:, :135], f["ref"])])
    one = proximity(f["s"], Xq, f["X"])
    assert np.array_equal(one["matches"], want) and row_blocks == [[(0, N)]]
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "1")                       # the floor, 64 KiB
    chunks = prox_mod.ProximityJob(f["s"], Xq, f["X"]).draw_chunks(200)
    assert len(chunks) == 2 and ((chunks[0][1] - chunks[0][0]) * M_TREES) % 4 != 0   # the first chunk ends inside a word
    cut = proximity(f["s"], Xq, f["X"])
    assert len(row_blocks) == 2 and len(row_blocks[1]) == 4
    assert np.array_equal(cut["matches"], want) and np.array_equal(cut["similarity"], one["similarity"])


@pytest.mark.parametrize("k", [1, 10, 100, 128])
def test_nearest_rows(k, two_chains, row_blocks, monkeypatch):
    f = two_chains
    ref = f["X"][:100] if k == 100 else f["X"]                          # k = n
    n = ref.shape[0]
    widx, wdk, wtotal = host.topk(f["dist"][:, :n], k)
    one = nearest_rows(f["s"], f["Xq"], ref, k=k)
    assert one["index"].dtype == np.int64 and np.array_equal(one["index"], widx)
    assert np.array_equal(one["matches"], f["T"] - wdk) and one["n_slots"] == f["T"]
    assert np.array_equal(one["similarity"], one["matches"] / float(f["T"]))
    assert np.array_equal(one["mean_similarity"], (n * f["T"] - wtotal) / float(n * f["T"]))
    if n == N:
        assert one["index"][0, 0] == N - 1 and one["matches"][0, 0] == f["T"]
        assert one["index"][1, 0] == 7
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "1")                       # blocks of 64 rows: the best row of query 0 in the last
    cut = nearest_rows(f["s"], f["Xq"], ref, k=k)
    assert [len(b) for b in row_blocks] == [1, -(-n // 64)]
    assert all(np.array_equal(one[key], cut[key]) for key in ("index", "matches", "mean_similarity"))


def test_nearest_rows_ties_exclude_self_and_the_mean(two_chains):
    f = two_chains
    X = np.vstack([f["X"][:60], f["X"][:30]])                           # rows 60 .. 89 repeat rows 0 .. 29: exact ties
    codes = np.hstack([f["ref"][:, :60], f["ref"][:, :30]])
    dist = host.distances(codes, codes)
    T, n = f["T"], 90
    prox = proximity(f["s"], X)
    assert np.array_equal(prox["matches"], T - dist)
    got = nearest_rows(f["s"], X, k=10)
    widx, wdk, wtotal = host.topk(dist, 10)
    assert np.array_equal(got["index"], widx) and np.array_equal(got["matches"], T - wdk)
    assert np.all(got["index"][:30, 0] == np.arange(30)) and np.all(got["index"][60:, 0] == np.arange(30))   # the smaller index
    assert np.all(got["index"][60:, 1] == np.arange(60, 90)) and np.all(got["matches"][60:, :2] == T)
    assert np.array_equal(got["mean_similarity"], prox["matches"].sum(1, dtype=np.int64) / float(n * T))
    assert np.allclose(got["mean_similarity"], prox["similarity"].mean(1), rtol=1e-12, atol=0)
    out = nearest_rows(f["s"], X, k=89, exclude_self=True)
    widx, wdk, wtotal = host.topk(dist, 89, exclude_self=True)
    assert np.array_equal(out["index"], widx) and np.array_equal(out["matches"], T - wdk)
    assert not (out["index"] == np.arange(n)[:, None]).any()
    assert np.all(out["index"][:30, 0] == np.arange(60, 90)) and np.all(out["index"][60:, 0] == np.arange(30))
    assert np.array_equal(out["mean_similarity"], ((n - 1) * T - wtotal) / float((n - 1) * T))
