"""Posterior proximity on the build box (no GPU): the contract of ``include/pgbart_proximity.h`` -- the byte-mismatch
count, the packing and its tail pad, the sequential references -- against an independent NumPy recount
(``tests/_proximity_host.py``), the identities the contract promises (row blocks, draw chunks and the top-k merge change
no bit), the host-side validation of ``pymc_bart_amd.proximity``, and the library's exports and budget.

Every comparison is an exact integer equality."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _predict_exact as px
import _proximity_host as host
from pymc_bart_amd import _abi, compiled, leaf_ids, nearest_rows, proximity

prox_mod = sys.modules["pymc_bart_amd.proximity"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def naive_mismatch(a: int, b: int) -> int:
    return sum(((a >> (8 * k)) & 0xFF) != ((b >> (8 * k)) & 0xFF) for k in range(4))


def pool_of(seed: int, p: int = 4, K: int = 1):
    """complete, chain and random trees on ``p`` columns with split values on a grid of eighths, so that rows drawn
    from the same grid hit split values exactly."""
    rng = np.random.default_rng(seed)
    split_of = lambda r, j: r.integers(-8, 9) / 8.0  # noqa: E731
    cols = list(range(p))
    roots = [px.complete_tree(rng, K, 3, cols, split_of), px.chain_tree(rng, K, 6, cols, split_of, "left"),
             px.chain_tree(rng, K, 5, cols, split_of, "right"), px.Leaf([0.5] * K)]
    roots += [px.dyadic_tree(rng, K, 5, cols, split_of) for _ in range(5)]
    return px.build_pool(roots, K), rng


def rows_of(rng, n: int, p: int, nan_rate: float = 0.0) -> np.ndarray:
    X = rng.integers(-10, 11, (n, p)) / 8.0
    if nan_rate:
        X[rng.random((n, p)) < nan_rate] = np.nan
    return X


def table(rng, n_trees: int, D: int, m: int) -> np.ndarray:
    return rng.integers(0, n_trees, (D, m)).astype(np.int32)


# ------------------------------------------------------------------ 1. the byte-mismatch count
def test_mismatch4_equals_the_naive_byte_loop():
    L = host.lib()
    edge = (0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF)
    words = [b0 | (b1 << 8) | (b2 << 16) | (b3 << 24) for b0 in edge for b1 in edge for b2 in edge for b3 in edge]
    rng = np.random.default_rng(5)
    pairs = [(a, b) for a in words[::7] for b in words[::11]]
    pairs += [(a, a) for a in words] + [(a, a ^ (0xFF << (8 * k))) for a in words[::5] for k in range(4)]
    pairs += [(int(a), int(b)) for a, b in rng.integers(0, 1 << 32, (4000, 2), dtype=np.uint64)]
    for a, b in pairs:
        assert L.prox_mismatch4(a, b) == naive_mismatch(a, b), (hex(a), hex(b))
    # every byte position on its own, every pair of edge bytes
    for k in range(4):
        for x in edge:
            for y in edge:
                assert L.prox_mismatch4(x << (8 * k), y << (8 * k)) == int(x != y)


def test_the_constants_agree_with_the_python_layer():
    L = host.lib()
    assert (L.prox_pad(), L.prox_max_k(), L.prox_max_nodes()) == (prox_mod.PAD, prox_mod.MAX_K, 255)
    assert L.prox_max_slots() == prox_mod.MAX_SLOTS == 2 ** 31 - 1
    for T in (1, 3, 4, 5, 15, 16, 17, 2 ** 31 - 1):
        assert L.prox_words(T) == prox_mod.words(T) == -(-T // 4)
    for q, k in ((1, 1), (7, 10), (65, 128)):
        assert 8 * L.prox_topk_ws_words(q, k) == prox_mod.topk_workspace_bytes(q, k)


# ------------------------------------------------------------------ 2. packing and the tail pad
@pytest.mark.parametrize("D, m", [(1, 1), (1, 3), (1, 4), (1, 5), (3, 5), (5, 3), (1, 15)])
def test_packing_and_the_tail_pad(D, m):
    pool, rng = pool_of(D * 100 + m)
    X, fidx = rows_of(rng, 9, 4), table(rng, pool.n_trees, D, m)
    T = D * m
    assert T in (1, 3, 4, 5, 15)
    want = host.stop_nodes(pool, fidx, X).reshape(T, 9)
    words = host.header_codes(pool, fidx, X, ldc=11)
    assert words.shape == (-(-T // 4), 11)
    assert np.all(words[:, 9:] == 0xDEADBEEF)                      # nothing written beyond the rows
    assert np.array_equal(words[:, :9], host.pack(want))
    by = words[:, :9].copy().view(np.uint8).reshape(-1, 9, 4)      # little endian: byte b of word w is slot 4 w + b
    for s in range(4 * words.shape[0]):
        assert np.array_equal(by[s // 4, :, s % 4], want[s] if s < T else np.full(9, 0xFF)), s
    assert np.array_equal(prox_mod.unpack_codes(words[:, :9], D, m), want.reshape(D, m, 9))


# ------------------------------------------------------------------ 3. the sequential references against the recount
@pytest.mark.parametrize("variant", ["plain", "nan", "excluded", "rules"])
def test_the_header_equals_the_recount(variant):
    p = 4
    pool, rng = pool_of(11)
    excluded = ()
    if variant == "rules":
        rules = {0: px.ONEHOT, 1: px.SUBSET}
        split_of = lambda r, j: float(r.integers(0, 4)) if j == 0 else (float(r.integers(1, 64)) if j == 1 else r.integers(-8, 9) / 8.0)  # noqa: E731
        pool = px.build_pool([px.dyadic_tree(rng, 1, 5, list(range(p)), split_of, rules=rules) for _ in range(8)], 1)
    X = rows_of(rng, 37, p, nan_rate=0.15 if variant == "nan" else 0.0)
    if variant == "rules":
        X[:, 0], X[:, 1] = rng.integers(0, 4, 37), rng.integers(0, 6, 37)
        X[3, 2], X[5, 0] = np.inf, -np.inf
    if variant == "excluded":
        excluded = (1, 3, 7, -2)                                       # (outside [0, p): ignored, as pgb_predict does)
    D, m = 3, 5
    fidx = table(rng, pool.n_trees, D, m)
    want = host.stop_nodes(pool, fidx, X, excluded)
    L, carr = host.lib(), pool.as_c()
    fl = host._flags(excluded, p)
    for t in range(pool.n_trees):                                      # pgb_prox_stop, one row and one tree at a time
        for i in (0, 5, 36):
            x = np.ascontiguousarray(X[i])
            assert L.prox_stop(C.addressof(carr), t, x.ctypes.data, None if fl is None else fl.ctypes.data) == \
                host.stop_node(pool, t, X[i], {1, 3} if variant == "excluded" else set())
    codes = want.reshape(D * m, 37)
    words = host.header_codes(pool, fidx, X, excluded)
    assert np.array_equal(words, host.pack(codes))
    if variant in ("nan", "excluded"):                                 # rows do stop at inner nodes
        is_split = np.array([[pool.var[pool.node_off[fidx[d, t]] + want[d, t]] >= 0 for t in range(m)] for d in range(D)])
        assert is_split.any()
    q = 7
    dist = host.header_count(words[:, :q].copy(), words)
    assert np.array_equal(dist, host.distances(codes[:, :q], codes))
    assert np.all(np.diag(dist[:, :q]) == 0)
    for k, ex in ((1, False), (5, False), (37, False), (36, True), (5, True)):
        idx, dk, total = host.split_ws(host.header_topk(dist, k, self_row0=0 if ex else -1), q, k)
        widx, wdk, wtotal = host.topk(dist, k, ex)
        assert np.array_equal(idx, widx) and np.array_equal(dk, wdk) and np.array_equal(total, wtotal), (k, ex)


# ------------------------------------------------------------------ 4. no bit depends on the cut
def test_row_blocks_carry_nothing_and_draw_chunks_add():
    pool, rng = pool_of(21)
    X = rows_of(rng, 50, 4, nan_rate=0.05)
    D, m, q = 4, 5, 9                                                    # T = 20; chunks of 1 and 3 draws end inside a word
    fidx = table(rng, pool.n_trees, D, m)
    codes = host.stop_nodes(pool, fidx, X).reshape(D * m, 50)
    want = host.distances(codes[:, :q], codes)
    words = host.header_codes(pool, fidx, X)
    # row blocks: every block starts its own distances (init), columns side by side
    got = np.hstack([host.header_count(words[:, :q].copy(), words[:, r0:r1].copy()) for r0, r1 in ((0, 17), (17, 49), (49, 50))])
    assert np.array_equal(got, want)
    # draw chunks, each packed on its own with its own tail pad: init, then continue
    for cuts in ((0, 1, 4), (0, 3, 4), (0, 1, 2, 3, 4), (0, 4)):
        dist = None
        for d0, d1 in zip(cuts[:-1], cuts[1:]):
            wchunk = host.header_codes(pool, fidx[d0:d1], X)
            assert ((d1 - d0) * m) % 4 == 0 or np.all(wchunk[-1] >> np.uint32(24) == 0xFF)
            dist = host.header_count(wchunk[:, :q].copy(), wchunk, dist=dist)
        assert np.array_equal(dist, want), cuts
    # continuing from stored distances adds to them
    twice = host.header_count(words[:, :q].copy(), words, dist=host.header_count(words[:, :q].copy(), words))
    assert np.array_equal(twice, 2 * want)


@pytest.mark.parametrize("case", ["random", "all equal", "best in the last block", "exclude self"])
def test_the_topk_merge_over_blocks_equals_the_one_block_result(case):
    rng = np.random.default_rng(3)
    q, n = 6, 41
    dist = rng.integers(0, 12, (q, n)).astype(np.uint32)                # (many ties)
    if case == "all equal":
        dist[:] = 7
    if case == "best in the last block":
        dist[:] = rng.integers(5, 12, (q, n))
        dist[:, n - 1] = 0
        dist[2, n - 2] = 0
    ex = case == "exclude self"
    for k in (1, 4, 35, 40):
        one = host.header_topk(dist, k, self_row0=0 if ex else -1)
        for cuts in ((0, 16, 32, 41), (0, 40, 41), (0, 1, 41)):
            ws = None
            for r0, r1 in zip(cuts[:-1], cuts[1:]):
                ws = host.header_topk(dist[:, r0:r1], k, first_row=r0, self_row0=0 if ex else -1, ws=ws)
            assert np.array_equal(ws, one), (k, cuts)
        idx, dk, total = host.split_ws(one, q, k)
        widx, wdk, wtotal = host.topk(dist, k, ex)
        assert np.array_equal(idx, widx) and np.array_equal(dk, wdk) and np.array_equal(total, wtotal), k
        if case == "all equal":
            assert np.array_equal(idx, np.tile(np.arange(k), (q, 1)))   # ties go to the smaller row index
        if case == "best in the last block":
            assert np.all(idx[[0, 1, 3, 4, 5], 0] == n - 1) and idx[2, 0] == n - 2
    # fewer candidates than places: the rest of the list stays at the all-ones key
    ws = host.header_topk(dist[:, :3], 5)
    assert np.all(ws[:q * 5].reshape(q, 5)[:, 3:] == host.KEY_NONE)


# ------------------------------------------------------------------ 5. the Python layer
def test_argument_errors_are_raised_before_a_backend_is_touched():
    from test_pointwise import _sampler

    s = _sampler(draws=5)
    X = np.zeros((8, 2))
    calls = (lambda **kw: leaf_ids(s, X, **kw), lambda **kw: proximity(s, X, **kw), lambda **kw: nearest_rows(s, X, k=3, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="draws must index"):
            call(draws=[0, 5])
        with pytest.raises(ValueError, match="at least 1 draw"):
            call(draws=[])
        with pytest.raises(ValueError, match="excluded must index"):
            call(excluded=[2])
        with pytest.raises(AttributeError):                 # a call that passes every check reaches the backend (none)
            call(draws=[4, 0], excluded=[1])
    for fn in (leaf_ids, proximity, nearest_rows):
        with pytest.raises(ValueError, match="matrix"):
            fn(s, np.zeros((2, 2, 2)))
        with pytest.raises(TypeError, match="sampler must be"):
            fn(object(), X)
    for fn in (proximity, nearest_rows):
        with pytest.raises(ValueError, match=r"X_ref must have the 2 columns of X, got shape \(8, 3\)"):
            fn(s, X, np.zeros((8, 3)))
        with pytest.raises(ValueError, match="matrix"):
            fn(s, X, np.zeros((2, 2, 2)))
    # the k rules
    for bad in (0, -1, 129):
        with pytest.raises(ValueError, match=r"k must be in \[1, 128\]"):
            nearest_rows(s, X, k=bad)
    with pytest.raises(ValueError, match="k = 9 neighbours of 8 reference rows"):
        nearest_rows(s, X, k=9)
    with pytest.raises(ValueError, match="k = 8 neighbours of 7 reference rows"):
        nearest_rows(s, X, k=8, exclude_self=True)
    with pytest.raises(ValueError, match="k = 4 neighbours of 3 reference rows"):
        nearest_rows(s, X, np.zeros((3, 2)), k=4)
    with pytest.raises(ValueError, match="exclude_self .* takes no X_ref"):
        nearest_rows(s, X, X, k=3, exclude_self=True)
    for ok in (lambda: nearest_rows(s, X, k=8), lambda: nearest_rows(s, X, k=7, exclude_self=True),
               lambda: nearest_rows(s, X, np.zeros((3, 2)), k=3), lambda: nearest_rows(s, np.zeros(8), k=1)):
        with pytest.raises(AttributeError):
            ok()


def test_the_draw_chunks_follow_the_block_rule(monkeypatch):
    from test_pointwise import _sampler

    s = _sampler(draws=7, m=3)
    job = prox_mod.ProximityJob(s, np.zeros((65, 2)))
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    assert job.draw_chunks(65) == [(0, 7)] and job.T == 21
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "1")                       # the floor: 64 KiB
    assert job.draw_chunks(65) == [(0, 7)]                              # 32 KiB / (4 * 129) = 63 words: 252 slots
    assert job.draw_chunks(3000) == [(0, 2), (2, 4), (4, 6), (6, 7)]    # 2 words: 8 slots, two draws of three trees
    assert job.draw_chunks(100000) == [(d, d + 1) for d in range(7)]    # at least one draw


def test_a_backend_that_is_not_hip_is_refused():
    from _oracle import oracle_backend
    from pymc_bart_amd.trees import PosteriorSampler
    from test_pointwise import _sampler

    s = _sampler(draws=5)
    ps = PosteriorSampler(s.pool, s.forest_idx, s.m, 1, backend=oracle_backend())
    X = np.zeros((8, 2))
    for call in (lambda: leaf_ids(ps, X), lambda: proximity(ps, X), lambda: nearest_rows(ps, X, k=2)):
        with pytest.raises(_abi.PGBError, match="HIP backend only"):
            call()


# ------------------------------------------------------------------ 6. the library
@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_points(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    if not os.path.exists(path):
        pytest.skip(f"{so} has not been built")
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    for name in ("pgb_predict_leaf_codes", "pgb_prox_count", "pgb_prox_topk", "pgb_prox_topk_workspace_bytes"):
        assert f" {name}\n" in syms and name not in _abi.SYMBOLS, name


def test_the_kernels_are_budgeted_without_scratch():
    budget = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    names = [f"k_leaf_codes<{a}, {b}>" for a in ("false", "true") for b in ("false", "true")] + ["k_prox_count", "k_prox_topk"]
    for name in names:
        row = budget[name]
        assert row["max_scratch_bytes"] == 0 and row["max_vgpr_spills"] == 0, name
    assert budget["k_prox_count"]["min_wgs_per_cu"] == 8               # 16 accumulators: eight waves per SIMD


def test_the_timing_tool_answers_help_and_counts_the_loop_of_the_count_kernel(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import timing_proximity as tool

    with pytest.raises(SystemExit) as e:
        tool.main(["--help"])
    assert e.value.code == 0 and capsys.readouterr().out.startswith("usage:")
    if not os.path.exists(os.path.join(ROOT, "pymc_bart_amd", "csrc", "libpgbart_hip.so")):
        pytest.skip("libpgbart_hip.so has not been built")
    per_word = tool.valu_per_word()
    # 16 queries x (xor, and, add, or3, population count) and at most a few address instructions: the five VALU
    # instructions per four byte comparisons the bound of profiles/proximity_timing.json is computed from
    assert per_word is not None and 5 * tool.QUERY_TILE <= per_word <= 5 * tool.QUERY_TILE + 4
