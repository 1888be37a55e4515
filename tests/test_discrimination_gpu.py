"""ROC AUC, KS and threshold counts on the MI355X: ``pgb_rank_keys`` (``k_rank_keys``) against the host build of
``include/pgbart_rank.h`` (``tests/_rank_host.py``) and ``pgb_rank_metrics`` (the segmented sort, ``k_rank_count``,
``k_rank_thr``) against the header's pair-counting reference, with guards behind every buffer, over the row counts,
segment lengths, groups, draws, thresholds and score patterns at which the kernels take another path; draws split over
two calls and rows permuted; every refusal; then ``discrimination`` end to end on a two-chain probit fit.

Every compared value is an integer (a key, a count) and is compared with ``np.array_equal``."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _rank_host as host
from pymc_bart_amd import BARTOp, BernoulliLikelihood, discrimination, discrimination_matrix
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.utils import _get_posterior_sampler

disc = importlib.import_module("pymc_bart_amd.discrimination")   # (the package's attribute of that name is the function)
pytestmark = pytest.mark.gpu

GUARD = -7.75e300              # behind every buffer of doubles
KEY_GUARD = 0x5A5A5A5A5A5A5A5A  # in the keys before a call and behind them; behind the workspace
INT_GUARD = -77
E_INVALID = -1


def _i64(u):
    return np.ascontiguousarray(u).view(np.int64)


# ------------------------------------------------------------------ pgb_rank_keys
def _keys(hip, a, dest, n, transform, off=None, pad=3, counters=(0, 0), change=None):
    """The entry point on ``a`` ``(D, nb)`` handed over with ``ld = nb + pad``.  ``change``: arguments replaced after
    everything is laid out.  -> ``(rc, keys (D, n) uint64, counters (2,), guards untouched)``."""
    mem = hip.mem
    D, nb = a.shape
    ld = nb + pad
    wide = np.full((D, ld), GUARD)
    wide[:, :nb] = a
    ad = mem.from_host(np.concatenate([wide.ravel(), np.full(64, GUARD)]))
    kd = mem.from_host(_i64(np.full(D * n + 64, KEY_GUARD, np.uint64)))
    cd = mem.from_host(np.array([counters[0], counters[1], INT_GUARD, INT_GUARD], np.int64))
    dd = mem.from_host(np.concatenate([np.ascontiguousarray(dest, np.int64), np.full(8, 1 << 40, np.int64)]))
    offd = None if off is None else mem.from_host(np.concatenate([np.ascontiguousarray(off, np.float64), np.full(8, GUARD)]))
    arg = dict(a=mem.ptr(ad), D=D, nb=nb, ld=ld, off=None if offd is None else mem.ptr(offd),
               transform=host.TRANSFORMS[transform] if isinstance(transform, str) else transform, dest=mem.ptr(dd), n=n,
               keys=mem.ptr(kd), cnt=mem.ptr(cd))
    arg.update(change or {})
    rc = hip.lib.rank_entry_points()[0](arg["a"], arg["D"], arg["nb"], arg["ld"], arg["off"], arg["transform"], arg["dest"], arg["n"],
                                        arg["keys"], arg["cnt"], mem.stream_ptr)
    got_k, got_c, got_a = mem.to_host(kd).view(np.uint64), mem.to_host(cd), mem.to_host(ad)
    guards = bool(np.all(got_k[D * n:] == np.uint64(KEY_GUARD)) and np.all(got_c[2:] == INT_GUARD)
                  and np.array_equal(got_a.view(np.int64), np.concatenate([wide.ravel(), np.full(64, GUARD)]).view(np.int64)))
    return rc, got_k[:D * n].reshape(D, n).copy(), got_c[:2].copy(), guards


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("D,transform,nan", [(1, "identity", True), (5, "logistic", True), (5, "probit", False), (5, "identity", False)])
def test_the_keys_equal_the_header_with_a_dest_that_reverses_the_rows(hip, nb, D, transform, nan):
    """``ld = nb + 3``, ``n = nb + 7``: the rows land reversed behind seven positions that nobody writes.  A NaN under
    the identity and the logistic transform only (``pgb_lphi_t``'s rule forbids a NaN under probit, as
    ``test_survival_gpu.py`` notes); the infinities and both zeros everywhere."""
    rng = np.random.default_rng(1000 + 7 * nb + D)
    n = nb + 7
    a = rng.normal(0.0, 1.5, (D, nb))
    dest = n - 1 - np.arange(nb)
    a[0, 0] = np.nan if nan else -0.0
    if nb >= 63:
        a[D - 1, [5, 6, 7, 8]] = [np.inf, -np.inf, -0.0, 0.0]
        a[D // 2, 40] = np.nan if nan else 40.0
    for off in (None, rng.normal(0, 0.3, nb)):
        rc, got, cnt, guards = _keys(hip, a, dest, n, transform, off, counters=(2, 0))
        hip.lib.check(rc, "pgb_rank_keys")
        want, want_c = host.keys_block(a, transform, dest, n, off, keys=np.full((D, n), KEY_GUARD, np.uint64),
                                       counters=np.array([2, 0], np.uint64))
        assert guards and np.array_equal(got, want), int((got != want).sum())
        assert cnt.tolist() == want_c.astype(np.int64).tolist() and (cnt[0] > 2) == nan
        assert np.all(got[:, :7] == np.uint64(KEY_GUARD))
        if transform == "identity" and off is None:
            assert np.array_equal(got[:, 7:][:, ::-1], host.key(a))


def test_a_dest_out_of_range_writes_nothing_and_is_counted(hip):
    rng = np.random.default_rng(1100)
    a = rng.normal(size=(3, 70))
    dest = np.arange(70)
    dest[[0, 13, 69]] = [-1, 80, 1 << 33]
    rc, got, cnt, guards = _keys(hip, a, dest, 80, "identity")
    want, want_c = host.keys_block(a, "identity", dest, 80, keys=np.full((3, 80), KEY_GUARD, np.uint64))
    assert rc == 0 and guards and np.array_equal(got, want) and cnt.tolist() == [0, 9] == want_c.astype(np.int64).tolist()


# ------------------------------------------------------------------ pgb_rank_metrics
def _metrics(hip, keys, seg_off, thr, counters=(0, 0), change=None):
    """The entry point on laid-out ``keys`` ``(D, n)`` uint64.  -> ``(rc, out (D, G, 2 + 2 T), counts (2,), guards
    untouched, the keys and the workspace after the call)``."""
    mem = hip.mem
    D, n = keys.shape
    seg_off, thr = np.ascontiguousarray(seg_off, np.int64), np.ascontiguousarray(thr, np.float64)
    G, T = (seg_off.size - 1) // 2, thr.size
    ws_bytes = int(hip.lib.rank_entry_points()[1](D, n, G))
    assert ws_bytes >= 8 * D * n and ws_bytes % 8 == 0
    kd = mem.from_host(_i64(np.concatenate([keys.ravel(), np.full(64, KEY_GUARD, np.uint64)])))
    wd = mem.from_host(_i64(np.full(ws_bytes // 8 + 64, KEY_GUARD, np.uint64)))
    cd = mem.from_host(np.array([counters[0], counters[1], INT_GUARD], np.int64))
    n_out = D * G * (2 + 2 * T)
    out, counts = np.full(n_out + 16, INT_GUARD, np.int64), np.full(4, INT_GUARD, np.int64)
    arg = dict(keys=mem.ptr(kd), ws=mem.ptr(wd), D=D, n=n, seg_off=seg_off.ctypes.data, G=G, thr=thr.ctypes.data if T else None, T=T,
               cnt=mem.ptr(cd), out=out.ctypes.data, counts=counts.ctypes.data)
    arg.update(change or {})
    rc = hip.lib.rank_entry_points()[2](arg["keys"], arg["ws"], arg["D"], arg["n"], arg["seg_off"], arg["G"], arg["thr"], arg["T"],
                                        arg["cnt"], arg["out"], arg["counts"], mem.stream_ptr)
    got_k, got_w, got_c = mem.to_host(kd).view(np.uint64), mem.to_host(wd).view(np.uint64), mem.to_host(cd)
    guards = bool(np.all(got_k[D * n:] == np.uint64(KEY_GUARD)) and np.all(got_w[ws_bytes // 8:] == np.uint64(KEY_GUARD))
                  and got_c.tolist() == [counters[0], counters[1], INT_GUARD] and np.all(out[n_out:] == INT_GUARD)
                  and np.all(counts[2:] == INT_GUARD))
    return rc, out[:n_out].reshape(D, G, 2 + 2 * T).copy(), counts[:2].copy(), guards, got_k[:D * n], got_w[:ws_bytes // 8]


LENGTHS = [(1, 1), (1, 300), (63, 65), (64, 64), (257, 255), (1025, 1)]     # (negatives, positives) of a group


def _scores(rng, pattern, D, n):
    if pattern == "equal":
        return np.full((D, n), 0.625)
    v = rng.normal(size=(D, n))
    if pattern == "ties":
        v = np.round(v * 2.0) / 2.0                                            # eight levels hold nearly all of them
        v = np.clip(v, -2.0, 1.5)
    if n >= 8:                                                                 # the infinities and both zeros, in every draw
        at = rng.choice(n, 4, replace=False)
        v[:, at] = [np.inf, -np.inf, -0.0, 0.0]
    return v


def _thresholds(rng, T, v):
    if T == 0:
        return np.empty(0)
    if T == 1:
        return np.array([0.0])
    return np.concatenate([[-np.inf, np.inf, -0.0, v.flat[0], v.min(), v.max()], rng.choice(v.ravel(), 26), rng.normal(size=32)])


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("first", range(len(LENGTHS)))
def test_the_metrics_equal_pair_counting(hip, first, G):
    """Group ``g`` has the lengths ``LENGTHS[(first + g) % 6]``; inside, ``D`` in {1, 7}, ``T`` in {0, 1, 64} and the
    three score patterns.  The reference sees the keys unsorted."""
    rng = np.random.default_rng(2000 + 10 * first + G)
    lens = [LENGTHS[(first + g) % len(LENGTHS)] for g in range(G)]
    seg_off = np.concatenate([[0], np.cumsum(np.ravel(lens))]).astype(np.int64)
    n = int(seg_off[-1])
    for D in (1, 7):
        for T in (0, 1, 64):
            for pattern in ("equal", "distinct", "ties"):
                v = _scores(rng, pattern, D, n)
                thr = _thresholds(rng, T, v)
                keys, _ = host.keys_block(v, "identity", np.arange(n), n)
                rc, out, counts, guards, _, _ = _metrics(hip, keys, seg_off, thr)
                hip.lib.check(rc, "pgb_rank_metrics")
                want = host.reference(keys, seg_off, thr)
                assert guards and counts.tolist() == [0, 0], (D, T, pattern)
                assert np.array_equal(out, want), (D, T, pattern, int((out != want).sum()))
                if pattern == "equal":
                    n0, n1 = np.array(lens).T
                    assert np.all(out[:, :, 0] == n1 * n0) and np.all(out[:, :, 1] == 0)


def test_nan_keys_are_counted_above_everything_and_reported(hip):
    rng = np.random.default_rng(2100)
    v = rng.normal(size=(2, 140))
    v[1, [3, 100]] = np.nan
    seg_off = np.array([0, 70, 140])
    keys, cnt = host.keys_block(v, "identity", np.arange(140), 140)
    rc, out, counts, guards, _, _ = _metrics(hip, keys, seg_off, [0.0, np.inf], counters=(int(cnt[0]), 0))
    assert rc == 0 and guards and counts.tolist() == [2, 0] and np.array_equal(out, host.reference(keys, seg_off, [0.0, np.inf]))
    assert out[1, 0, 3] == 1 and out[1, 0, 5] == 1 and out[0, 0, 3] == 0                    # a NaN key is >= +inf


def _through_both(hip, v, cls, gid, G, thr, transform="identity", off=None, rows=64):
    """Layout, ``pgb_rank_keys`` in blocks of ``rows`` rows, ``pgb_rank_metrics`` -> ``out``."""
    mem = hip.mem
    D, n = v.shape
    seg_off, dest = host.layout(cls, gid, G)
    keys_fn, ws_query, metrics_fn = hip.lib.rank_entry_points()
    kd, cd = mem.empty((D * n,), np.float64), mem.from_host(np.zeros(2, np.int64))
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        ad, dd = mem.from_host(np.ascontiguousarray(v[:, r0:r1])), mem.from_host(dest[r0:r1])
        od = None if off is None else mem.from_host(off[r0:r1])
        hip.lib.check(keys_fn(mem.ptr(ad), D, r1 - r0, r1 - r0, None if od is None else mem.ptr(od), host.TRANSFORMS[transform],
                              mem.ptr(dd), n, mem.ptr(kd), mem.ptr(cd), mem.stream_ptr), "pgb_rank_keys")
    wd = mem.empty((int(ws_query(D, n, G)) // 8,), np.float64)
    thr = np.ascontiguousarray(thr, np.float64)
    out, counts = np.empty((D, G, 2 + 2 * thr.size), np.int64), (C.c_int64 * 2)()
    hip.lib.check(metrics_fn(mem.ptr(kd), mem.ptr(wd), D, n, seg_off.ctypes.data, G, thr.ctypes.data if thr.size else None, thr.size,
                             mem.ptr(cd), out.ctypes.data, counts, mem.stream_ptr), "pgb_rank_metrics")
    assert list(counts) == [0, 0]
    return out


def test_draws_split_three_and_four_equal_seven_and_permuted_rows_change_nothing(hip):
    rng = np.random.default_rng(2200)
    n, G, thr = 333, 3, (0.25, 0.5, 0.75)
    v = np.round(rng.normal(size=(7, n)), 1)
    cls, gid = rng.integers(0, 2, n), rng.integers(0, G, n)
    off = rng.normal(0, 0.2, n)
    whole = _through_both(hip, v, cls, gid, G, thr, "logistic", off)
    want, n_nan = host.reference_scores(host.value(v, "logistic", off), cls, gid, G, thr)
    assert n_nan == 0 and np.array_equal(whole, want)
    assert np.array_equal(whole, host.numpy_counts(host.value(v, "logistic", off), cls, gid, G, thr))
    parts = [_through_both(hip, v[:3], cls, gid, G, thr, "logistic", off), _through_both(hip, v[3:], cls, gid, G, thr, "logistic", off)]
    assert np.array_equal(np.concatenate(parts), whole)
    perm = rng.permutation(n)
    assert np.array_equal(_through_both(hip, v[:, perm], cls[perm], gid[perm], G, thr, "logistic", off[perm], rows=130), whole)


def test_every_refusal_leaves_every_buffer_untouched(hip):
    rng = np.random.default_rng(2300)
    a, dest = rng.normal(size=(2, 70)), np.arange(70)
    cases = [
        (dict(a=None), "a_dev is null"), (dict(dest=None), "dest_dev is null"), (dict(keys=None), "keys_dev is null"),
        (dict(cnt=None), "counters_dev is null"), (dict(D=0), "D must be >= 1"), (dict(nb=0), "nb must be >= 1"),
        (dict(nb=-5), "nb must be >= 1"), (dict(n=1, nb=1), "n must be >= 2"), (dict(n=69), "nb must be <= n"),
        (dict(ld=69), "ld must be >= nb"), (dict(ld=(1 << 40) + 1), "ld overflows"), (dict(transform=4), "transform is not one of"),
        (dict(transform=-1), "transform is not one of"), (dict(n=1 << 31), "D x n must be < 2^31"), (dict(n=1 << 30), "D x n must be < 2^31"),
    ]
    for change, msg in cases:
        rc, got, cnt, guards = _keys(hip, a, dest, 77, "probit", rng.normal(0, 0.1, 70), counters=(5, 6), change=change)
        text = hip.lib.lib.pgb_last_error().decode()
        assert rc == E_INVALID and msg in text and text.startswith("pgb_rank_keys: "), (change, rc, text)
        assert guards and np.all(got == np.uint64(KEY_GUARD)) and cnt.tolist() == [5, 6], change

    v = rng.normal(size=(2, 40))
    keys, _ = host.keys_block(v, "identity", np.arange(40), 40)
    seg_off, thr = np.array([0, 10, 20, 25, 40], np.int64), np.array([0.5, 0.1])
    keep = {"late": np.array([1, 10, 20, 25, 40], np.int64), "short": np.array([0, 10, 20, 25, 39], np.int64),
            "empty": np.array([0, 10, 10, 25, 40], np.int64), "back": np.array([0, 20, 10, 25, 40], np.int64),
            "pairs": np.array([0, 1 << 26, 1 << 27], np.int64), "thr_nan": np.array([0.5, np.nan]), "long": np.zeros(600, np.int64)}
    p = lambda name: keep[name].ctypes.data  # noqa: E731
    cases = [
        (dict(keys=None), "keys_dev is null"), (dict(ws=None), "ws_dev is null"), (dict(cnt=None), "counters_dev is null"),
        (dict(out=None), "out_host is null"), (dict(counts=None), "counts_host is null"), (dict(seg_off=None), "seg_off_host is null"),
        (dict(thr=None), "thr_host is null"), (dict(D=0), "D must be >= 1"), (dict(n=1), "n must be >= 2"),
        (dict(G=0), "G must be in [1, PGB_RANK_MAX_GROUPS = 256]"), (dict(G=257, seg_off=p("long")), "G must be in [1, PGB_RANK_MAX_GROUPS = 256]"),
        (dict(T=-1), "T must be in [0, PGB_RANK_MAX_THRESHOLDS = 64]"), (dict(T=65), "T must be in [0, PGB_RANK_MAX_THRESHOLDS = 64]"),
        (dict(D=1 << 27), "D x n must be < 2^31"), (dict(n=1 << 31), "D x n must be < 2^31"),
        (dict(seg_off=p("late")), "seg_off_host must start at 0 and end at n"), (dict(seg_off=p("short")), "must start at 0 and end at n"),
        (dict(seg_off=p("empty")), "segment 1 is empty or out of order"), (dict(seg_off=p("back")), "segment 1 is empty or out of order"),
        (dict(seg_off=p("pairs"), G=1, n=1 << 27, D=1), "n1 x n0 of group 0 must be < 2^52"),
        (dict(thr=p("thr_nan")), "thr_host[1] is a NaN"),
    ]
    for change, msg in cases:
        rc, out, counts, guards, got_k, got_w = _metrics(hip, keys, seg_off, thr, counters=(0, 0), change=change)
        text = hip.lib.lib.pgb_last_error().decode()
        assert rc == E_INVALID and msg in text and text.startswith("pgb_rank_metrics: "), (change, rc, text)
        assert guards and np.all(out == INT_GUARD) and np.all(counts == INT_GUARD), change
        assert np.array_equal(got_k, keys.ravel()) and np.all(got_w == np.uint64(KEY_GUARD)), change
    # keys whose dest was out of range: refused after the counters alone are reported
    rc, out, counts, guards, got_k, got_w = _metrics(hip, keys, seg_off, thr, counters=(1, 3))
    text = hip.lib.lib.pgb_last_error().decode()
    assert rc == E_INVALID and "3 keys had a dest outside [0, n)" in text and counts.tolist() == [1, 3]
    assert guards and np.all(out == INT_GUARD) and np.array_equal(got_k, keys.ravel()) and np.all(got_w == np.uint64(KEY_GUARD))
    assert int(hip.lib.rank_entry_points()[1](0, 40, 2)) == 0 and int(hip.lib.rank_entry_points()[1](2, 40, 257)) == 0
    assert int(hip.lib.rank_entry_points()[1](1 << 20, 1 << 20, 1)) == 0


# ------------------------------------------------------------------ end to end
N_ROWS, M_FIT = 300, 10


@pytest.fixture(scope="module")
def fit(hip):
    """Two chains of 8 draws (probit, m = 10) on 300 rows of three covariates."""
    rng = np.random.default_rng(81)
    X = rng.normal(size=(N_ROWS, 3))
    y = (rng.random(N_ROWS) < np.where(X[:, 0] > 0, 0.85, 0.15)).astype(np.float64)
    op = BARTOp(X, y, m=M_FIT)
    attach_history(op, [sample_chain(op, 30, 8, random_seed=5, chain=c, backend=hip, keep_draws=False, batch=(1.0, 1.0),
                                     likelihood=BernoulliLikelihood("probit")) for c in (0, 1)])
    return X, y, np.where(X[:, 1] > 0.3, "right", "left"), _get_posterior_sampler(op, backend=hip)


def _same(got, want, draws=slice(None)):
    for key in ("U2", "KSN", "tp", "fp", "auc", "ks", "tpr", "fpr", "precision"):
        assert np.array_equal(got[key], want[key][draws], equal_nan=True), key
    assert got["group_labels"].tolist() == want["group_labels"].tolist()


def test_discrimination_end_to_end_against_the_matrix_route_and_under_the_smallest_blocks(hip, fit, monkeypatch):
    """A device-resident ``X`` (``resident_rows``) is REFUSED by name, not served: the row blocks of a chunk of draws
    upload their rows of ``X`` from the host, and a second path would have to slice a device matrix per chunk."""
    X, y, groups, s = fit
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    thr = (0.2, 0.5, 0.8)
    off = np.random.default_rng(82).normal(0, 0.2, N_ROWS)
    kw = dict(groups=groups, thresholds=thr, transform="probit", offset=off)
    whole = discrimination(s, X, y, **kw)
    assert whole["n_draws"] == 16 and whole["n_chunks"] == 1 and whole["auc"].shape == (16, 2) and whole["tp"].shape == (16, 2, 3)
    assert whole["auc_hdi"].shape == (2, 2) and whole["group_labels"].tolist() == ["left", "right"]
    f = np.asarray(s.sample_posterior(X, list(range(16)), None))[:, 0, :]
    v = host.value(f, "probit", off)
    _same(discrimination_matrix(v, y, groups, thr), whole)
    gid = (groups == "right").astype(np.int32)
    want = host.numpy_counts(v, y.astype(np.int32), gid, 2, thr)                          # ... and the definition itself
    assert np.array_equal(whole["U2"], want[:, :, 0]) and np.array_equal(whole["KSN"], want[:, :, 1])
    assert np.array_equal(whole["tp"], want[:, :, 2:5]) and np.array_equal(whole["fp"], want[:, :, 5:8])
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")                                     # the floor: several chunks, blocks of 64 rows
    cut = discrimination(s, X, y, **kw)
    assert cut["n_chunks"] > 1
    _same(cut, whole)
    _same(discrimination_matrix(v, y, groups, thr), whole)
    draws = [9, 1, 15, 6]
    _same(discrimination(s, X, y, draws=draws, **kw), whole, draws)
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES")
    with pytest.raises(ValueError, match="device-resident X"):
        discrimination(s, hip.mem.from_host(X), y, **kw)
    print("auc_mean (left, right):", whole["auc_mean"], "ks_mean:", whole["ks_mean"])
    assert np.all(whole["auc_mean"] > 0.7)                                                # the one sanity check: the classes separate
    keys_ms = hip.lib.rank_kernel_ms()
    assert len(keys_ms) == 3
