"""Per-row posterior summaries on the MI355X: ``k_rowsum`` through ``pgb_row_summary`` against the host build of the
same header (``tests/_rowsummary_host.py``) -- bit for bit, on synthetic matrices at every tile regime of the kernel,
for every argument variant, and end to end on short real chains -- and the refusals.

"Bit for bit" is the 64-bit pattern of every output that is a number.  Where an output is a NaN on both sides (inf -
inf in the variance after a column of 1e300s overflowed the sum of squares) it counts as equal: the sign and payload
of a NaN an operation GENERATES are the hardware's, not the contract's."""
import numpy as np
import pytest

import _rowsummary_host as host
from pymc_bart_amd import (BARTOp, CategoricalLikelihood, _abi, partial_dependence, posterior_summary, summarize_matrix)
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler

pytestmark = pytest.mark.gpu

SMALL_D = (2, 3, 63, 64, 65, 127, 128, 129)
# the kernel keeps 16384 keys per workgroup: 8 columns up to Dp = 2048, then 4, 2 and 1 -- the last D of every regime
# and the first of the next, and the cap
LARGE_D = (2048, 2049, 4096, 4097, 8192, 8193, 16384)
KINDS = ("constant", "ascending", "descending", "zeros", "half tied", "magnitudes", "normal")
Q16 = np.array([0.0, 1.0, 0.5, 0.25, 0.03, 0.97, 0.123, 0.75, 0.9, 0.1, 1e-9, 1.0 - 1e-9, 0.3333333333333333, 0.6, 0.05, 0.95])


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)


def column(kind: str, D: int, rng) -> np.ndarray:
    if kind == "constant":
        return np.full(D, float(rng.choice([0.1, -3.0, 1e300, -1e-300, 0.0])))
    if kind == "ascending":
        return np.sort(rng.normal(0, 1, D))
    if kind == "descending":
        return np.sort(rng.normal(0, 1, D))[::-1].copy()
    if kind == "zeros":
        return rng.choice([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], D)
    if kind == "half tied":
        x = rng.normal(0, 1, D)
        x[rng.permutation(D)[:D // 2]] = 0.25
        return x
    if kind == "magnitudes":
        return rng.choice([-1.0, 1.0], D) * 10.0 ** rng.uniform(-300.0, 300.0, D)
    return rng.normal(0, 1, D)


def matrix(D: int, n_cols: int, ld: int, shift: int, seed: int) -> np.ndarray:
    """(D, ld): column c is of kind (c + shift) mod 7; the columns beyond n_cols hold a value no result may show."""
    rng = np.random.default_rng(seed)
    a = np.full((D, ld), 7.0e77)
    for c in range(n_cols):
        a[:, c] = column(KINDS[(c + shift) % len(KINDS)], D, rng)
    return a


def same(got: np.ndarray, want: np.ndarray) -> bool:
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


def device(hip, a, n_cols, q, k, transform="identity", offset=None, D=None, ld=None):
    """pgb_row_summary on the first n_cols columns of the device copy of a (D, ld) -> (rc, out (rows, n_cols), guard)."""
    mem, lib = hip.mem, hip.lib
    q = np.ascontiguousarray(q, np.float64)
    rows = 2 + q.size + 2
    md = mem.from_host(np.ascontiguousarray(a))
    od = mem.from_host(np.full(rows * n_cols + 8, -7.0))
    offd = None if offset is None else mem.from_host(np.ascontiguousarray(offset, np.float64))
    code = transform if isinstance(transform, int) else host.TRANSFORMS[transform]
    rc = lib.rowsummary_entry_point()(mem.ptr(md), a.shape[0] if D is None else D, n_cols, a.shape[1] if ld is None else ld,
                                      None if offd is None else mem.ptr(offd), code, q.ctypes.data if q.size else None,
                                      int(q.size), int(k), mem.ptr(od), mem.stream_ptr)
    out = mem.to_host(od)
    return rc, out[:rows * n_cols].reshape(rows, n_cols), out[rows * n_cols:]


def check(hip, a, n_cols, q, k, transform="identity", offset=None, what=None):
    rc, out, guard = device(hip, a, n_cols, q, k, transform, offset)
    assert rc == 0, what
    want = host.summary(a[:, :n_cols], q, k, transform, offset)
    bad = [r for r in range(out.shape[0]) if not same(out[r], want[r])]
    assert not bad, (what, "output rows that differ", bad)
    assert np.all(guard == -7.0), what                       # nothing written beyond [rows][n_cols]


# ------------------------------------------------------------------ 1. every shape, every kind of input
@pytest.mark.parametrize("D", SMALL_D + LARGE_D)
def test_device_equals_the_host_header_at_every_shape(D, hip):
    q = np.array([0.0, 0.03, 0.5, 0.97, 1.0])
    k = host.hdi_k(D, 0.94)
    for n_cols in (1, 7, 8, 9) + ((67,) if D <= 129 else ()):
        for ld in (n_cols, n_cols + 5):
            for shift in (range(len(KINDS)) if n_cols < len(KINDS) else (0,)):   # (every kind at every shape)
                a = matrix(D, n_cols, ld, shift, seed=D * 100 + n_cols)
                check(hip, a, n_cols, q, k, what=(D, n_cols, ld, shift))


# ------------------------------------------------------------------ 2. every argument variant
@pytest.mark.parametrize("D", [3, 65, 129, 2049, 4097])
def test_device_equals_the_host_header_for_every_argument_variant(D, hip):
    n_cols, ld = 9, 14
    a = matrix(D, n_cols, ld, 0, seed=D)
    a[:, 5] = np.random.default_rng(D).uniform(-30.0, 30.0, D)       # (where the transforms are not saturated)
    a[:, 6] = np.random.default_rng(D + 1).normal(0.0, 2.0, D)
    off = np.random.default_rng(D + 2).normal(0.0, 3.0, n_cols)
    for transform in host.TRANSFORMS:
        for offset in (None, off):
            for q in (np.array([]), Q16):
                for k in (0, 1, D - 1, D):
                    check(hip, a, n_cols, q, k, transform, offset, what=(D, transform, offset is not None, q.size, k))


def test_permuting_the_draws_changes_no_bit_on_the_device(hip):
    rng = np.random.default_rng(11)
    for D in (129, 2049):
        a = matrix(D, 9, 9, 0, seed=3 * D)
        _, one, _ = device(hip, a, 9, Q16, host.hdi_k(D, 0.9), "logistic")
        _, two, _ = device(hip, a[rng.permutation(D)], 9, Q16, host.hdi_k(D, 0.9), "logistic")
        assert same(one, two)


# ------------------------------------------------------------------ 3. refusals
def test_refusals_before_any_launch(hip):
    a = np.zeros((50, 16))
    q = np.array([0.5])
    for D, n, ld, code, qq, k, msg in ((1, 16, 16, 0, q, 1, "at least 2 draws"),
                                       (host.max_draws() + 1, 16, 16, 0, q, 1, "at most"),
                                       (50, 16, 15, 0, q, 1, "ld >= n_cols"), (50, 0, 16, 0, q, 1, "n_cols must be >= 1"),
                                       (50, 16, 16, 0, np.full(17, 0.5), 1, "n_q must be in"),
                                       (50, 16, 16, 0, np.array([1.5]), 1, "quantile 0 must be in"),
                                       (50, 16, 16, 0, np.array([0.5, -0.1]), 1, "quantile 1 must be in"),
                                       (50, 16, 16, 0, np.array([np.nan]), 1, "quantile 0 must be in"),
                                       (50, 16, 16, 0, np.array([np.inf]), 1, "quantile 0 must be in"),
                                       (50, 16, 16, 0, q, -1, "hdi_k must be >= 0"), (50, 16, 16, 4, q, 1, "unknown transform"),
                                       (50, 16, 16, -1, q, 1, "unknown transform")):
        mem, lib = hip.mem, hip.lib
        md = mem.from_host(a)
        od = mem.from_host(np.full(21 * 16, -7.0))
        rc = lib.rowsummary_entry_point()(mem.ptr(md), D, n, ld, None, code, qq.ctypes.data, int(qq.size), k, mem.ptr(od),
                                          mem.stream_ptr)
        assert rc == -1, (D, n, ld, code, k)                  # PGB_E_INVALID
        with pytest.raises(_abi.PGBError, match=msg):
            lib.check(rc, "pgb_row_summary")
        assert np.all(mem.to_host(od) == -7.0)


# ------------------------------------------------------------------ 4. end to end
N, P, M_TREES = 300, 4, 10


def _data(seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, P))
    f = 2.0 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 1.5 * (X[:, 2] - 0.5) + X[:, 3]
    return rng, X, f


@pytest.fixture(scope="module")
def normal_fit(hip):
    """Two chains of a Normal fit behind one sampler: 2 x 24 pooled draws."""
    rng, X, f = _data(41)
    y = f + rng.normal(0, 0.5, N)
    op = BARTOp(X, y, m=M_TREES)
    chains = [sample_chain(op, 8, 24, random_seed=2, chain=c, backend=hip, keep_draws=False) for c in (0, 1)]
    attach_history(op, chains)
    return op, X, _get_posterior_sampler(op, backend=hip)


@pytest.fixture(scope="module")
def categorical_fit(hip):
    rng, X, f = _data(42)
    y = np.minimum((f + rng.normal(0, 0.5, N)).clip(0) // 1.2, 2.0)
    op = BARTOp(X, y, m=M_TREES)
    res = sample_chain(op, 8, 30, num_particles=10, random_seed=3, chain=0, backend=hip, keep_draws=False,
                       likelihood=CategoricalLikelihood(3))
    base, batches = res["history"]
    return X, PosteriorSampler.from_history(batches, base, M_TREES, 3, backend=hip)


def _expect(res, pred, quantiles, hdi_prob, transform="identity", offset=None):
    """``res`` == the host header on the predictions ``pred`` (D, K, n) of the same draws."""
    D, K, n = pred.shape
    want = host.public(pred.reshape(D, K * n), quantiles, hdi_prob, transform,
                       None if offset is None else np.asarray(offset, np.float64).reshape(K * n))
    assert res["n_draws"] == D and np.array_equal(res["q"], np.asarray(quantiles, np.float64))
    for key in ("mean", "var", "sd"):
        assert res[key].shape == (n, K) and same(res[key], want[key].reshape(K, n).T), key
    Q = len(quantiles)
    assert res["quantiles"].shape == (Q, n, K)
    assert same(res["quantiles"], np.moveaxis(want["quantiles"].reshape(Q, K, n), 1, 2))
    if hdi_prob is None:
        assert res["hdi"] is None and res["hdi_prob"] is None
    else:
        assert res["hdi"].shape == (2, n, K) and same(res["hdi"], np.moveaxis(want["hdi"].reshape(2, K, n), 1, 2))


def test_posterior_summary_of_two_pooled_chains(normal_fit, hip, monkeypatch):
    op, X, sampler = normal_fit
    assert sampler.n_draws == 48
    everything = list(range(48))
    pred = sampler.sample_posterior(X, everything, None)
    res = posterior_summary(sampler, X)
    _expect(res, pred, (0.03, 0.5, 0.97), 0.94)
    assert res["hdi_prob"] == 0.94 and np.all(res["hdi"][0] <= res["mean"]) and np.all(res["mean"] <= res["hdi"][1])
    excl = posterior_summary(sampler, X, excluded=[1, 3], quantiles=[0.1, 0.9], hdi_prob=0.5)
    _expect(excl, sampler.sample_posterior(X, everything, [1, 3]), [0.1, 0.9], 0.5)
    assert not np.array_equal(excl["mean"], res["mean"])
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(1 << 16))               # blocks of 64 rows: five of them
    for kw in ({}, {"excluded": [1, 3], "quantiles": [0.1, 0.9], "hdi_prob": 0.5}):
        again, first = posterior_summary(sampler, X, **kw), (excl if kw else res)
        for key in ("mean", "var", "sd", "quantiles", "hdi"):
            assert same(again[key], first[key]), (key, kw)
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES")
    # a subset of the draws with a repeat, an offset and a transform, no interval
    idx = [3, 3] + list(range(5, 47, 2))
    off = np.random.default_rng(5).normal(0, 1, N)
    sub = posterior_summary(sampler, X, draws=idx, quantiles=[], hdi_prob=None, transform="logistic", offset=off)
    _expect(sub, sampler.sample_posterior(X, idx, None), [], None, "logistic", off[None, :])
    # held-out rows, one column of them (a vector is one covariate ... here: fewer rows than a block)
    X2 = np.random.default_rng(6).uniform(0, 1, (77, P))
    _expect(posterior_summary(sampler, X2, transform="exp"), sampler.sample_posterior(X2, everything, None),
            (0.03, 0.5, 0.97), 0.94, "exp")


def test_posterior_summary_of_a_categorical_fit(categorical_fit, monkeypatch):
    X, ps = categorical_fit
    everything = list(range(ps.n_draws))
    pred = ps.sample_posterior(X, everything, None)
    assert pred.shape == (30, 3, N)
    res = posterior_summary(ps, X)
    _expect(res, pred, (0.03, 0.5, 0.97), 0.94)
    off = np.random.default_rng(7).normal(0, 1, (3, N))
    _expect(posterior_summary(ps, X, excluded=[1, 3], transform="probit", offset=off),
            ps.sample_posterior(X, everything, [1, 3]), (0.03, 0.5, 0.97), 0.94, "probit", off)
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(1 << 16))
    again = posterior_summary(ps, X)
    for key in ("mean", "var", "quantiles", "hdi"):
        assert same(again[key], res[key]), key


def test_partial_dependence_with_a_summary(normal_fit, hip):
    op, X, sampler = normal_fit
    kw = dict(xs_interval="linear", xs_values=11, samples=40, random_seed=9, backend=hip)
    plain = partial_dependence(op, X, **kw)
    spec = {"quantiles": [0.05, 0.5, 0.95], "hdi_prob": 0.9}
    got = partial_dependence(op, X, summary=spec, **kw)
    assert sorted(got) == ["labels", "pd", "reference", "summary", "x"] and set(got["summary"]) == set(range(P))
    assert got["reference"] == plain["reference"]
    for j in range(P):
        pd_j = got["pd"][j]
        assert pd_j.shape == (40, 11, 1) and np.array_equal(pd_j, plain["pd"][j]), j    # the same picks, the same numbers
        _expect(got["summary"][j], np.moveaxis(pd_j, 1, 2), [0.05, 0.5, 0.95], 0.9)
    logit = partial_dependence(op, X, var_idx=[2], summary={"transform": "logistic"}, **kw)
    _expect(logit["summary"][2], np.moveaxis(logit["pd"][2], 1, 2), (0.03, 0.5, 0.97), 0.94, "logistic")
    assert np.array_equal(logit["pd"][2], partial_dependence(op, X, var_idx=[2], **kw)["pd"][2])


def test_summarize_matrix(hip, monkeypatch):
    a = matrix(403, 300, 300, 0, seed=17)
    res = summarize_matrix(a, backend=hip)
    want = host.public(a, (0.03, 0.5, 0.97), 0.94)
    for key in ("mean", "var", "sd", "quantiles", "hdi"):
        assert res[key].shape == want[key].shape and same(res[key], want[key]), key
    assert res["n_draws"] == 403 and res["hdi_prob"] == 0.94
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(8 * (403 + 7) * 64))   # blocks of 64 columns: five of them
    again = summarize_matrix(a, backend=hip)
    for key in ("mean", "var", "quantiles", "hdi"):
        assert same(again[key], res[key]), key
    ex = summarize_matrix(a[:, :9], quantiles=None, hdi_prob=None, transform="exp", backend=hip)
    want = host.public(a[:, :9], None, None, "exp")
    assert ex["hdi"] is None and ex["quantiles"].shape == (0, 9) and same(ex["mean"], want["mean"]) and same(ex["var"], want["var"])
