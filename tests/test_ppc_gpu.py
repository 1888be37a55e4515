"""Replicated observations on the MI355X: ``k_ppc`` through ``pgb_ppc_draw`` against the host build of the same header
(``tests/_ppc_host.py``) -- bit for bit, on uploaded matrices for every family across the chunk and workgroup edges,
in place and out of place, the PIT counts, the refusals -- and end to end on short real chains.

"Bit for bit" is the 64-bit pattern of every value, as in ``test_rowsummary_gpu.same``."""
import ctypes as C

import numpy as np
import pytest

import _ppc_host as host
import _rowsummary_host as rowsum
from pymc_bart_amd import (BARTOp, CategoricalLikelihood, NormalLikelihood, _abi, posterior_predictive, predictive_pit,
                           predictive_summary)
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.pointwise import _chains
from pymc_bart_amd.trees import PosteriorSampler, pooled_history
from pymc_bart_amd.utils import _get_posterior_sampler
from test_rowsummary_gpu import same

pytestmark = pytest.mark.gpu

SENTINEL = 7.0e77
PIT_SENTINEL = -77
ROW0 = (0, (1 << 32) + 5)
# family -> (K, the params of draw d).  The params vary per draw; the predictors below reach both Poisson samplers
CASES = {
    "normal": (1, lambda d: [0.3 + 0.01 * d]),
    "normal_meanscale": (2, lambda d: []),
    "bernoulli_probit": (1, lambda d: []),
    "bernoulli_logit": (1, lambda d: []),
    "categorical": (3, lambda d: []),
    "categorical16": (16, lambda d: []),
    "asymmetric_laplace": (1, lambda d: [0.5 + 0.02 * d, 0.1 + 0.8 * ((d * 7) % 10) / 10.0]),
    "gamma_log": (1, lambda d: [0.05 + 0.37 * (d % 9)]),
    "student_t": (1, lambda d: [0.5 + 0.01 * d, 1.5 + 0.5 * (d % 12)]),
    "poisson_log": (1, lambda d: []),
    "negbin_log": (1, lambda d: [0.3 + 0.4 * (d % 8)]),
}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)


def inputs(case: str, D: int, n: int, seed: int):
    """-> (family, mu (D, K, n), params (D, n_params), offset (K, n))."""
    K, par = CASES[case]
    rng = np.random.default_rng(seed)
    mu = rng.normal(1.0, 1.5, (D, K, n))                     # rates from 0.01 to 1000: inversion and PTRS
    params = np.array([par(d) for d in range(D)], np.float64).reshape(D, -1)
    return case.rstrip("0123456789"), mu, params, rng.normal(0.0, 0.5, (K, n))


def device(hip, family, mu, params, n, row0=0, seed=5, offset=None, y=None, out="apart", D=None, K=None, ld=None,
           ld_out=None, n_params=None):
    """pgb_ppc_draw on the device copy of ``mu`` (D, K, ld) -> (rc, out (D, ld_out) or None, pit (2 n + 8,) or None,
    flags, the device copy of mu afterwards)."""
    mem, lib = hip.mem, hip.lib
    DD, KK, LD = mu.shape
    md = mem.from_host(np.ascontiguousarray(mu))
    lik = _abi.PpcLik()
    lik.family = family if isinstance(family, int) else host.FAMILIES[family]
    lik.n_params = params.shape[1] if n_params is None else n_params
    par = np.ascontiguousarray(params, np.float64)
    lik.params_host = par.ctypes.data if par.size else None
    offd = None if offset is None else mem.from_host(np.ascontiguousarray(offset))
    lik.offset_dev = None if offd is None else mem.ptr(offd)
    lo = LD if ld_out is None else ld_out
    outd = {"apart": lambda: mem.from_host(np.full((DD, lo), SENTINEL)), "in place": lambda: md, None: lambda: None}[out]()
    yd = None if y is None else mem.from_host(np.ascontiguousarray(y, np.float64))
    pd = None if y is None else mem.from_host(np.concatenate([np.zeros(2 * n, np.int32), np.full(8, PIT_SENTINEL, np.int32)]))
    flags = (C.c_int64 * 2)(-1, -1)
    rc = lib.ppc_entry_point()(mem.ptr(md), DD if D is None else D, KK if K is None else K, n, LD if ld is None else ld, row0,
                               C.byref(lik), seed, None if outd is None else mem.ptr(outd), lo,
                               None if yd is None else mem.ptr(yd), None if pd is None else mem.ptr(pd), flags, mem.stream_ptr)
    return (rc, None if out != "apart" else mem.to_host(outd).reshape(DD, -1), None if pd is None else mem.to_host(pd),
            (int(flags[0]), int(flags[1])), mem.to_host(md).reshape(mu.shape))


def padded(a: np.ndarray, pad: int = 5) -> np.ndarray:
    """The last axis widened by ``pad`` sentinels: a leading dimension of n + pad."""
    out = np.full(a.shape[:-1] + (a.shape[-1] + pad,), SENTINEL)
    out[..., :a.shape[-1]] = a
    return out


# ------------------------------------------------------------------ 1. every family, every edge
@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_the_host_header(case, hip):
    shapes = [(D, 65) for D in (1, 2, 31, 32, 33, 65)] + [(33, n) for n in (1, 63, 64, 257)]
    for j, (D, n) in enumerate(shapes):
        family, mu, params, off = inputs(case, D, n, seed=100 * D + n)
        row0 = ROW0[j % 2]
        for offset in (None, off):
            y = np.round(mu[0, 0]) if offset is None else None       # (the counts ride along on half the calls)
            want, wpit, wflags = host.fill(family, mu, params, row0=row0, seed=5, offset=offset, y=y)
            rc, got, pit, flags, mu_after = device(hip, family, padded(mu), params, n, row0, 5,
                                                   None if offset is None else padded(off), y)
            what = (case, D, n, row0, offset is not None)
            assert rc == 0, what
            assert same(got[:, :n], want), what
            assert np.all(got[:, n:] == SENTINEL) and same(mu_after, padded(mu)), what   # the padding, the input
            assert flags == wflags, what
            if y is not None:
                assert np.array_equal(pit[:2 * n].reshape(2, n), wpit) and np.all(pit[2 * n:] == PIT_SENTINEL), what


def test_the_caps_are_counted_on_the_device(hip):
    D, n = 3, 70
    mu = np.full((D, 1, n), 25.0)                                       # a rate above 2^30
    want, _, wflags = host.fill("poisson_log", mu, None, seed=2)
    rc, got, _, flags, _ = device(hip, "poisson_log", mu, np.zeros((D, 0)), n, seed=2)
    assert rc == 0 and same(got, want) and flags == wflags == (D * n, 0)
    mu = np.full((D, 1, n), 800.0)                                      # exp(mu) overflows
    par = np.full((D, 1), 2.0)
    want, _, wflags = host.fill("gamma_log", mu, par, seed=2)
    rc, got, _, flags, _ = device(hip, "gamma_log", mu, par, n, seed=2)
    assert rc == 0 and same(got, want) and flags == wflags == (D * n, 0)


# ------------------------------------------------------------------ 2. in place, refusals
@pytest.mark.parametrize("case", ["normal", "negbin_log"])
def test_in_place_gives_the_same_bits(case, hip):
    D, n = 65, 257
    family, mu, params, off = inputs(case, D, n, seed=8)
    rc, apart, _, flags, _ = device(hip, family, padded(mu), params, n, 9, 5, padded(off))
    rc2, _, _, flags2, inplace = device(hip, family, padded(mu), params, n, 9, 5, padded(off), out="in place")
    assert rc == 0 and rc2 == 0 and flags == flags2
    assert same(inplace[:, 0, :n], apart[:, :n]) and np.all(inplace[:, 0, n:] == SENTINEL)


def _refused(hip, msg, family, mu, params, n, **kw):
    rc, out, pit, flags, mu_after = device(hip, family, mu, params, n, **kw)
    assert rc == -1, msg                                                 # PGB_E_INVALID
    with pytest.raises(_abi.PGBError, match=msg):
        hip.lib.check(rc, "pgb_ppc_draw")
    assert out is None or np.all(out == SENTINEL), msg
    assert pit is None or (np.all(pit[:2 * n] == 0) and np.all(pit[2 * n:] == PIT_SENTINEL)), msg
    assert same(mu_after, mu) and flags == (-1, -1), msg


def test_refusals_before_any_launch(hip):
    D, n = 4, 20
    mu = np.zeros((D, 1, n + 5))
    one = np.ones((D, 1))
    none = np.zeros((D, 0))
    _refused(hip, "D must be >= 1", "normal", mu, one, n, D=0)
    _refused(hip, "n_rows must be >= 1", "normal", mu, one, 0)
    _refused(hip, "ld must be >= n_rows", "normal", mu, one, n, ld=n - 1)
    _refused(hip, "ld_out must be >= n_rows", "normal", mu, one, n + 5, ld_out=n)
    _refused(hip, "row0 must be >= 0", "normal", mu, one, n, row0=-1)
    _refused(hip, "the callback family has a log density only", 10, mu, none, n)
    _refused(hip, "the compiled family has a log density only", 11, mu, none, n)
    _refused(hip, "unknown family", 12, mu, none, n)
    _refused(hip, "takes n_params = 1 per draw, 0 given", "normal", mu, none, n)
    _refused(hip, "takes n_params = 0 per draw, 1 given", "poisson_log", mu, one, n)
    _refused(hip, "does not take K = 2", "normal", np.zeros((D, 2, n)), one, n)
    _refused(hip, "does not take K = 1", "normal_meanscale", mu, none, n)
    _refused(hip, "does not take K = 1", "categorical", mu, none, n)
    _refused(hip, "does not take K = 17", "categorical", np.zeros((D, 17, n)), none, n)
    for bad in (0.0, -1.0, np.nan, np.inf):
        _refused(hip, "the params of draw 2 are outside family 0's domain", "normal", mu,
                 np.array([[1.0], [1.0], [bad], [bad]]), n)
    _refused(hip, "the params of draw 1 are outside family 7's domain", "asymmetric_laplace", mu,
             np.array([[1.0, 0.5], [1.0, 1.0], [1.0, 0.5], [1.0, 0.5]]), n)
    _refused(hip, "no output", "normal", mu, one, n, out=None)
    # an overlapping out with K = 2: out_dev == mu_dev is in place only for K == 1
    _refused(hip, "out_dev overlaps mu_dev", "normal_meanscale", np.zeros((D, 2, n)), none, n, out="in place")
    # ... and K = 1 in place with another leading dimension
    _refused(hip, "out_dev overlaps mu_dev", "normal", mu, one, n, out="in place", ld_out=n)
    # null pointers, y without counts
    mem, call = hip.mem, hip.lib.ppc_entry_point()
    md = mem.from_host(mu)
    lik = _abi.PpcLik()
    lik.family, lik.n_params, lik.params_host = 0, 1, one.ctypes.data
    flags = (C.c_int64 * 2)()
    for args, msg in (((None, D, 1, n, n + 5, 0, C.byref(lik), 1, mem.ptr(md), n + 5, None, None, flags), "mu_dev is null"),
                      ((mem.ptr(md), D, 1, n, n + 5, 0, None, 1, mem.ptr(md), n + 5, None, None, flags), "lik is null"),
                      ((mem.ptr(md), D, 1, n, n + 5, 0, C.byref(lik), 1, mem.ptr(md), n + 5, None, None, None), "flags_host is null"),
                      ((mem.ptr(md), D, 1, n, n + 5, 0, C.byref(lik), 1, mem.ptr(md), n + 5, mem.ptr(md), None, flags),
                       "y_dev and pit_counts_dev come together")):
        rc = call(*args, mem.stream_ptr)
        assert rc == -1, msg
        with pytest.raises(_abi.PGBError, match=msg):
            hip.lib.check(rc, "pgb_ppc_draw")
    lik.params_host = None
    rc = call(mem.ptr(md), D, 1, n, n + 5, 0, C.byref(lik), 1, mem.ptr(md), n + 5, None, None, flags, mem.stream_ptr)
    with pytest.raises(_abi.PGBError, match="params_host is null"):
        hip.lib.check(rc, "pgb_ppc_draw")
    assert np.all(mem.to_host(md) == 0.0)


# ------------------------------------------------------------------ 3. PIT counts: several chunks add into one row
@pytest.mark.parametrize("case", ["poisson_log", "student_t", "categorical"])
def test_pit_counts_without_a_matrix(case, hip):
    D, n = 65, 257
    family, mu, params, off = inputs(case, D, n, seed=3)
    yrep, _, _ = host.fill(family, mu, params, row0=ROW0[1], seed=6, offset=off)
    rng = np.random.default_rng(4)
    y = yrep[rng.integers(0, D, n), np.arange(n)] if case != "student_t" else rng.normal(1.0, 2.0, n)
    _, wpit, wflags = host.fill(family, mu, params, row0=ROW0[1], seed=6, offset=off, y=y, values=False)
    assert np.array_equal(wpit[0], (yrep < y).sum(0)) and np.array_equal(wpit[1], (yrep == y).sum(0))
    rc, out, pit, flags, _ = device(hip, family, padded(mu), params, n, ROW0[1], 6, padded(off), y, out=None)
    assert rc == 0 and out is None and flags == wflags
    assert np.array_equal(pit[:2 * n].reshape(2, n), wpit) and np.all(pit[2 * n:] == PIT_SENTINEL)


# ------------------------------------------------------------------ 4. end to end
N, P, M_TREES, TUNE, DRAWS = 200, 4, 10, 20, 20


def _data(seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, P))
    f = 2.0 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 1.5 * (X[:, 2] - 0.5) + X[:, 3]
    return rng, X, f


class Pooled:
    """Several chains behind one object, as the multi-chain sampler presents them."""

    def __init__(self, parts):
        self._chain_samplers = parts

    def sample_posterior(self, X, idx, excluded=None):
        assert idx is None
        return np.concatenate([p.sample_posterior(X, list(range(p.n_draws)), excluded) for p in self._chain_samplers])


@pytest.fixture(scope="module")
def normal_fit(hip):
    """Two chains of a Normal fit behind one sampler: 2 x 20 pooled draws, sigma per draw."""
    rng, X, f = _data(41)
    y = f + rng.normal(0, 0.5, N)
    op = BARTOp(X, y, m=M_TREES)
    chains = [sample_chain(op, TUNE, DRAWS, random_seed=2, chain=c, backend=hip, keep_draws=False) for c in (0, 1)]
    attach_history(op, chains)
    multi = _get_posterior_sampler(op, backend=hip)
    sigma = np.concatenate([c["sigma"] for c in chains])
    pred = multi.sample_posterior(X, list(range(2 * DRAWS)), None)
    return X, y, multi, NormalLikelihood("sigma"), {"sigma": sigma}, sigma[:, None], pred


@pytest.fixture(scope="module")
def categorical_fit(hip):
    """Two chains of a K = 3 softmax fit."""
    rng, X, f = _data(42)
    y = np.minimum((f + rng.normal(0, 0.5, N)).clip(0) // 1.2, 2.0)
    op = BARTOp(X, y, m=M_TREES)
    parts = []
    for c in (0, 1):
        res = sample_chain(op, TUNE, DRAWS, num_particles=10, random_seed=3, chain=c, backend=hip, keep_draws=False,
                           likelihood=CategoricalLikelihood(3))
        base, batches = res["history"]
        parts.append(PosteriorSampler.from_history(batches, base, M_TREES, 3, backend=hip))
    multi = Pooled(parts)
    return X, y, multi, CategoricalLikelihood(3), None, None, multi.sample_posterior(X, None)


def _everything(sampler, X, y, lik, points, **kw):
    yrep, info = posterior_predictive(sampler, X, lik, points=points, return_info=True, **kw)
    return yrep, info, predictive_summary(sampler, X, lik, points=points, **kw), predictive_pit(sampler, X, y, lik, points=points, **kw)


def _equal(a, b):
    (ya, ia, sa, pa), (yb, ib, sb, pb) = a, b
    assert same(ya, yb) and ia == ib
    for key in ("mean", "var", "sd", "quantiles", "hdi"):
        assert same(sa[key], sb[key]), key
    for key in ("pit", "n_below", "n_equal"):
        assert np.array_equal(pa[key], pb[key]), key
    for key in ("n_draws", "n_capped", "n_exhausted"):
        assert sa[key] == sb[key] and pa[key] == pb[key], key


@pytest.mark.parametrize("which", ["normal", "categorical"])
def test_end_to_end(which, request, hip, monkeypatch):
    X, y, multi, lik, points, params, pred = request.getfixturevalue(which + "_fit")
    D, K, n = pred.shape
    assert (D, n) == (2 * DRAWS, N) and K == (1 if which == "normal" else 3)
    off = np.random.default_rng(5).normal(0, 0.3, (K, N))
    for kw in ({"random_seed": 7}, {"random_seed": 8, "offset": off}):
        got = _everything(multi, X, y, lik, points, **kw)
        yrep, info, summ, pit = got
        want, _, wflags = host.fill(lik.family, pred, params, seed=kw["random_seed"], offset=kw.get("offset"))
        assert yrep.shape == (D, n) and same(yrep, want)
        assert info == {"n_capped": wflags[0], "n_exhausted": wflags[1]} == {"n_capped": 0, "n_exhausted": 0}
        ref = rowsum.public(want, (0.03, 0.5, 0.97), 0.94)
        for key in ("mean", "var", "sd", "quantiles", "hdi"):
            assert summ[key].shape == ref[key].shape and same(summ[key], ref[key]), key
        assert summ["n_draws"] == D and summ["n_capped"] == 0 and summ["n_exhausted"] == 0
        assert np.array_equal(pit["n_below"], (want < y).sum(0)) and np.array_equal(pit["n_equal"], (want == y).sum(0))
        assert np.array_equal(pit["pit"], ((want < y).sum(0) + 0.5 * (want == y).sum(0)) / D) and pit["n_draws"] == D
        monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(1 << 16))               # several blocks of 64 rows
        _equal(_everything(multi, X, y, lik, points, **kw), got)
        monkeypatch.delenv("PGB_PW_BLOCK_BYTES")
        # the chains as one multi-chain sampler, or their pooled draws behind one plain sampler
        pool, table = pooled_history(_chains(multi))
        _equal(_everything(PosteriorSampler(pool, table, M_TREES, K, backend=hip), X, y, lik, points, **kw), got)
    # a subset of the draws: the value belongs to the POSITION in the list
    idx = [DRAWS + 2, 1, 1, DRAWS - 1]
    sub = posterior_predictive(multi, X, lik, points=None if points is None else {"sigma": points["sigma"][idx]},
                               draws=idx, random_seed=7)
    want, _, _ = host.fill(lik.family, pred[idx], None if params is None else params[idx], seed=7)
    assert same(sub, want)
