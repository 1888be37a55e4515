"""PSIS-weighted expectations on the MI355X: ``k_psis_expect`` against the host build of the same header
(``tests/_psis_expect_host.py``) -- bit for bit, both kinds, on synthetic matrices at the kernel's edges, on the edge
cases of the tail and end to end (``loo_pit``, ``loo_predictive``) on short real chains -- and the refusals.

"Bit for bit" is the 64-bit pattern of every value (``test_psis_expect.bits``)."""
import sys
import warnings

import numpy as np
import pytest

import _psis_expect_host as host
import _psis_host as psis_host
from pymc_bart_amd import (BARTOp, BernoulliLikelihood, CategoricalLikelihood, NormalLikelihood, PoissonLikelihood, _abi,
                           loo_pit, loo_predictive, pointwise_log_likelihood, posterior_predictive, psis_expectation_matrix)
from pymc_bart_amd.chains import sample_chain
from pymc_bart_amd.loo import loo
from pymc_bart_amd.trees import PosteriorSampler
from test_psis import _tied
from test_psis_expect import bits, synthetic

pytestmark = pytest.mark.gpu
loo_mod = sys.modules["pymc_bart_amd.loo"]
SENTINEL = -7.0


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.delenv("PGB_PW_WGS", raising=False)
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)       # (rows with a high k are the data's, not the test's)
        return fn(*a, **kw)


def _raw(hip, ll, g, n, M, y=None, kind="value", D=None, ld=None, ldg=None, g_null=False, ll_null=False, kind_code=None):
    """pgb_psis_expect on the first n columns of the device copies of ll (D, ld) and g (D, ldg) -> (rc, out)."""
    mem, lib = hip.mem, hip.lib
    md, gd = mem.from_host(np.ascontiguousarray(ll)), mem.from_host(np.ascontiguousarray(g))
    yd = None if y is None else mem.from_host(np.ascontiguousarray(y, np.float64))
    rows = 4 if kind == "value" else 3
    od = mem.from_host(np.full(rows * n + 8, SENTINEL))
    rc = lib.psis_expect_entry_point()(None if ll_null else mem.ptr(md), ll.shape[0] if D is None else D, n,
                                       ll.shape[1] if ld is None else ld, M, None if g_null else mem.ptr(gd),
                                       g.shape[1] if ldg is None else ldg, None if yd is None else mem.ptr(yd),
                                       host.KINDS[kind] if kind_code is None else kind_code, mem.ptr(od), mem.stream_ptr)
    return rc, mem.to_host(od)


def _functional(rng, D, ldg, n, kind):
    if kind == "pit":                                        # integer draws: ties with the integer y
        return rng.poisson(3.0, (D, ldg)).astype(float), rng.poisson(3.0, n).astype(float)
    return rng.normal(0.3, 1.2, (D, ldg)), None


# ------------------------------------------------------------------ 1. device == the host header
# D, rows, ld, ldg: fewer draws than lanes and fewer rows than a tile | D no multiple of 128 or 64, n no multiple of 8,
# ld > n, ldg != ld | T = 96 > 64 lanes, the candidate buffer compacts | the caps: M = 384, cap = 512
SHAPES = [(25, 3, 3, 3), (403, 11, 16, 29), (1003, 20, 20, 20), (16384, 9, 9, 9)]


@pytest.mark.parametrize("D,n,ld,ldg", SHAPES)
@pytest.mark.parametrize("kind", ["value", "pit"])
def test_device_equals_the_host_header(D, n, ld, ldg, kind, hip):
    ll = synthetic(D, n=ld)
    M = loo_mod.tail_length(D)
    assert M == {25: 5, 403: 61, 1003: 96, 16384: 384}[D]
    g, y = _functional(np.random.default_rng(D), D, ldg, n, kind)
    rc, out = _raw(hip, ll, g, n, M, y=y, kind=kind)
    assert rc == 0
    want = host.expect(ll, g, M, y=y, kind=kind, n=n)
    rows = want.shape[0]
    assert bits(out[:rows * n].reshape(rows, n), want), [int(np.sum(a != b)) for a, b in zip(out[:rows * n].reshape(rows, n), want)]
    assert np.all(out[rows * n:] == SENTINEL)                # nothing written beyond [2 + n_e][n]
    # outputs 0 and 1 are pgb_psis_rows' bits, on the device and on the host
    mem, lib = hip.mem, hip.lib
    md, od = mem.from_host(np.ascontiguousarray(ll)), mem.from_host(np.full(2 * n, SENTINEL))
    assert lib.psis_entry_point()(mem.ptr(md), D, n, ld, M, mem.ptr(od), mem.stream_ptr) == 0
    assert bits(mem.to_host(od), out[:2 * n])
    e, k = psis_host.psis(ll[:, :n], M)
    assert bits(out[:n], e) and bits(out[n:2 * n], k)


def _edge_matrices():
    rng = np.random.default_rng(21)
    out = {"three distinct values": np.log(rng.choice([.2, .5, .9], (1000, 37))),
           "five above the ties": _tied(rng, 1000, 5, 13), "four above the ties": _tied(rng, 999, 4, 9)}
    ll = rng.normal(-1.0, 0.5, (601, 30))
    for c in range(30):
        rows = rng.permutation(601)
        if c % 3 == 0:
            ll[rows[:1 + c % 7], c] = -2047.0
        elif c % 3 == 1:
            ll[rows[:3], c] = 2047.0
        else:
            ll[rows[:8], c] = -2047.0 + np.arange(8) * 3.0
            ll[rows[8:11], c] = 2047.0
    ll[:, 29] = -2047.0
    out["clamp values"] = ll
    return out


def test_matrix_call_equals_the_host_header_on_the_edge_cases(hip, monkeypatch):
    for what, ll in _edge_matrices().items():
        D, n = ll.shape
        M = loo_mod.tail_length(D)
        rng = np.random.default_rng(n)
        g = rng.normal(0.0, 2.0, (D, n))
        g[::7] = 1e200                                       # held at +-1e150
        g[3::7] = -np.inf
        res = _quiet(psis_expectation_matrix, ll, g, backend=hip)
        want = host.expect(ll, g, M)
        assert bits(res["elpd_loo_i"], want[0]) and bits(res["pareto_k_i"], want[1]), what
        assert bits(res["loo_mean"], want[2]) and bits(res["loo_sd"], np.sqrt(np.maximum(want[3] - want[2] * want[2], 0.0))), what
        assert res["n_clamped"] == int(np.sum(np.abs(ll) >= 2047.0)) and res["tail_len"] == M and res["n_draws"] == D
        gp, y = rng.poisson(3.0, (D, n)).astype(float), rng.poisson(3.0, n).astype(float)
        res = _quiet(psis_expectation_matrix, ll, gp, y=y, kind="pit", backend=hip)
        want = host.expect(ll, gp, M, y=y, kind="pit")
        assert bits(res["elpd_loo_i"], want[0]) and bits(res["pareto_k_i"], want[1]) and bits(res["loo_pit"], want[2]), what
        assert np.all((res["loo_pit"] >= 0.0) & (res["loo_pit"] <= 1.0))
    # several row blocks, a longer tail (reff), the exact identities on the device
    ll = synthetic(403, n=150)
    g = np.random.default_rng(3).normal(0.0, 1.0, ll.shape)
    one = _quiet(psis_expectation_matrix, ll, g, reff=0.25, backend=hip)
    want = host.expect(ll, g, loo_mod.tail_length(403, 0.25))
    assert one["tail_len"] == loo_mod.tail_length(403, 0.25) and bits(one["loo_mean"], want[2])
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(8 * (2 * 403 + 5) * 64))     # blocks of 64 rows: three of them
    again = _quiet(psis_expectation_matrix, ll, g, reff=0.25, backend=hip)
    for key in ("elpd_loo_i", "pareto_k_i", "loo_mean", "loo_sd"):
        assert bits(again[key], one[key]), key
    const = _quiet(psis_expectation_matrix, ll, np.full(ll.shape, 2.0), backend=hip)
    assert np.all(const["loo_mean"] == 2.0) and np.all(const["loo_sd"] == 0.0)
    pit = _quiet(psis_expectation_matrix, ll, g, y=np.full(150, 1e9), kind="pit", backend=hip)
    assert np.all(pit["loo_pit"] == 1.0)


def test_refusals_before_any_launch(hip):
    ll, g, y = np.zeros((50, 16)), np.zeros((50, 16)), np.zeros(16)
    cases = [(dict(M=0), "tail_len must be in"), (dict(M=50), "tail_len must be in"), (dict(ld=15), "ld >= n_rows"),
             (dict(D=1, M=1), "at least 2 draws"), (dict(D=psis_host.max_draws() + 1), "pgb_psis_expect takes at most"),
             (dict(D=8000, M=psis_host.max_tail() + 1), "beyond"), (dict(ll_null=True), "null argument"),
             (dict(g_null=True), "g_dev is null"), (dict(ldg=15), "ldg must be >= n_rows"),
             (dict(kind_code=2), "kind must be 0"), (dict(kind_code=-1), "kind must be 0"),
             (dict(kind="pit", y=None), "y_dev is null")]
    for kw, msg in cases:
        args = dict(M=10, y=y if kw.get("kind") != "pit" else None)
        args.update(kw)
        M = args.pop("M")
        rc, out = _raw(hip, ll, g, 16, M, **args)
        assert rc == -1, kw                                  # PGB_E_INVALID
        with pytest.raises(_abi.PGBError, match=msg):
            hip.lib.check(rc, "pgb_psis_expect")
        assert np.all(out == SENTINEL), kw
    mem, lib = hip.mem, hip.lib
    ad, od = mem.from_host(np.zeros(32)), mem.from_host(np.zeros(16))
    add = lib.add_offset_entry_point()
    for a, D, K, n, o, msg in ((None, 2, 1, 16, mem.ptr(od), "a_dev is null"), (mem.ptr(ad), 2, 1, 16, None, "offset_dev is null"),
                               (mem.ptr(ad), 0, 1, 16, mem.ptr(od), "must be >= 1"), (mem.ptr(ad), 2, 1, 0, mem.ptr(od), "must be >= 1")):
        rc = add(a, D, K, n, o, mem.stream_ptr)
        assert rc == -1
        with pytest.raises(_abi.PGBError, match=msg):
            lib.check(rc, "pgb_add_offset")


# ------------------------------------------------------------------ 2. loo_pit / loo_predictive, end to end
N, P, M_TREES, TUNE, DRAWS = 150, 4, 10, 20, 30


class Pooled:
    """Several chains behind one object, as the multi-chain sampler presents them."""

    def __init__(self, parts):
        self._chain_samplers = parts

    def sample_posterior(self, X, idx=None):
        mu = np.concatenate([p.sample_posterior(X, list(range(p.n_draws)), None) for p in self._chain_samplers])
        return mu if idx is None else mu[np.asarray(idx)]


def _fit(which, hip):
    """Two chains of a short fit pooled: (X, y, sampler, likelihood, points, K)."""
    rng = np.random.default_rng({"normal": 51, "poisson": 52, "probit": 53, "categorical": 54}[which])
    X = rng.uniform(0, 1, (N, P))
    f = 2.0 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 1.5 * (X[:, 2] - 0.5) + X[:, 3]
    K = 1
    if which == "normal":
        y, lik, fit_lik = f + rng.normal(0, 0.5, N), NormalLikelihood("sigma"), None
    elif which == "poisson":
        y, lik = rng.poisson(np.exp(0.5 * f)).astype(float), PoissonLikelihood()
        fit_lik = lik
    elif which == "probit":
        y, lik = (rng.random(N) < 1.0 / (1.0 + np.exp(-2 * (f - 1.5)))).astype(float), BernoulliLikelihood("probit")
        fit_lik = lik
    else:
        y, lik, K = np.minimum((f + rng.normal(0, 0.5, N)).clip(0) // 1.2, 2.0), CategoricalLikelihood(3), 3
        fit_lik = lik
    op = BARTOp(X, y, m=M_TREES)
    parts, sigma = [], []
    for c in (0, 1):
        kw = {} if fit_lik is None else {"likelihood": fit_lik}
        res = sample_chain(op, TUNE, DRAWS, num_particles=10, random_seed=4, chain=c, backend=hip, keep_draws=False, **kw)
        base, batches = res["history"]
        parts.append(PosteriorSampler.from_history(batches, base, M_TREES, K, backend=hip))
        sigma.append(res.get("sigma"))
    points = {"sigma": np.concatenate(sigma)} if which == "normal" else None
    return X, y, Pooled(parts), lik, points, K


_FITS = {}


def _cached_fit(which, hip):
    if which not in _FITS:
        _FITS[which] = _fit(which, hip)
    return _FITS[which]


def _end_to_end(fit, monkeypatch, idx=None, seed=11):
    X, y, multi, lik, points, K = fit
    off = np.random.default_rng(5).normal(0, 0.2, (K, N))
    kw = {"offset": off}
    if points is not None:
        kw["points"] = points if idx is None else {"sigma": points["sigma"][idx]}
    if idx is not None:
        kw["draws"] = idx
    ll = pointwise_log_likelihood(multi, X, y, lik, **kw)
    yrep = posterior_predictive(multi, X, lik, random_seed=seed, **kw)
    mu = multi.sample_posterior(X, idx) + off[None]          # (D, K, n)
    D = ll.shape[0]
    M = loo_mod.tail_length(D)
    assert ll.shape == yrep.shape == (D, N) and mu.shape == (D, K, N)
    plain = _quiet(loo, multi, X, y, lik, **kw)

    def same_loo(res):
        for key in ("elpd_loo_i", "pareto_k_i", "lppd_i", "p_loo_i"):
            assert bits(res[key], plain[key]), key
        for key in ("elpd_loo", "p_loo", "se_elpd_loo", "khat_threshold", "n_high_k", "tail_len", "n_draws", "n_clamped"):
            assert res[key] == plain[key], key

    results = []
    for blk in (None, str(1 << 16), str(160000)):            # one block of rows, blocks of 64, blocks of 64 or 128
        monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
        if blk:
            monkeypatch.setenv("PGB_PW_BLOCK_BYTES", blk)
        results.append((_quiet(loo_pit, multi, X, y, lik, random_seed=seed, **kw),
                        _quiet(loo_predictive, multi, X, y, lik, kind="mu", **kw),
                        _quiet(loo_predictive, multi, X, y, lik, kind="y", random_seed=seed, **kw)))
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    pit, pmu, py = results[0]
    # LOO-PIT: the host build on the two matrices the public calls give
    want = host.expect(ll, yrep, M, y=y, kind="pit")
    same_loo(pit)
    assert bits(pit["elpd_loo_i"], want[0]) and bits(pit["pareto_k_i"], want[1]) and bits(pit["loo_pit"], want[2])
    assert pit["n_capped"] == 0 and pit["n_exhausted"] == 0
    # the linear predictor, output by output
    same_loo(pmu)
    wm = np.stack([host.expect(ll, mu[:, k, :], M) for k in range(K)])            # (K, 4, n)
    mean, sd = wm[:, 2], np.sqrt(np.maximum(wm[:, 3] - wm[:, 2] * wm[:, 2], 0.0))
    assert pmu["loo_mean"].shape == ((N,) if K == 1 else (K, N)) and "loo_residual" not in pmu
    assert bits(pmu["loo_mean"], mean.reshape(pmu["loo_mean"].shape)) and bits(pmu["loo_sd"], sd.reshape(pmu["loo_sd"].shape))
    # the replicated observations
    same_loo(py)
    wy = host.expect(ll, yrep, M)
    assert bits(py["loo_mean"], wy[2]) and bits(py["loo_sd"], np.sqrt(np.maximum(wy[3] - wy[2] * wy[2], 0.0)))
    assert ("loo_residual" in py) == (K == 1) and (K > 1 or bits(py["loo_residual"], y - wy[2]))
    # ... whatever the blocking
    for other in results[1:]:
        for a, b in zip(other, results[0]):
            assert a.keys() == b.keys()
            for key in a:
                assert bits(a[key], b[key]) if isinstance(a[key], np.ndarray) else a[key] == b[key], key
    return pit


def test_loo_pit_of_a_normal_fit_and_of_a_subset_of_its_draws(hip, monkeypatch):
    fit = _cached_fit("normal", hip)
    pit = _end_to_end(fit, monkeypatch)
    assert pit["n_draws"] == 2 * DRAWS and pit["tail_len"] == 12
    assert 0.2 < pit["loo_pit"].mean() < 0.8 and np.all((pit["loo_pit"] >= 0.0) & (pit["loo_pit"] <= 1.0))
    idx = [DRAWS + 2, 1, 1] + list(range(3, 2 * DRAWS, 2))  # a subset with a repeat (a tie): values belong to positions
    sub = _end_to_end(fit, monkeypatch, idx=idx)
    assert sub["n_draws"] == len(idx)


@pytest.mark.parametrize("which", ["poisson", "probit", "categorical"])
def test_loo_pit_of_the_discrete_families(which, hip, monkeypatch):
    pit = _end_to_end(_cached_fit(which, hip), monkeypatch)
    assert np.all((pit["loo_pit"] >= 0.0) & (pit["loo_pit"] <= 1.0))
