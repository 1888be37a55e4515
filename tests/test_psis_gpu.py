"""PSIS-LOO on the MI355X: ``k_psis`` against the host build of the same header (``tests/_psis_host.py``) -- bit for
bit, on synthetic matrices, on the edge cases of the tail and end to end on short real chains of ``sample_chain`` --
one tie to arithmetic that does not come from the shared header (``tests/_psis_numpy.py``), and the refusals."""
import sys
import warnings

import numpy as np
import pytest

import _pointwise_host as pw_host
import _psis_host as host
import _psis_numpy as ref
from pymc_bart_amd import (BARTOp, BernoulliLikelihood, CategoricalLikelihood, CompiledLikelihood, NormalLikelihood, _abi)
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.loo import loo, psis_loo_matrix
from pymc_bart_amd.pointwise import log_predictive_density, pointwise_log_likelihood
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler
from test_psis import _tied, bound, synthetic

pytestmark = pytest.mark.gpu
loo_mod = sys.modules["pymc_bart_amd.loo"]

N, P, M_TREES, DRAWS = 1500, 7, 20, 70


@pytest.fixture(autouse=True)
def _env(tmp_path_factory, monkeypatch):
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit"))
    monkeypatch.delenv("PGB_PW_WGS", raising=False)
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)       # (rows with a high k are the data's, not the test's)
        return fn(*a, **kw)


def _same(res, ll, reff=1.0):
    e, k = host.psis(ll, loo_mod.tail_length(ll.shape[0], reff))
    assert res["tail_len"] == loo_mod.tail_length(ll.shape[0], reff) and res["n_draws"] == ll.shape[0]
    assert np.array_equal(res["elpd_loo_i"], e), int(np.sum(res["elpd_loo_i"] != e))
    assert np.array_equal(res["pareto_k_i"], k), int(np.sum(res["pareto_k_i"] != k))


def _edge_matrices():
    rng = np.random.default_rng(21)
    out = {"three distinct values": np.log(rng.choice([.2, .5, .9], (1000, 37))),
           "five above the ties": _tied(rng, 1000, 5, 13), "four above the ties": _tied(rng, 999, 4, 9),
           "D = 2": rng.normal(-1.0, 0.7, (2, 70)), "D = 25": rng.normal(-1.0, 0.7, (25, 70)),
           "bounded ratios": -0.5 * rng.uniform(0.0, 1.0, (2001, 19))}
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


# ------------------------------------------------------------------ 1. psis_loo_matrix == the host header
@pytest.mark.parametrize("D", [400, 1000, 4000])
def test_matrix_call_equals_the_host_header_on_synthetic_matrices(D, hip, monkeypatch):
    ll = synthetic(D + 3, n=397)                            # D not a multiple of 32, n not a multiple of 8 or 64
    res = _quiet(psis_loo_matrix, ll, backend=hip)
    _same(res, ll)
    assert res["n_clamped"] == 0 and "lppd_i" not in res
    assert res["elpd_loo"] == float(res["elpd_loo_i"].sum()) and res["se_elpd_loo"] > 0.0
    assert res["n_high_k"] == int(np.sum(res["pareto_k_i"] > res["khat_threshold"])) > 0
    with pytest.warns(UserWarning, match=f"{res['n_high_k']} of 397 rows have a Pareto k above"):
        psis_loo_matrix(ll, backend=hip)
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(8 * (D + 5) * 64))    # blocks of 64 rows: seven of them
    again = _quiet(psis_loo_matrix, ll, backend=hip)
    assert np.array_equal(again["elpd_loo_i"], res["elpd_loo_i"]) and np.array_equal(again["pareto_k_i"], res["pareto_k_i"])


def test_matrix_call_equals_the_host_header_on_the_edge_cases(hip):
    for what, ll in _edge_matrices().items():
        res = _quiet(psis_loo_matrix, ll, backend=hip)
        _same(res, ll)
        assert res["n_clamped"] == int(np.sum(np.abs(ll) >= 2047.0)), what
    ll = synthetic(1000, n=50)
    _same(_quiet(psis_loo_matrix, ll, reff=0.25, backend=hip), ll, reff=0.25)
    for D, n in ((8003, 41), (host.max_draws(), 17)):       # the long tails: the larger candidate buffer, the cap itself
        ll = synthetic(D, n=n)
        assert loo_mod.tail_length(D) > 191
        _same(_quiet(psis_loo_matrix, ll, backend=hip), ll)
    big = np.random.default_rng(1).normal(-1, 1, (300, 10)) * 3000.0   # values beyond the clamp are held and counted
    res = _quiet(psis_loo_matrix, big, backend=hip)
    _same(res, np.clip(big, -2047.0, 2047.0))
    assert res["n_clamped"] == int(np.sum(np.abs(big) >= 2047.0)) > 0


def _raw(hip, ll, n, ld, M):
    """pgb_psis_rows on the first n columns of the device copy of ll (D, ld)."""
    mem, lib = hip.mem, hip.lib
    md = mem.from_host(np.ascontiguousarray(ll))
    od = mem.from_host(np.full(2 * n + 8, -7.0))
    rc = lib.psis_entry_point()(mem.ptr(md), ll.shape[0], n, ld, M, mem.ptr(od), mem.stream_ptr)
    return rc, mem.to_host(od)


def test_entry_point_with_a_leading_dimension_beyond_the_rows(hip):
    ll = synthetic(403, n=300)
    M = loo_mod.tail_length(403)
    for n in (1, 7, 8, 9, 131, 300):
        rc, out = _raw(hip, ll, n, 300, M)
        assert rc == 0
        e, k = host.psis(ll[:, :n], M)
        assert np.array_equal(out[:n], e) and np.array_equal(out[n:2 * n], k), n
        assert np.all(out[2 * n:] == -7.0)                  # nothing written beyond [2][n]


def test_refusals_before_any_launch(hip):
    ll = np.zeros((50, 16))
    for D, n, ld, M, msg in ((50, 16, 16, 0, "tail_len"), (50, 16, 16, 50, "tail_len"), (50, 16, 15, 10, "ld >= n_rows"),
                             (1, 16, 16, 1, "at least 2 draws"), (host.max_draws() + 1, 16, 16, 10, "at most"),
                             (8000, 16, 16, host.max_tail() + 1, "beyond")):
        mem, lib = hip.mem, hip.lib
        md = mem.from_host(ll)
        od = mem.from_host(np.full(32, -7.0))
        rc = lib.psis_entry_point()(mem.ptr(md), D, n, ld, M, mem.ptr(od), mem.stream_ptr)
        assert rc == -1, (D, n, ld, M)                        # PGB_E_INVALID
        with pytest.raises(_abi.PGBError, match=msg):
            lib.check(rc, "pgb_psis_rows")
        assert np.all(mem.to_host(od) == -7.0)


# ------------------------------------------------------------------ 2. loo, end to end
def _data(seed=0, n=N, p=P):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, p))
    f = 2.0 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 1.5 * (X[:, 2] - 0.5) + X[:, 3]
    return rng, X, f


def _fit(X, Y, lik, hip, K=1, seed=1, sigma=None, draws=DRAWS):
    op = BARTOp(X, Y, m=M_TREES)
    res = sample_chain(op, 8, draws, num_particles=10, random_seed=seed, chain=0, backend=hip, keep_draws=False,
                       likelihood=lik, sigma=sigma)
    base, batches = res["history"]
    return PosteriorSampler.from_history(batches, base, M_TREES, K, backend=hip), res


def _end_to_end(ps, X, y, lik, **kw):
    """loo == the host header on the matrix call's output; lppd_i == log_predictive_density's bits."""
    res = _quiet(loo, ps, X, y, lik, **kw)
    ll, nc = pointwise_log_likelihood(ps, X, y, lik, return_clamped=True, **kw)
    _same(res, ll)
    s = log_predictive_density(ps, X, y, lik, **kw)
    assert np.array_equal(res["lppd_i"], s["lppd_i"]) and np.array_equal(res["lppd_i"], pw_host.reduce(ll)[0])
    assert np.array_equal(res["p_loo_i"], res["lppd_i"] - res["elpd_loo_i"])
    assert res["p_loo"] == float(res["p_loo_i"].sum()) and res["elpd_loo"] == float(res["elpd_loo_i"].sum())
    assert res["n_clamped"] == nc == s["n_clamped"]
    n = res["elpd_loo_i"].size
    assert res["se_elpd_loo"] == float(np.sqrt(n * res["elpd_loo_i"].var()))
    assert res["khat_threshold"] == min(1.0 - 1.0 / np.log10(ll.shape[0]), 0.7)
    assert res["n_high_k"] == int(np.sum(res["pareto_k_i"] > res["khat_threshold"]))
    return res, ll


def test_loo_of_a_normal_fit_for_any_launch_geometry_and_block_size(hip, monkeypatch):
    rng, X, f = _data(31)
    y = f + rng.normal(0, 0.5, N)
    lik = NormalLikelihood("sigma")
    ps, fit = _fit(X, y, lik, hip)
    pts = {"sigma": fit["sigma"]}
    res, ll = _end_to_end(ps, X, y, lik, points=pts)
    assert ll.shape == (DRAWS, N) and res["tail_len"] == 14 and np.isfinite(res["pareto_k_i"]).mean() > 0.9
    for wgs, blk in (("64", None), ("100000", str(1 << 16)), (None, str(8 * (DRAWS + 40) * 128))):
        monkeypatch.delenv("PGB_PW_WGS", raising=False)
        monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
        if wgs:
            monkeypatch.setenv("PGB_PW_WGS", wgs)
        if blk:
            monkeypatch.setenv("PGB_PW_BLOCK_BYTES", blk)
        again = _quiet(loo, ps, X, y, lik, points=pts)
        for key in ("elpd_loo_i", "pareto_k_i", "lppd_i"):
            assert np.array_equal(again[key], res[key]), (wgs, blk, key)
        assert again["n_clamped"] == res["n_clamped"]
    monkeypatch.delenv("PGB_PW_WGS", raising=False)
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    # a subset of the draws (with a repeat: a tie), and held-out rows
    idx = [3, 3] + list(range(5, 60, 2))
    _end_to_end(ps, X, y, lik, points={"sigma": fit["sigma"][idx]}, draws=idx)
    _, X2, f2 = _data(32, n=777)
    y2 = f2 + np.random.default_rng(33).normal(0, 0.5, 777)
    _end_to_end(ps, X2, y2, lik, points=pts)
    # the matrix call on the same matrix: the same bits, the same clamp count
    m = _quiet(psis_loo_matrix, ll, backend=hip)
    assert np.array_equal(m["elpd_loo_i"], res["elpd_loo_i"]) and np.array_equal(m["pareto_k_i"], res["pareto_k_i"])
    assert m["n_clamped"] == res["n_clamped"] == 0
    tight = NormalLikelihood(1e-3)                          # residuals against sigma = 1e-3: clamped pairs
    rt = _quiet(loo, ps, X, y, tight)
    llt, nct = pointwise_log_likelihood(ps, X, y, tight, return_clamped=True)
    _same(rt, llt)
    assert rt["n_clamped"] == nct == _quiet(psis_loo_matrix, llt, backend=hip)["n_clamped"] > 0


def test_loo_of_a_probit_and_of_a_categorical_fit(hip):
    rng, X, f = _data(34)
    yb = (rng.random(N) < 1.0 / (1.0 + np.exp(-2 * (f - 1.5)))).astype(float)
    lik = BernoulliLikelihood("probit")
    ps, _ = _fit(X, yb, lik, hip)
    _end_to_end(ps, X, yb, lik)
    yc = np.minimum((f + rng.normal(0, 0.5, N)).clip(0) // 1.2, 2.0)
    likc = CategoricalLikelihood(3)
    pc, _ = _fit(X, yc, likc, hip, K=3)
    _end_to_end(pc, X, yc, likc)


CENSORED = """double z = (y - mu) / s;
if (aux > 0.5) return log_ndtr(-z) * t;      /* right-censored at y */
return -log(s) - 0.5 * z * z - 0.9189385332046727;"""


def test_loo_of_a_compiled_right_censored_normal(hip):
    rng, X, f = _data(35)
    y = f + rng.normal(0, 0.5, N)
    aux = (rng.random(N) < 0.2).astype(float)
    ps, _ = _fit(X, y, CompiledLikelihood(CENSORED, params={"s": 0.5, "t": 1.0}, aux=aux), hip, sigma=1.0)
    lik = CompiledLikelihood(CENSORED, params={"s": "s", "t": "t"}, aux=aux)
    pts = {"s": rng.uniform(0.3, 0.8, DRAWS), "t": rng.uniform(0.9, 1.1, DRAWS)}
    _end_to_end(ps, X, y, lik, points=pts)


def test_loo_of_two_chains_pooled(hip):
    rng, X, f = _data(36)
    y = f + rng.normal(0, 0.5, N)
    lik = NormalLikelihood("sigma")
    op = BARTOp(X, y, m=M_TREES)
    chains = [sample_chain(op, 8, 40, random_seed=2, chain=c, backend=hip, keep_draws=False) for c in (0, 1)]
    attach_history(op, chains)
    multi = _get_posterior_sampler(op, backend=hip)
    sig = np.concatenate([c["sigma"] for c in chains])
    res, ll = _end_to_end(multi, X, y, lik, points={"sigma": sig})
    assert ll.shape == (80, N) and res["n_draws"] == 80 and res["tail_len"] == 16


# ------------------------------------------------------------------ 3. one tie to arithmetic outside the header
def test_device_against_the_numpy_restatement(hip):
    for D in (400, 1000):
        ll = synthetic(D)
        res = _quiet(psis_loo_matrix, ll, backend=hip)
        er, kr, _ = ref.psis_matrix(ll)
        ok = kr <= 0.7
        assert int((~ok).sum()) <= 0.02 * ok.size
        dk = float(np.max(np.abs(res["pareto_k_i"][ok] - kr[ok])))
        de = float(np.max(np.abs(res["elpd_loo_i"][ok] - er[ok])))
        print(f"D = {D}: device against NumPy, max |dk| = {dk:.3e}, max |d elpd| = {de:.3e} (bound {bound():.3e})")
        assert dk <= bound() and de <= bound()
