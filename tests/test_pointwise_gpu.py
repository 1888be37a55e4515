"""Pointwise log-likelihood / lppd / WAIC on the MI355X: the fused kernels against the host build of the same header
(``tests/_pointwise_host.py``) applied to what ``sample_posterior`` predicts -- bit for bit, matrix and summary --
for every built-in family and for compiled bodies, on short real chains of ``sample_chain``; and one tie to
arithmetic that does not come from the shared header (NumPy / SciPy)."""
import warnings

import numpy as np
import pytest
from scipy import special, stats

import _pointwise_host as host
from pymc_bart_amd import (AsymmetricLaplaceLikelihood, BARTOp, BernoulliLikelihood, CategoricalLikelihood,
                           CompiledLikelihood, GammaLikelihood, NegativeBinomialLikelihood, NormalLikelihood,
                           NormalMeanScaleLikelihood, PoissonLikelihood, StudentTLikelihood, _abi)
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.compiled import compile_loglik
from pymc_bart_amd.pointwise import log_predictive_density, pointwise_log_likelihood
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler

pytestmark = pytest.mark.gpu

N, P, M, DRAWS = 3000, 7, 20, 12
C_ = 32  # PGB_PW_CHUNK


@pytest.fixture(autouse=True)
def _jit_cache(tmp_path_factory, monkeypatch):
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit"))


def _data(seed=0, n=N, p=P):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, p))
    f = 2.0 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 1.5 * (X[:, 2] - 0.5) + X[:, 3] if p >= 4 else X.sum(axis=1)
    return rng, X, f


def _fit(X, Y, lik, hip, K=1, seed=1, chain=0, sigma=None, **op_kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (response="mix" is flagged experimental, as upstream flags it)
        op = BARTOp(X, Y, m=M, **op_kw)
    res = sample_chain(op, 8, DRAWS, num_particles=10, random_seed=seed, chain=chain, backend=hip, keep_draws=False,
                       likelihood=lik, sigma=sigma)
    base, batches = res["history"]
    return PosteriorSampler.from_history(batches, base, M, K, backend=hip), res


def _family_case(name, rng, f):
    """(likelihood, y, K, points builder) of one built-in family, with data the family could have produced."""
    n = f.size
    if name == "normal":
        return NormalLikelihood("sigma"), f + rng.normal(0, 0.5, n), 1
    if name in ("bernoulli_probit", "bernoulli_logit"):
        return BernoulliLikelihood(name.split("_")[1]), (rng.random(n) < special.expit(2 * (f - 1.5))).astype(float), 1
    if name == "poisson_log":
        return PoissonLikelihood(), rng.poisson(np.exp(0.5 * f)).astype(float), 1
    if name == "negbin_log":
        return NegativeBinomialLikelihood(2.0), rng.poisson(np.exp(0.5 * f)).astype(float), 1
    if name == "asymmetric_laplace":
        return AsymmetricLaplaceLikelihood(q=0.7, b=0.5), f + rng.normal(0, 0.5, n), 1
    if name == "student_t":
        return StudentTLikelihood(nu=4.0, sigma=0.5), f + 0.5 * rng.standard_t(4, n), 1
    if name == "gamma_log":
        return GammaLikelihood(3.0), rng.gamma(3.0, np.exp(0.3 * f) / 3.0), 1
    if name == "categorical":
        return CategoricalLikelihood(3), np.minimum((f + rng.normal(0, 0.5, n)).clip(0) // 1.2, 2.0), 3
    if name == "normal_meanscale":
        return NormalMeanScaleLikelihood(), f + rng.normal(0, 0.5, n), 2
    raise KeyError(name)


def _points(lik, res, idx):
    """The per-draw params the way a user has them: sigma from the chain for the Normal family."""
    return {"sigma": res["sigma"][np.asarray(idx)]} if lik.family == "normal" else None


def _host_matrix(ps, lik, X, y, idx, points, offset=None):
    mu = ps.sample_posterior(X, list(idx), None)                      # (D, K, n): pgb_predict
    D = len(idx)
    if points is None:
        prm = np.tile(np.asarray(lik.params(None), float), (D, 1))
    else:
        prm = np.array([lik.params({k: v[d] for k, v in points.items()}) for d in range(D)], float).reshape(D, -1)
    off = None if offset is None else np.asarray(offset, float).reshape(mu.shape[1:])
    return host.matrix(lik.family, y, mu, prm, off, return_clamped=True)


FAMILIES = ["normal", "bernoulli_probit", "bernoulli_logit", "poisson_log", "negbin_log", "asymmetric_laplace",
            "student_t", "gamma_log", "categorical", "normal_meanscale"]


# ------------------------------------------------------------------ 1. matrix == host, bit for bit
@pytest.mark.parametrize("name", FAMILIES)
def test_matrix_equals_the_host_on_the_predictions_of_every_family(name, hip):
    rng, X, f = _data(3)
    lik, y, K = _family_case(name, rng, f)
    ps, res = _fit(X, y, lik, hip, K=K)
    idx = list(range(DRAWS))
    pts = _points(lik, res, idx)
    got, nc = pointwise_log_likelihood(ps, X, y, lik, points=pts, return_clamped=True)
    want, nc_host = _host_matrix(ps, lik, X, y, idx, pts)
    assert got.shape == (DRAWS, N) and np.array_equal(got, want), name
    assert nc == 0 and nc_host == 0
    # held-out rows too (the walk meets values the trees were not grown on)
    _, X2, f2 = _data(4, n=1000)
    _, y2, _ = _family_case(name, np.random.default_rng(5), f2)
    got2 = pointwise_log_likelihood(ps, X2, y2, lik, points=pts, draws=idx)
    assert np.array_equal(got2, _host_matrix(ps, lik, X2, y2, idx, pts)[0])


def test_matrix_with_an_offset_and_with_mix_leaves(hip):
    rng, X, f = _data(6)
    y = f + rng.normal(0, 0.5, N)
    lik = NormalLikelihood("sigma")
    ps, res = _fit(X, y, lik, hip)
    idx = [0, 3, 3, 11, 7]                                             # a draw index list with a repeat
    pts = _points(lik, res, idx)
    off = rng.normal(0, 0.3, N)
    got, nc = pointwise_log_likelihood(ps, X, y, lik, points=pts, offset=off, draws=idx, return_clamped=True)
    assert np.array_equal(got, _host_matrix(ps, lik, X, y, idx, pts, off)[0]) and nc == 0
    assert not np.array_equal(got, pointwise_log_likelihood(ps, X, y, lik, points=pts, draws=idx))
    K2 = CategoricalLikelihood(3)                                      # an offset of K rows
    yc = np.minimum((f + rng.normal(0, 0.5, N)).clip(0) // 1.2, 2.0)
    pc, _ = _fit(X, yc, K2, hip, K=3)
    offk = rng.normal(0, 0.3, (3, N))
    got = pointwise_log_likelihood(pc, X, yc, K2, offset=offk, draws=idx)
    assert np.array_equal(got, _host_matrix(pc, K2, X, yc, idx, None, offk)[0])
    pm, resm = _fit(X, y, lik, hip, response="mix")                    # linear leaves: the walk applies the slopes
    assert pm.pool.svar is not None and np.any(np.asarray(pm.pool.svar) >= 0)
    ptm = _points(lik, resm, idx)
    got = pointwise_log_likelihood(pm, X, y, lik, points=ptm, draws=idx)
    assert np.array_equal(got, _host_matrix(pm, lik, X, y, idx, ptm)[0])


def test_matrix_on_the_stack_walk_and_on_the_global_read_walk(hip):
    """One-hot / subset columns and NaN rows in X (the walk that marginalises); p > PRED_LDS_MAXP (no LDS tile)."""
    rng, X, f = _data(7)
    X[:, 4] = (X[:, 4] > 0.5).astype(float)                            # one-hot
    X[:, 5] = np.floor(X[:, 5] * 6)                                    # subset: category codes 0 .. 5
    f = f + 0.8 * X[:, 4] + 0.5 * np.isin(X[:, 5], (1, 4))
    X[rng.random(N) < 0.05, 0] = np.nan
    X[rng.random(N) < 0.03, 5] = np.nan
    y = f + rng.normal(0, 0.5, N)
    lik = NormalLikelihood("sigma")
    rules = ["ContinuousSplit"] * 4 + ["OneHotSplit", "SubsetSplit", "ContinuousSplit"]
    ps, res = _fit(X, y, lik, hip, split_rules=rules)
    assert set(np.unique(np.asarray(ps.pool.rule)[np.asarray(ps.pool.var) >= 0])) >= {1, 2}
    idx = list(range(DRAWS))
    pts = _points(lik, res, idx)
    got, nc = pointwise_log_likelihood(ps, X, y, lik, points=pts, return_clamped=True)
    assert np.array_equal(got, _host_matrix(ps, lik, X, y, idx, pts)[0]) and nc == 0
    Xc = np.where(np.isnan(X), 0.0, X)                                 # clean rows under the same (non-continuous) trees
    assert np.array_equal(pointwise_log_likelihood(ps, Xc, y, lik, points=pts),
                          _host_matrix(ps, lik, Xc, y, idx, pts)[0])
    rng, Xw, fw = _data(8, n=1500, p=130)
    yw = fw + rng.normal(0, 0.5, 1500)
    pw, resw = _fit(Xw, yw, lik, hip)
    ptw = _points(lik, resw, idx)
    got, nc = pointwise_log_likelihood(pw, Xw, yw, lik, points=ptw, return_clamped=True)
    assert np.array_equal(got, _host_matrix(pw, lik, Xw, yw, idx, ptw)[0]) and nc == 0
    Xn = Xw.copy()
    Xn[::7, 0] = np.nan                                                # ... and the stack walk without the tile
    assert np.array_equal(pointwise_log_likelihood(pw, Xn, yw, lik, points=ptw),
                          _host_matrix(pw, lik, Xn, yw, idx, ptw)[0])
    s = log_predictive_density(pw, Xn, yw, lik, points=ptw)
    lln = pointwise_log_likelihood(pw, Xn, yw, lik, points=ptw)
    assert np.array_equal(np.stack([s["lppd_i"], s["mean_i"], s["p_waic_i"]]), host.reduce(lln))


# ------------------------------------------------------------------ 2. summary == host reduction of that matrix
def test_summary_equals_the_host_reduction_for_any_launch_geometry(hip, monkeypatch):
    rng, X, f = _data(9)
    y = f + rng.normal(0, 0.5, N)
    lik = NormalLikelihood("sigma")
    ps, res = _fit(X, y, lik, hip)
    pick = np.random.default_rng(1)
    for D in (1, 2, C_ - 1, C_, C_ + 1, 3 * C_ + 5):
        idx = pick.integers(0, DRAWS, D).tolist()                      # repeats: D draws without a long chain
        pts = _points(lik, res, idx)
        monkeypatch.delenv("PGB_PW_WGS", raising=False)
        ll, nc = pointwise_log_likelihood(ps, X, y, lik, points=pts, draws=idx, return_clamped=True)
        want = host.reduce(ll)
        outs = []
        for wgs in (None, "64", "100000"):
            if wgs is None:
                monkeypatch.delenv("PGB_PW_WGS", raising=False)
            else:
                monkeypatch.setenv("PGB_PW_WGS", wgs)
            s = log_predictive_density(ps, X, y, lik, points=pts, draws=idx)
            outs.append(np.stack([s["lppd_i"], s["mean_i"], s["p_waic_i"]]))
            assert s["n_draws"] == D and s["n_clamped"] == nc == 0
            assert s["lppd"] == float(s["lppd_i"].sum())
            assert s["elpd_waic"] == float((s["lppd_i"] - s["p_waic_i"]).sum()) and s["se_elpd_waic"] > 0.0
            assert np.array_equal(pointwise_log_likelihood(ps, X, y, lik, points=pts, draws=idx), ll)  # matrix mode too
        for o in outs:
            assert np.array_equal(o, want), D
    monkeypatch.delenv("PGB_PW_WGS", raising=False)


# ------------------------------------------------------------------ 3. compiled bodies
CENSORED = """double z = (y - mu) / s;
if (aux > 0.5) return log_ndtr(-z) * t;      /* right-censored at y */
return -log(s) - 0.5 * z * z - 0.9189385332046727;"""
TWO = """double sd = fabs(mu[1]) + 0.1;
double z = (y - mu[0]) / sd;
return -log(sd) - 0.5 * z * z - w * aux;"""


def test_compiled_bodies_equal_their_host_builds(hip):
    rng, X, f = _data(10)
    y = f + rng.normal(0, 0.5, N)
    aux = (rng.random(N) < 0.2).astype(float)
    ps, _ = _fit(X, y, CompiledLikelihood(CENSORED, params={"s": 0.5, "t": 1.0}, aux=aux), hip, sigma=1.0)
    lik = CompiledLikelihood(CENSORED, params={"s": "s", "t": "t"}, aux=aux)   # the score reads s, t per draw
    idx = [0, 5, 5, 11] + list(range(DRAWS))
    D = len(idx)
    pts = {"s": rng.uniform(0.3, 0.8, D), "t": rng.uniform(0.9, 1.1, D)}
    got, nc = pointwise_log_likelihood(ps, X, y, lik, points=pts, draws=idx, return_clamped=True)
    mu = ps.sample_posterior(X, idx, None)
    fn = lik.compiled().host_function()
    from pymc_bart_amd.compiled import CompiledContext
    import ctypes as C

    want = np.empty((D, N))
    rows = np.arange(N, dtype=np.int64)
    clamp = np.vectorize(host.lib().pw_clamp)
    for d in range(D):
        ctx = CompiledContext()
        ctx.aux = aux.ctypes.data
        ctx.params[0], ctx.params[1] = float(pts["s"][d]), float(pts["t"][d])
        raw = np.empty(N)
        m = np.ascontiguousarray(mu[d, 0])
        assert fn(C.cast(C.pointer(ctx), C.c_void_p), rows.ctypes.data_as(C.POINTER(C.c_int64)),
                  y.ctypes.data_as(C.POINTER(C.c_double)), m.ctypes.data_as(C.POINTER(C.c_double)), N,
                  raw.ctypes.data_as(C.POINTER(C.c_double))) == 0
        want[d] = clamp(raw)
    assert np.array_equal(got, want) and nc == 0
    s = log_predictive_density(ps, X, y, lik, points=pts, draws=idx)
    assert np.array_equal(np.stack([s["lppd_i"], s["mean_i"], s["p_waic_i"]]), host.reduce(got))
    # K = 2, with an offset
    lik2 = CompiledLikelihood(TWO, params={"w": 0.25}, aux=aux, n_outputs=2)
    p2, _ = _fit(X, y, lik2, hip, K=2, sigma=1.0)
    off = rng.normal(0, 0.2, (2, N))
    got2 = pointwise_log_likelihood(p2, X, y, lik2, offset=off, draws=idx)
    mu2 = p2.sample_posterior(X, idx, None)
    ev = lik2.compiled()
    assert np.array_equal(got2, np.stack([ev.host_eval(y, mu2[d] + off, aux, [0.25]) for d in range(D)]))
    # refusals, before a launch, naming both sides
    lik._builds[(64, False, True)] = compile_loglik(CENSORED, ["s", "t"])               # a sampler's pass kernel
    with pytest.raises(_abi.PGBError, match="built without pointwise=True.*takes one built with pointwise=True"):
        pointwise_log_likelihood(ps, X, y, lik, points=pts, draws=idx)
    lik._builds[(64, False, True)] = compile_loglik(
        "return -(y - mu[0]) * (y - mu[0]) - fabs(mu[1]) * s * t;", ["s", "t"], n_outputs=2, pointwise=True)   # another K
    with pytest.raises(_abi.PGBError, match="compiled for 2 outputs, the trees have n_outputs = 1"):
        pointwise_log_likelihood(ps, X, y, lik, points=pts, draws=idx)
    lik._builds[(64, False, True)] = compile_loglik(CENSORED, ["s", "t", "u"], pointwise=True)      # other params
    with pytest.raises(_abi.PGBError, match="compiled for 3 params, the call gives n_params = 2"):
        pointwise_log_likelihood(ps, X, y, lik, points=pts, draws=idx)
    del lik._builds[(64, False, True)]
    assert np.array_equal(pointwise_log_likelihood(ps, X, y, lik, points=pts, draws=idx), got)  # (still usable)


# ------------------------------------------------------------------ 4. two chains
def test_two_chains_equal_the_per_chain_matrices_stacked(hip):
    rng, X, f = _data(11)
    y = f + rng.normal(0, 0.5, N)
    lik = NormalLikelihood("sigma")
    op = BARTOp(X, y, m=M)
    chains = [sample_chain(op, 8, DRAWS, random_seed=2, chain=c, backend=hip, keep_draws=False) for c in (0, 1)]
    attach_history(op, chains)
    multi = _get_posterior_sampler(op, backend=hip)
    assert multi.n_draws == 2 * DRAWS
    sig = np.concatenate([c["sigma"] for c in chains])
    got = pointwise_log_likelihood(multi, X, y, lik, points={"sigma": sig})
    parts = []
    for c in chains:
        base, batches = c["history"]
        ps = PosteriorSampler.from_history(batches, base, M, 1, backend=hip)
        parts.append(pointwise_log_likelihood(ps, X, y, lik, points={"sigma": c["sigma"]}))
    assert got.shape == (2 * DRAWS, N) and np.array_equal(got, np.concatenate(parts))
    idx = [DRAWS + 2, 1, DRAWS - 1, DRAWS]                             # across the chain boundary
    assert np.array_equal(pointwise_log_likelihood(multi, X, y, lik, points={"sigma": sig[idx]}, draws=idx), got[idx])
    s = log_predictive_density(multi, X, y, lik, points={"sigma": sig})
    assert np.array_equal(np.stack([s["lppd_i"], s["mean_i"], s["p_waic_i"]]), host.reduce(got))


# ------------------------------------------------------------------ 5. the clamp is counted
def test_the_clamp_is_counted(hip):
    rng, X, f = _data(12)
    y = f + rng.normal(0, 0.5, N)
    ps, _ = _fit(X, y, NormalLikelihood("sigma"), hip)
    lik = NormalLikelihood(1e-3)                                       # residuals of 0.5 against sigma = 1e-3: input data
    idx = list(range(DRAWS))
    got, nc = pointwise_log_likelihood(ps, X, y, lik, return_clamped=True)
    want, nc_host = _host_matrix(ps, lik, X, y, idx, None)
    assert np.array_equal(got, want)
    assert nc == nc_host == int((got == -2047.0).sum()) and nc > DRAWS * N // 2
    assert log_predictive_density(ps, X, y, lik)["n_clamped"] == nc


# ------------------------------------------------------------------ 6. one tie to independent arithmetic
def test_normal_lppd_against_numpy_and_scipy(hip):
    rng, X, f = _data(13)
    y = f + rng.normal(0, 0.5, N)
    lik = NormalLikelihood("sigma")
    ps, res = _fit(X, y, lik, hip)
    _, Xh, fh = _data(14, n=2000)
    yh = fh + np.random.default_rng(15).normal(0, 0.5, 2000)          # held-out rows
    s = log_predictive_density(ps, Xh, yh, lik, points={"sigma": res["sigma"]})
    mu = ps.sample_posterior(Xh, list(range(DRAWS)), None)[:, 0, :]
    ll = stats.norm.logpdf(yh[None, :], mu, res["sigma"][:, None])
    want = special.logsumexp(ll, axis=0) - np.log(DRAWS)
    bound = (DRAWS + 16) * 2.3e-16 * (1.0 + np.abs(want))
    err = np.abs(s["lppd_i"] - want)
    print(f"lppd_i max error / bound = {np.max(err / bound):.3f}; lppd = {s['lppd']:.6f} (SciPy {want.sum():.6f})")
    assert np.all(err <= bound)
    assert abs(s["lppd"] - want.sum()) <= bound.sum()
    L = ll.astype(np.longdouble)
    v2 = np.asarray(((L - L.mean(axis=0)) ** 2).sum(axis=0) / (DRAWS - 1), float)
    m2 = np.asarray(L.mean(axis=0), float)
    ok = v2 >= 0.01
    tol = 8 * DRAWS * 2.0 ** -53 * (1.0 + m2 * m2 / np.where(ok, v2, 1.0))
    rel = np.abs(s["p_waic_i"] - v2) / np.where(ok, v2, 1.0)
    print(f"p_waic_i: {int(ok.sum())} rows with var >= 0.01, max error / bound = {np.max((rel / tol)[ok]) if ok.any() else 0.0:.3f}")
    assert np.all(rel[ok] <= tol[ok])
    assert s["n_clamped"] == 0 and s["elpd_waic"] < s["lppd"]
