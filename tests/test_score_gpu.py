"""Scoring rules of the posterior predictive on the MI355X: ``k_rowscore`` through ``pgb_row_score`` against the host
build of the same header (``tests/_score_host.py``) -- bit for bit, on uploaded matrices at every tile regime of the
kernel and every lane boundary --, against ``pgb_row_summary`` on the same matrix (the two kernels share their load and
sort), the refusals, and ``predictive_scores`` / ``score_matrix`` end to end on short real chains.

"Bit for bit" is the 64-bit pattern of every value, as in ``test_rowsummary_gpu.same``."""
import numpy as np
import pytest

import _score_host as host
from pymc_bart_amd import (BARTOp, CategoricalLikelihood, CompiledLikelihood, NormalLikelihood, NormalMeanScaleLikelihood,
                           PoissonLikelihood, _abi, posterior_predictive, predictive_pit, predictive_scores,
                           predictive_summary, score_matrix)
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler
from test_rowsummary_gpu import device as summary_device
from test_rowsummary_gpu import same

pytestmark = pytest.mark.gpu

SMALL_D = (2, 3, 63, 64, 65, 127, 128, 129)     # the lane boundaries; padding (Dp > D) against none
LARGE_D = (2048, 2049, 4097, 8193, 16384)       # 8 -> 4 -> 2 -> 1 columns per workgroup; the last fills 128 KiB
N_COLS = (1, 7, 9, 19)                          # a partial last workgroup, waves without a column
Q16 = np.array([0.0, 1.0, 0.5, 0.25, 0.03, 0.97, 0.123, 0.75, 0.9, 0.1, 1e-9, 1.0 - 1e-9, 0.3333333333333333, 0.6, 0.05, 0.95])
SENTINEL = -7.0
ARRAYS = ("crps", "crps_fair", "squared_error", "dss", "pit", "n_below", "n_equal", "mean", "sd", "quantiles", "pinball",
          "interval_score", "covered", "mean_pinball", "mean_interval_score", "coverage")
SCALARS = ("n_zero_var", "mean_crps", "se_crps", "rmse", "n_draws")


@pytest.fixture(autouse=True)
def _env(monkeypatch, tmp_path_factory):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit"))


def matrix(D: int, n_cols: int, ld: int, seed: int):
    """(D, ld) and y (n_cols,): column c holds continuous draws, tied integer draws or one constant, and its y lies
    below every draw, above every draw, on a draw (a tie) or between; the columns beyond n_cols hold a value no
    result may show."""
    rng = np.random.default_rng(seed)
    a = np.full((D, ld), 7.0e77)
    y = np.empty(n_cols)
    for c in range(n_cols):
        kind, place = (c + seed) % 3, (c + seed // 3) % 4
        x = (rng.normal(0.0, 2.0, D), rng.poisson(3.0, D).astype(np.float64), np.full(D, float(rng.integers(-3, 4))))[kind]
        a[:, c] = x
        y[c] = (x.min() - 1.5, x.max() + 0.75, x[rng.integers(D)], np.median(x) + 0.123)[place]
    return a, y


def device(hip, a, y, n_cols, q, D=None, ld=None, null=()):
    """pgb_row_score on the first n_cols columns of the device copy of a (D, ld) -> (rc, out (rows, n_cols), guard)."""
    mem, lib = hip.mem, hip.lib
    q = np.ascontiguousarray(q, np.float64)
    rows = 6 + 2 * min(q.size, 16)
    md = mem.from_host(np.ascontiguousarray(a))
    yd = mem.from_host(np.ascontiguousarray(y, np.float64))
    od = mem.from_host(np.full(rows * max(n_cols, 1) + 8, SENTINEL))
    rc = lib.score_entry_point()(None if "a" in null else mem.ptr(md), a.shape[0] if D is None else D, n_cols,
                                 a.shape[1] if ld is None else ld, None if "y" in null else mem.ptr(yd),
                                 None if "q" in null or not q.size else q.ctypes.data, int(q.size),
                                 None if "out" in null else mem.ptr(od), mem.stream_ptr)
    out = mem.to_host(od)
    cut = rows * max(n_cols, 1)
    return rc, out[:cut].reshape(rows, -1), out[cut:]


# ------------------------------------------------------------------ 1. every shape
@pytest.mark.parametrize("D", SMALL_D + LARGE_D)
def test_device_equals_the_host_header_at_every_shape(D, hip):
    for n_cols in N_COLS:
        a, y = matrix(D, n_cols, n_cols + 3, seed=D + n_cols)
        for q in (np.array([]), np.array([0.9]), Q16):
            rc, out, guard = device(hip, a, y, n_cols, q)
            what = (D, n_cols, q.size)
            assert rc == 0, what
            want = host.columns(a[:, :n_cols], y, q)
            bad = [r for r in range(out.shape[0]) if not same(out[r], want[r])]
            assert not bad, (what, "output rows that differ", bad)
            assert np.all(guard == SENTINEL), what                       # nothing written beyond [rows][n_cols]


def test_permuting_the_draws_changes_no_bit_on_the_device(hip):
    rng = np.random.default_rng(11)
    for D in (129, 2049):
        a, y = matrix(D, 9, 12, seed=3 * D)
        _, one, _ = device(hip, a, y, 9, Q16)
        _, two, _ = device(hip, a[rng.permutation(D)], y, 9, Q16)
        assert same(one, two)


# ------------------------------------------------------------------ 2. refusals
def test_refusals_before_any_launch(hip):
    a, y = np.zeros((50, 16)), np.zeros(16)
    q = np.array([0.5])
    for D, n, ld, qq, null, msg in ((1, 16, 16, q, (), "at least 2 draws"), (0, 16, 16, q, (), "at least 2 draws"),
                                    (16385, 16, 16, q, (), "pgb_row_score takes at most 16384 draws, 16385 given"),
                                    (50, 16, 15, q, (), "ld >= n_cols"), (50, 0, 16, q, (), "n_cols must be >= 1"),
                                    (50, 16, 16, np.full(17, 0.5), (), r"n_q must be in \[0, 16\], got 17"),
                                    (50, 16, 16, np.array([1.5]), (), r"level 0 must be in \[0, 1\]"),
                                    (50, 16, 16, np.array([0.5, -0.1]), (), r"level 1 must be in \[0, 1\]"),
                                    (50, 16, 16, np.array([np.nan]), (), r"level 0 must be in \[0, 1\]"),
                                    (50, 16, 16, np.array([0.5, 0.5, np.inf]), (), r"level 2 must be in \[0, 1\]"),
                                    (50, 16, 16, q, ("a",), "null argument"), (50, 16, 16, q, ("y",), "null argument"),
                                    (50, 16, 16, q, ("q",), "null argument"), (50, 16, 16, q, ("out",), "null argument")):
        rc, out, guard = device(hip, a, y, n, qq, D=D, ld=ld, null=null)
        assert rc == -1, (D, n, ld, msg)                      # PGB_E_INVALID
        with pytest.raises(_abi.PGBError, match=msg):
            hip.lib.check(rc, "pgb_row_score")
        assert np.all(out == SENTINEL) and np.all(guard == SENTINEL), msg
    rc, out, _ = device(hip, a, y, 16, q, D=50, ld=16)        # (the same call, valid)
    assert rc == 0 and not np.any(out == SENTINEL)


# ------------------------------------------------------------------ 3. the stages shared with k_rowsum
@pytest.mark.parametrize("D", [129, 2049])
def test_mean_var_and_quantiles_are_pgb_row_summarys_bits(D, hip):
    a, y = matrix(D, 19, 22, seed=D)
    rc, out, _ = device(hip, a, y, 19, Q16)
    rc2, summ, _ = summary_device(hip, a, 19, Q16, 0)
    assert rc == 0 and rc2 == 0
    assert same(out[0], summ[0]) and same(out[1], summ[1]) and same(out[6:22], summ[2:18])


# ------------------------------------------------------------------ 4. end to end
N, P, M_TREES, TUNE, DRAWS = 200, 4, 10, 20, 20
QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)


def _data(seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, P))
    f = 2.0 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 1.5 * (X[:, 2] - 0.5) + X[:, 3]
    return rng, X, f


@pytest.fixture(scope="module")
def normal_fit(hip):
    """Two chains of a Normal fit behind one sampler: 2 x 20 pooled draws, sigma per draw."""
    rng, X, f = _data(41)
    y = f + rng.normal(0, 0.5, N)
    op = BARTOp(X, y, m=M_TREES)
    chains = [sample_chain(op, TUNE, DRAWS, random_seed=2, chain=c, backend=hip, keep_draws=False) for c in (0, 1)]
    attach_history(op, chains)
    return X, y, _get_posterior_sampler(op, backend=hip), {"sigma": np.concatenate([c["sigma"] for c in chains])}


def _one_chain(hip, X, y, lik, K):
    op = BARTOp(X, y, m=M_TREES)
    res = sample_chain(op, TUNE, DRAWS, num_particles=10, random_seed=3, chain=0, backend=hip, keep_draws=False, likelihood=lik)
    base, batches = res["history"]
    return PosteriorSampler.from_history(batches, base, M_TREES, K, backend=hip)


def _same_dict(got: dict, want: dict, what=None):
    for key in ARRAYS:
        assert np.shape(got[key]) == np.shape(want[key]) and same(np.asarray(got[key], np.float64),
                                                                  np.asarray(want[key], np.float64)), (what, key)
    for key in SCALARS:
        assert got[key] == want[key], (what, key)


def test_predictive_scores_of_two_pooled_chains(normal_fit, hip, monkeypatch):
    X, y, sampler, points = normal_fit
    lik = NormalLikelihood("sigma")
    kw = dict(points=points, random_seed=7)
    res = predictive_scores(sampler, X, y, lik, **kw)
    yrep = posterior_predictive(sampler, X, lik, **kw)
    assert yrep.shape == (2 * DRAWS, N) and res["n_draws"] == 2 * DRAWS
    assert res["n_capped"] == 0 and res["n_exhausted"] == 0
    _same_dict(res, host.public(yrep, y), "the host header on posterior_predictive's matrix")
    assert res["crps"].shape == (N,) and res["quantiles"].shape == (5, N) and res["interval_score"].shape == (2, N)
    assert np.all(res["crps"] >= 0.0) and np.all(res["crps_fair"] <= res["crps"]) and res["covered"].dtype == bool
    pit = predictive_pit(sampler, X, y, lik, **kw)
    assert np.array_equal(res["n_below"], pit["n_below"]) and np.array_equal(res["n_equal"], pit["n_equal"])
    assert np.array_equal(res["pit"], pit["pit"])
    summ = predictive_summary(sampler, X, lik, quantiles=QUANTILES, **kw)
    assert same(res["mean"], summ["mean"]) and same(res["sd"], summ["sd"]) and same(res["quantiles"], summ["quantiles"])
    # score_matrix on the host matrix: the same dict
    again = score_matrix(yrep, y, backend=hip)
    _same_dict(again, res, "score_matrix")
    assert set(res) - set(again) == {"n_capped", "n_exhausted"}
    # an offset, a subset of the draws with a repeat, other levels
    idx = [DRAWS + 2, 1, 1, DRAWS - 1, 5]
    off = np.random.default_rng(5).normal(0, 0.3, N)
    kw2 = dict(points={"sigma": points["sigma"][idx]}, draws=idx, offset=off, random_seed=8)
    sub = predictive_scores(sampler, X, y, lik, quantiles=(0.5,), intervals=(0.8,), **kw2)
    _same_dict(sub, host.public(posterior_predictive(sampler, X, lik, **kw2), y, (0.5,), (0.8,)), "a subset")
    # several blocks of rows
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(1 << 16))
    _same_dict(predictive_scores(sampler, X, y, lik, **kw), res, "blocks")
    _same_dict(score_matrix(yrep, y, backend=hip), res, "score_matrix in blocks")


def test_a_poisson_fit_with_ties(hip):
    rng, X, f = _data(43)
    y = rng.poisson(np.exp(0.5 * f)).astype(float)
    lik = PoissonLikelihood()
    ps = _one_chain(hip, X, y, lik, 1)
    res = predictive_scores(ps, X, y, lik, random_seed=3)
    yrep = posterior_predictive(ps, X, lik, random_seed=3)
    assert np.array_equal(yrep, np.round(yrep)) and np.any(res["n_equal"] > 1)
    _same_dict(res, host.public(yrep, y), "poisson")


def test_a_compiled_normal_body_scores_as_the_built_in_family(normal_fit, hip):
    X, y, sampler, points = normal_fit
    body = CompiledLikelihood("double z = (y - mu) / s; return -0.5 * z * z - log(s);", {"s": "sigma"},
                              sampler="return mu + s * normal();")
    res = predictive_scores(sampler, X, y, body, points=points, random_seed=7)
    _same_dict(res, host.public(posterior_predictive(sampler, X, body, points=points, random_seed=7), y), "compiled")
    _same_dict(res, predictive_scores(sampler, X, y, NormalLikelihood("sigma"), points=points, random_seed=7), "built in")


def test_a_mean_scale_fit_has_one_replicate_per_row(hip):
    rng, X, f = _data(44)
    y = f + rng.normal(0, 0.5, N)
    lik = NormalMeanScaleLikelihood()
    ps = _one_chain(hip, X, y, lik, 2)
    res = predictive_scores(ps, X, y, lik, random_seed=5)
    yrep = posterior_predictive(ps, X, lik, random_seed=5)
    assert yrep.shape == (DRAWS, N) and res["crps"].shape == (N,)
    _same_dict(res, host.public(yrep, y), "mean/scale")


def test_a_categorical_fit_is_refused(hip):
    rng, X, f = _data(42)
    y = np.minimum((f + rng.normal(0, 0.5, N)).clip(0) // 1.2, 2.0)
    lik = CategoricalLikelihood(3)
    ps = _one_chain(hip, X, y, lik, 3)
    with pytest.raises(ValueError, match="class labels have no order.*log_predictive_density"):
        predictive_scores(ps, X, y, lik)
