"""Chain diagnostics on the MI355X: ``k_chain_diag`` through ``pgb_chain_diag`` against the host build of the same
header (``tests/_diag_host.py``) -- bit for bit on all 10 outputs, on synthetic matrices at every shape and tile edge
and for every kind of column -- the refusals of the entry point, and the public calls end to end on short real chains.

"Bit for bit" is the 64-bit pattern of every output that is a number; a NaN on both sides counts as equal (the sign
and payload of a NaN an operation GENERATES are the hardware's, not the contract's)."""
import math

import numpy as np
import pytest

import _diag_host as host
from pymc_bart_amd import (BARTOp, CategoricalLikelihood, NormalLikelihood, _abi, convergence, diagnose_matrix, diagnostics,
                           loo, pointwise_log_likelihood, relative_efficiency)
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.loo import tail_length
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler, _MultiChainSampler
from test_diag import KINDS, SHAPES, loglik_matrix, matrix

pytestmark = pytest.mark.gpu

N_COLS = (1, 7, 8, 9, 33)   # a tile holds up to 8 columns: below, at and above it, and several tiles


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)


def same(got: np.ndarray, want: np.ndarray) -> bool:
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


def device(hip, a, n_chains, n_cols, transform="identity", stats=host.ALL, n_per_chain=None, ld=None, z="table",
           tau_floor=None):
    """pgb_chain_diag on the first n_cols columns of the device copy of a -> (rc, out (10, n_cols), guard)."""
    mem, lib = hip.mem, hip.lib
    npc = a.shape[0] // n_chains if n_per_chain is None else n_per_chain
    S = 2 * n_chains * (npc // 2)
    if isinstance(z, str):
        z = diagnostics.z_table(S) if stats == host.ALL else None
    if tau_floor is None:
        tau_floor = 1.0 / math.log10(S)
    md = mem.from_host(np.ascontiguousarray(a))
    od = mem.from_host(np.full(10 * max(n_cols, 1) + 8, -7.0))
    code = transform if isinstance(transform, int) else host.TRANSFORMS[transform]
    rc = lib.chain_diag_entry_point()(mem.ptr(md), n_chains, npc, n_cols, a.shape[1] if ld is None else ld, code, stats,
                                      None if z is None else z.ctypes.data, tau_floor, mem.ptr(od), mem.stream_ptr)
    out = mem.to_host(od)
    return rc, out[:10 * n_cols].reshape(10, n_cols), out[10 * n_cols:]


def check(hip, a, n_chains, n_cols, transform="identity", stats=host.ALL, what=None):
    rc, out, guard = device(hip, a, n_chains, n_cols, transform, stats)
    assert rc == 0, what
    want = host.columns(a[:, :n_cols], n_chains, transform, stats)
    bad = [host.ROWS[r] for r in range(10) if not same(out[r], want[r])]
    assert not bad, (what, "outputs that differ", bad)
    assert np.all(guard == -7.0), what                       # nothing written beyond [10][n_cols]
    return out


# ------------------------------------------------------------------ 1. every shape, every kind of column
@pytest.mark.parametrize("shape", SHAPES)
def test_device_equals_the_host_header_at_every_shape(shape, hip):
    nc, n = shape
    for n_cols in N_COLS:
        shifts = range(len(KINDS)) if n_cols == 1 else ((0, 5) if n_cols < len(KINDS) else (0,))   # (every kind everywhere)
        for shift in shifts:
            a = matrix(nc, n, n_cols, n_cols + 5, shift, seed=1000 * nc + 10 * n + n_cols)
            check(hip, a, nc, n_cols, what=(shape, n_cols, shift))
        a = matrix(nc, n, n_cols, n_cols, 3, seed=n_cols)                                          # ld == n_cols
        check(hip, a, nc, n_cols, what=(shape, n_cols, "dense"))
        out = check(hip, a, nc, n_cols, stats=host.MEAN_ONLY, what=(shape, n_cols, "mean only"))
        assert not out[:5].any() and not out[9].any()


@pytest.mark.parametrize("shape", SHAPES)
def test_exp_shift_on_log_likelihoods(shape, hip):
    nc, n = shape
    a = np.full((nc * n, 14), 7.0e77)
    a[:, :9] = loglik_matrix(nc, n, 9, seed=31 * n + nc)
    assert a[:, :9].min() >= -2047.0 and a[:, :9].max() <= 0.0
    for stats in (host.ALL, host.MEAN_ONLY):
        check(hip, a, nc, 9, "exp_shift", stats, what=(shape, stats))


def test_the_caps(hip):
    """S = 8192 with every statistic (128 KiB of dynamic LDS; the random walk runs Geyer's loop to h - 3) and S = 16384
    mean only."""
    nc, n = 4, 2048
    assert host.kept(nc, n) == host.max_draws()
    a = matrix(nc, n, 1, 3, KINDS.index("walk"), seed=8192)
    check(hip, a, nc, 1, what="S = 8192")
    nc, n = 8, 2048
    assert host.kept(nc, n) == host.max_draws_mean()
    a = np.full((nc * n, 2), 7.0e77)
    a[:, :1] = loglik_matrix(nc, n, 2, seed=16384)[:, 1:]
    check(hip, a, nc, 1, "exp_shift", host.MEAN_ONLY, what="S = 16384")


def test_permuting_whole_chains_changes_no_bit_on_the_device(hip):
    nc, n = 4, 65
    a = matrix(nc, n, 10, 10, 0, seed=65)
    _, one, _ = device(hip, a, nc, 10)
    b = a.reshape(nc, n, -1)[[2, 0, 3, 1]].reshape(a.shape)
    _, two, _ = device(hip, b, nc, 10)
    assert same(one, two)


# ------------------------------------------------------------------ 2. refusals
def test_refusals_before_any_launch(hip):
    a = np.zeros((64, 16))
    tbl = diagnostics.z_table(64)
    ok = dict(n_chains=2, n_per_chain=32, n_cols=16, ld=16, transform=0, stats=host.ALL, z=tbl, tau_floor=0.5)
    for change, msg in ((dict(n_chains=0), r"n_chains must be in \[1, 64\], got 0"),
                        (dict(n_chains=65, n_per_chain=4), r"n_chains must be in \[1, 64\], got 65"),
                        (dict(n_per_chain=3), "at least 4 draws per chain, got n_per_chain = 3"),
                        (dict(n_per_chain=4098), r"at most 8192 kept draws \(all statistics\), 8196 given"),
                        (dict(n_chains=4, n_per_chain=4098, stats=host.MEAN_ONLY),
                         r"at most 16384 kept draws \(mean only\), 16392 given"),
                        (dict(n_cols=0), "n_cols must be >= 1 and ld >= n_cols, got n_cols = 0"),
                        (dict(ld=15), "ld >= n_cols, got n_cols = 16, ld = 15"),
                        (dict(transform=2), "unknown transform 2"), (dict(transform=-1), "unknown transform -1"),
                        (dict(stats=2), "unknown stats 2"), (dict(stats=-1), "unknown stats -1"),
                        (dict(z=None), "z_host is NULL"),
                        (dict(tau_floor=0.0), "tau_floor must be finite and positive, got 0"),
                        (dict(tau_floor=-1.0), "tau_floor must be finite and positive, got -1"),
                        (dict(tau_floor=float("nan")), "tau_floor must be finite and positive, got nan"),
                        (dict(tau_floor=float("inf")), "tau_floor must be finite and positive, got inf")):
        kw = dict(ok, **change)
        rc, out, guard = device(hip, a, kw["n_chains"], kw["n_cols"], kw["transform"], kw["stats"], kw["n_per_chain"], kw["ld"],
                                kw["z"], kw["tau_floor"])
        assert rc == -1, change                                   # PGB_E_INVALID
        with pytest.raises(_abi.PGBError, match=msg):
            hip.lib.check(rc, "pgb_chain_diag")
        assert np.all(out == -7.0) and np.all(guard == -7.0), change
    rc, _, _ = device(hip, a, 2, 16, stats=host.MEAN_ONLY, z=None)    # (mean only takes no table)
    assert rc == 0


# ------------------------------------------------------------------ 3. the public calls
N, P, M_TREES, DRAWS = 40, 3, 5, 16
KEYS = ("rhat", "ess_bulk", "ess_tail", "ess_mean", "mcse_mean", "mean", "sd")


def _data(seed, n=N):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, P))
    f = 2.0 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 1.5 * (X[:, 2] - 0.5)
    return rng, X, f


@pytest.fixture(scope="module")
def normal_fit(hip):
    """Two chains of a Normal fit behind one sampler: 2 x 16 draws."""
    rng, X, f = _data(51)
    y = f + rng.normal(0, 0.5, N)
    op = BARTOp(X, y, m=M_TREES)
    chains = [sample_chain(op, 8, DRAWS, random_seed=2, chain=c, backend=hip, keep_draws=False) for c in (0, 1)]
    attach_history(op, chains)
    return X, y, _get_posterior_sampler(op, backend=hip), np.concatenate([c["sigma"] for c in chains])


@pytest.fixture(scope="module")
def two_output_fit(hip):
    """Two chains of a two-class categorical fit (K = 2)."""
    rng, X, f = _data(52)
    y = (f + rng.normal(0, 0.5, N) > 1.0).astype(np.float64)
    parts = []
    for c in (0, 1):
        op = BARTOp(X, y, m=M_TREES)
        res = sample_chain(op, 8, DRAWS, num_particles=10, random_seed=3, chain=c, backend=hip, keep_draws=False,
                           likelihood=CategoricalLikelihood(2))
        base, batches = res["history"]
        parts.append(PosteriorSampler.from_history(batches, base, M_TREES, 2, backend=hip))
    return X, _MultiChainSampler(parts)


def _expect(res, pred, n_chains, hip, n_per_chain=DRAWS):
    """``res`` == diagnose_matrix of the predictions ``pred`` (D, K, n) of the same draws, and the host header."""
    D, K, n = pred.shape
    flat = pred.reshape(D, K * n)
    want = diagnose_matrix(flat, n_chains, backend=hip)
    ref = host.public(flat, n_chains)
    for key in KEYS:
        assert res[key].shape == (n, K) and same(res[key], want[key].reshape(K, n).T), key
        assert same(want[key], ref[key]), key
    assert res["n_constant"] == want["n_constant"] == ref["n_constant"]
    assert res["n_chains"] == want["n_chains"] == n_chains and res["n_per_chain"] == want["n_per_chain"] == n_per_chain
    assert res["n_high_rhat"] == int(np.sum(res["rhat"] > 1.01))
    assert res["n_low_ess"] == int(np.sum(np.minimum(res["ess_bulk"], res["ess_tail"]) < 100.0 * n_chains))


def test_convergence_equals_diagnose_matrix_of_the_predictions(normal_fit, two_output_fit, hip, monkeypatch):
    X, _, sampler, _ = normal_fit
    X2, multi = two_output_fit
    _, Xbig, _ = _data(53, n=200)
    for ps, rows, K in ((sampler, X, 1), (multi, X2, 2), (sampler, Xbig, 1), (multi, Xbig, 2)):
        assert ps.n_draws == 2 * DRAWS
        pred = np.asarray(ps.sample_posterior(rows, list(range(2 * DRAWS)), None))
        assert pred.shape == (2 * DRAWS, K, rows.shape[0])
        res = convergence(ps, rows)
        _expect(res, pred, 2, hip)
        monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(1 << 16))                # its minimum: blocks of 64 or 128 rows
        again = convergence(ps, rows)
        monkeypatch.delenv("PGB_PW_BLOCK_BYTES")
        for key in KEYS:
            assert same(again[key], res[key]), key
        # the last 8 draws of every chain
        last = convergence(ps, rows, draws_per_chain=8)
        _expect(last, pred.reshape(2, DRAWS, K, -1)[:, DRAWS - 8:].reshape(16, K, -1), 2, hip, n_per_chain=8)
    # an offset shifts the mean and nothing else; excluded covariates are the trees' own
    off = np.random.default_rng(5).normal(0, 1, N)
    base, shifted = convergence(sampler, X), convergence(sampler, X, offset=off)
    for key in KEYS:
        assert same(shifted[key], base[key] + off[:, None] if key == "mean" else base[key]), key
    _expect(convergence(sampler, X, excluded=[1]), np.asarray(sampler.sample_posterior(X, list(range(2 * DRAWS)), [1])), 2, hip)


def test_relative_efficiency_and_loo(normal_fit, hip, monkeypatch):
    X, y, sampler, sigma = normal_fit
    lik = NormalLikelihood("sigma")
    pts = {"sigma": sigma}
    S = 2 * DRAWS
    ll = pointwise_log_likelihood(sampler, X, y, lik, points=pts)
    assert ll.shape == (S, N)
    res = relative_efficiency(sampler, X, y, lik, points=pts)
    want = host.columns(ll, 2, "exp_shift", host.MEAN_ONLY)
    full = diagnose_matrix(ll, 2, transform="exp_shift", backend=hip)
    assert same(res["ess_mean_i"], want[5]) and same(full["ess_mean"], want[5])
    assert same(full["mean"], want[6]) and same(full["sd"], np.sqrt(want[7]))
    assert same(res["reff_i"], np.minimum(want[5] / S, 1.0)) and np.all(res["reff_i"] > 0.0) and np.all(res["reff_i"] <= 1.0)
    assert res["reff"] == float(res["reff_i"].mean()) and res["reff_min"] == float(res["reff_i"].min())
    assert res["n_draws"] == S and res["n_chains"] == 2 and res["n_per_chain"] == DRAWS and res["n_clamped"] == 0
    # blocks of rows: held-out rows, more than one block at the smallest block size
    rng, Xbig, fbig = _data(54, n=200)
    ybig = fbig + rng.normal(0, 0.5, 200)
    one = relative_efficiency(sampler, Xbig, ybig, lik, points=pts)
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(1 << 16))
    two = relative_efficiency(sampler, Xbig, ybig, lik, points=pts)
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES")
    assert same(one["reff_i"], two["reff_i"]) and one["reff"] == two["reff"]
    llbig = pointwise_log_likelihood(sampler, Xbig, ybig, lik, points=pts)
    assert same(one["ess_mean_i"], host.columns(llbig, 2, "exp_shift", host.MEAN_ONLY)[5])
    # the scalar is what loo takes: it enters through the tail length and through nothing else
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        plain = loo(sampler, X, y, lik, points=pts)
        with_reff = loo(sampler, X, y, lik, points=pts, reff=res["reff"])
    assert with_reff["tail_len"] == tail_length(S, res["reff"]) and plain["tail_len"] == tail_length(S, 1.0)
    if with_reff["tail_len"] == plain["tail_len"]:
        for key in ("elpd_loo_i", "pareto_k_i", "lppd_i"):
            assert same(with_reff[key], plain[key]), key
    assert same(with_reff["lppd_i"], plain["lppd_i"])
