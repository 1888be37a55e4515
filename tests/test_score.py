"""Scoring rules of the posterior predictive on the build box (no GPU): the contract of ``include/pgbart_score.h``
through its host build (``tests/_score_host.py``) against NumPy written from the definitions, the exact cases, the
host arithmetic of ``pymc_bart_amd/scores.py`` against hand numbers, the calls a block makes (on the recording
backend) and the refusals.

Tolerances.  ``abs_err``, ``pair_sum / D^2`` and ``crps`` against the O(D^2) definition: ``1e-10 max(1, |value|)`` -- a
lane sum of D non-negative terms is off by at most about ``(D + 3) 2^-53`` relative, 2e-12 at the largest D the
contract takes, and NumPy's pairwise sums are no worse.  A quantile against ``np.quantile``: both interpolate once
between the same two neighbours, in differently rounded forms, each within 3 ulp of the larger neighbour:
``16 EPS max(1, max |t|)``.  Everything else is exact."""
import os
import subprocess

import numpy as np
import pytest

import _rowsummary_host as rowsum
import _score_host as host
from _recording_backend import Recorder
from pymc_bart_amd import (CategoricalLikelihood, CompiledLikelihood, NormalLikelihood, _abi, compiled, predictive_scores,
                           score_matrix, scores)
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
DS = (2, 3, 64, 65, 129, 1025)
KINDS = ("normal", "shifted", "poisson", "constant")
LEVELS = np.array([0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0, 0.123])


def draws(kind: str, D: int, rng) -> np.ndarray:
    if kind == "normal":
        return rng.normal(0.0, 1.0, D)
    if kind == "shifted":
        return rng.normal(0.0, 1.0, D) + 1.0e3
    if kind == "poisson":
        return rng.poisson(3.0, D).astype(np.float64)
    return np.full(D, 2.5)


def ys(x: np.ndarray, rng) -> list:
    """Below every draw, above every draw, on a draw (a tie for the integer kinds) and between."""
    return [float(x.min() - 1.5), float(x.max() + 0.75), float(x[rng.integers(x.size)]), float(np.median(x) + 0.123)]


def close(got, want):
    return abs(got - want) <= 1e-10 * max(1.0, abs(want))


# ------------------------------------------------------------------ 1. the header against the definition
@pytest.mark.parametrize("D", DS)
def test_header_against_numpy(D):
    rng = np.random.default_rng(100 + D)
    for kind in KINDS:
        x = draws(kind, D, rng)
        t = np.sort(x)
        for y in ys(x, rng):
            got = host.column(x, y, LEVELS)
            what = (D, kind, y)
            abs_err = np.mean(np.abs(t - y))
            half_pair = 0.5 * np.mean(np.abs(t[:, None] - t[None, :]))
            assert close(got["abs_err"], abs_err), what
            assert close(got["pair_sum"] / (D * D), half_pair), what
            assert close(got["abs_err"] - got["pair_sum"] / (D * D), abs_err - half_pair), what
            assert got["n_below"] == np.sum(t < y) and got["n_equal"] == np.sum(t == y), what
            # mean, var and the quantiles: pgb_row_summary's bits
            ref = rowsum.summary(x[:, None], LEVELS)[:, 0]
            assert got["mean"].tobytes() == ref[0].tobytes() and got["var"].tobytes() == ref[1].tobytes(), what
            assert got["q"].tobytes() == ref[2:2 + LEVELS.size].tobytes(), what
            assert np.all(np.abs(got["q"] - np.quantile(t, LEVELS)) <= 16 * EPS * max(1.0, np.abs(t).max())), what
            u = y - got["q"]
            assert np.array_equal(got["pinball"], np.where(u >= 0, LEVELS * u, (LEVELS - 1.0) * u)), what
            assert np.all(got["pinball"] >= 0.0), what


# ------------------------------------------------------------------ 2. exact cases
def test_a_constant_column():
    # (values with few mantissa bits: D |c - y| is exact in every partial sum, so the mean of D of them is |c - y| itself)
    for D in (2, 65, 1025):
        for c, y in ((2.5, 4.0), (-1.0e3, -1.0e3), (0.125, -7.25)):
            got = host.column(np.full(D, c), y, [0.5])
            assert got["pair_sum"] == 0.0 and got["var"] == 0.0 and got["mean"] == c
            assert got["abs_err"] - got["pair_sum"] / (D * D) == abs(c - y)
            assert got["q"][0] == c and got["pinball"][0] == abs(c - y) / 2


def test_y_outside_the_draws_and_on_a_tie():
    rng = np.random.default_rng(4)
    for D in (3, 64, 129):
        x = rng.poisson(3.0, D).astype(np.float64)
        assert host.column(x, x.min() - 1.0)["n_below"] == 0 and host.column(x, x.min() - 1.0)["n_equal"] == 0
        above = host.column(x, x.max() + 1.0)
        assert above["n_below"] == D and above["n_equal"] == 0
        v = float(np.bincount(x.astype(int)).argmax())
        tie = host.column(x, v)
        assert tie["n_equal"] == np.sum(x == v) and tie["n_below"] == np.sum(x < v)
        assert D < 64 or tie["n_equal"] > 1


def test_both_zeros_are_equal_to_zero():
    x = np.array([-0.0, 0.0, 1.0, -1.0, 0.0, -0.0, 2.0])
    for y in (0.0, -0.0):
        got = host.column(x, y)
        assert got["n_equal"] == 4 and got["n_below"] == 1


def test_two_draws():
    for a, b in ((1.0, 4.5), (4.5, 1.0), (-3.0, -3.0), (-0.0, 0.0)):
        got = host.column(np.array([a, b]), 0.3)
        assert got["pair_sum"] == max(a, b) - min(a, b)


@pytest.mark.parametrize("D", [3, 65, 129, 1025])
def test_permuting_the_draws_changes_no_bit(D):
    rng = np.random.default_rng(D)
    a = np.stack([draws(KINDS[c % 3], D, rng) for c in range(6)], axis=1)
    a[rng.permutation(D)[:D // 2], 0] = 0.25
    y = a[rng.integers(0, D, 6), np.arange(6)]
    one = host.columns(a, y, LEVELS)
    for _ in range(3):
        assert host.columns(a[rng.permutation(D)], y, LEVELS).tobytes() == one.tobytes()
    assert host.columns(np.sort(a, axis=0)[::-1], y, LEVELS).tobytes() == one.tobytes()


# ------------------------------------------------------------------ 3. the host arithmetic, by hand
T4 = np.array([4.0, 1.0, 7.0, 2.0])


def _result(y, quantiles, intervals):
    lev = scores.Levels(quantiles, intervals)
    yy = np.atleast_1d(np.asarray(y, np.float64))
    a = np.tile(T4[:, None], (1, yy.size))
    return scores.result(host.columns(a, yy, lev.all), yy, 4, lev), lev


def test_level_merging():
    lev = scores.Levels((0.25, 0.5), (0.5,))
    assert lev.all.tolist() == [0.25, 0.5, 0.75] and lev.ends.tolist() == [[0, 2]] and lev.n_out == 12
    lev = scores.Levels((0.05, 0.25, 0.5, 0.75, 0.95), (0.5, 0.9))
    assert lev.all.tolist() == [0.05, 0.25, 0.5, 0.75, 0.95, (1.0 - 0.9) / 2.0] and lev.ends.tolist() == [[1, 3], [5, 4]]
    lev = scores.Levels(None, (0.5, 0.5, 0.8))
    assert lev.all.tolist() == [0.25, 0.75, (1.0 - 0.8) / 2.0, 0.9] and lev.ends.tolist() == [[0, 1], [0, 1], [2, 3]]
    assert lev.q.size == 0 and scores.Levels((), None).all.size == 0
    got, want = host.merged_levels((0.05, 0.25, 0.5, 0.75, 0.95), (0.5, 0.9)), scores.Levels(scores.DEFAULT_QUANTILES,
                                                                                            scores.DEFAULT_INTERVALS)
    assert np.array_equal(got[0], want.all) and np.array_equal(got[1], want.ends)


def test_scores_of_four_draws_by_hand():
    # t = 1, 2, 4, 7: sum |t - 3| = 8; the pairs: 1 + 3 + 6 + 2 + 5 + 3 = 20 = 3 * 1 + 4 * 2 + 3 * 3
    res, lev = _result([3.0, 6.0, 0.0, 5.0], (0.25, 0.5), (0.5,))
    assert lev.all.tolist() == [0.25, 0.5, 0.75]
    assert res["crps"][0] == 2.0 - 20.0 / 16.0 and res["crps_fair"][0] == 2.0 - 20.0 / 12.0
    assert np.array_equal(res["mean"], np.full(4, 3.5)) and np.array_equal(res["sd"], np.full(4, np.sqrt(7.0)))
    assert res["squared_error"].tolist() == [0.25, 6.25, 12.25, 2.25] and res["rmse"] == np.sqrt(21.0 / 4.0)
    assert res["dss"][0] == 0.25 / 7.0 + np.log(7.0) and res["n_zero_var"] == 0
    assert res["n_below"].tolist() == [2, 3, 0, 3] and res["n_equal"].tolist() == [0, 0, 0, 0]
    assert res["pit"].tolist() == [0.5, 0.75, 0.0, 0.75] and res["n_below"].dtype == np.int64
    # the quartiles 1.75 and 4.75, the median 3
    assert res["quantiles"].shape == (2, 4) and res["quantiles"][:, 0].tolist() == [1.75, 3.0]
    assert res["pinball"][1].tolist() == [0.0, 1.5, 1.5, 1.0]                       # |median - y| / 2
    assert res["pinball"][0].tolist() == [0.25 * 1.25, 0.25 * 4.25, 0.75 * 1.75, 0.25 * 3.25]
    # width 3; y = 6 is 1.25 above, y = 0 is 1.75 below, y = 5 is 0.25 above; 2 / alpha = 4
    assert res["interval_score"].tolist() == [[3.0, 8.0, 10.0, 4.0]] and res["covered"].tolist() == [[True, False, False, False]]
    assert res["coverage"].tolist() == [0.25] and res["mean_interval_score"].tolist() == [6.25]
    assert res["mean_pinball"].tolist() == [np.mean(res["pinball"][0]), 1.0]
    assert res["mean_crps"] == np.mean(res["crps"]) and res["se_crps"] == np.std(res["crps"]) / 2.0
    assert res["n_draws"] == 4 and res["q"].tolist() == [0.25, 0.5] and res["intervals"].tolist() == [0.5]
    # y on an end of the interval is covered; a column of equal draws has no finite Dawid-Sebastiani score
    on, _ = _result([1.75, 4.75], (), (0.5,))
    assert on["covered"].tolist() == [[True, True]] and on["interval_score"].tolist() == [[3.0, 3.0]]
    assert on["quantiles"].shape == (0, 2) and on["pinball"].shape == (0, 2) and on["mean_pinball"].shape == (0,)
    lev = scores.Levels((0.5,), ())
    y = np.array([2.5, 1.0])
    flat = scores.result(host.columns(np.full((4, 2), 2.5), y, lev.all), y, 4, lev)
    assert np.all(np.isinf(flat["dss"])) and flat["n_zero_var"] == 2 and flat["crps"].tolist() == [0.0, 1.5]
    assert flat["interval_score"].shape == (0, 2) and flat["coverage"].shape == (0,)


def test_the_restated_arithmetic_of_the_shim_is_the_modules():
    rng = np.random.default_rng(8)
    a = np.stack([draws(KINDS[c % 4], 65, rng) for c in range(9)], axis=1)
    y = np.array([ys(a[:, c], rng)[c % 4] for c in range(9)])
    lev = scores.Levels(scores.DEFAULT_QUANTILES, scores.DEFAULT_INTERVALS)
    got, want = scores.result(host.columns(a, y, lev.all), y, 65, lev), host.public(a, y)
    for key, w in want.items():
        g = got[key]
        assert (np.asarray(g).tobytes() == np.asarray(w).tobytes() and np.shape(g) == np.shape(w)) if isinstance(w, np.ndarray) \
            else g == w, key
    assert set(got) - set(want) == {"q", "intervals"}


# ------------------------------------------------------------------ 4. the Python surface
M_TREES, N_DRAWS = 3, 5


def _fit(backend, draws=N_DRAWS, K=1):
    pool = TreeArrays.empty(M_TREES, M_TREES, K)                      # stumps
    pool.tree_id[:] = np.arange(M_TREES)
    pool.node_off[:] = np.arange(M_TREES + 1)
    pool.var[:] = -1
    pool.count[:] = 10
    return PosteriorSampler(pool, np.tile(np.arange(M_TREES, dtype=np.int32), (draws, 1)), M_TREES, K, backend=backend)


def _recorder():
    rec = Recorder()
    rec.lib.score_entry_point = lambda: rec.function("pgb_row_score")
    return rec


def test_refusals_come_before_a_backend_is_touched():
    rec = _recorder()
    s = _fit(rec)
    X, y = np.zeros((8, 2)), np.zeros(8)
    lik = NormalLikelihood(1.0)
    with pytest.raises(ValueError, match="at most 16 levels per call.*got 17"):
        predictive_scores(s, X, y, lik, quantiles=np.linspace(0.0, 1.0, 15), intervals=(0.9,))
    with pytest.raises(ValueError, match="at most 16 levels per call.*got 17"):
        score_matrix(np.zeros((4, 8)), y, quantiles=np.linspace(0.0, 1.0, 15), intervals=(0.9,))
    predictive_scores(s, X, y, lik, quantiles=np.linspace(0.0, 1.0, 15) / 2.0, intervals=(0.5,))     # 15 + 0.75: taken
    assert rec.trace and not rec.trace.clear()
    for bad in (0.0, 1.0, -0.5, 1.5, np.nan):
        with pytest.raises(ValueError, match=r"the mass of a central interval must be in \(0, 1\)"):
            predictive_scores(s, X, y, lik, intervals=(0.5, bad))
        with pytest.raises(ValueError, match=r"the mass of a central interval must be in \(0, 1\)"):
            score_matrix(np.zeros((4, 8)), y, intervals=(bad,))
    for bad in (1.5, -0.1, np.nan):
        with pytest.raises(ValueError, match=r"quantiles must be in \[0, 1\]"):
            predictive_scores(s, X, y, lik, quantiles=[0.5, bad])
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="y must be finite"):
            predictive_scores(s, X, np.where(np.arange(8) == 3, bad, 0.0), lik)
        with pytest.raises(ValueError, match="y must be finite"):
            score_matrix(np.zeros((4, 8)), np.where(np.arange(8) == 3, bad, 0.0))
        with pytest.raises(ValueError, match="y_rep must be finite"):
            score_matrix(np.where(np.arange(32).reshape(4, 8) == 9, bad, 0.0), y)
    with pytest.raises(ValueError, match="y must hold one value per row"):
        predictive_scores(s, X, np.zeros(7), lik)
    with pytest.raises(ValueError, match="y must hold one value per row"):
        score_matrix(np.zeros((4, 8)), np.zeros(7))
    with pytest.raises(ValueError, match="class labels have no order.*log_predictive_density"):
        predictive_scores(_fit(rec, K=3), X, y, CategoricalLikelihood(3))
    density = "double z = (y - mu) / s; return -0.5 * z * z - log(s);"
    with pytest.raises(ValueError, match="the compiled family has a log density only, no sampler"):
        predictive_scores(s, X, y, CompiledLikelihood(density, {"s": 1.0}))
    with pytest.raises(ValueError, match="at least 2 draws, got 1"):
        predictive_scores(_fit(rec, draws=1), X, y, lik)
    with pytest.raises(ValueError, match="at least 2 draws, got 1"):
        predictive_scores(s, X, y, lik, draws=[3])
    with pytest.raises(ValueError, match="at least 2 draws, got 1"):
        score_matrix(np.zeros((1, 8)), y)
    with pytest.raises(ValueError, match="at most 16384 draws, got 16385"):
        predictive_scores(s, X, y, lik, draws=np.zeros(scores.MAX_DRAWS + 1, int))
    with pytest.raises(ValueError, match="at most 16384 draws, got 16385"):
        score_matrix(np.zeros((scores.MAX_DRAWS + 1, 1)), np.zeros(1))
    with pytest.raises(ValueError, match="matrix"):
        score_matrix(np.zeros(8), y)
    with pytest.raises(ValueError, match="no draws"):
        predictive_scores(s, X, y, lik, draws=[])
    with pytest.raises(TypeError, match="sampler must be"):
        predictive_scores(object(), X, y, lik)
    assert rec.trace == []
    assert scores.MAX_DRAWS == rowsum.max_draws() and scores.MAX_LEVELS == rowsum.max_q() and host.nout(16) == 6 + 32


def test_a_backend_that_is_not_hip_is_refused():
    from _oracle import oracle_backend

    be = oracle_backend()
    with pytest.raises(NotImplementedError, match="pgb_row_score"):
        score_matrix(np.zeros((10, 4)), np.zeros(4), backend=be)
    with pytest.raises(NotImplementedError, match="pgb_row_score"):
        predictive_scores(_fit(be), np.zeros((8, 2)), np.zeros(8), NormalLikelihood(1.0))
    rec = _recorder()
    rec.lib.backend_name = "cpu-oracle"                      # (a library with the symbol that is not the HIP one)
    with pytest.raises(_abi.PGBError, match="predictive scores run on the HIP backend only, not on cpu-oracle"):
        predictive_scores(_fit(rec), np.zeros((8, 2)), np.zeros(8), NormalLikelihood(1.0))
    assert rec.trace == []


def test_each_block_predicts_replicates_in_place_and_scores_and_only_the_scores_come_back(monkeypatch):
    n, p = 600, 2
    X, y = np.zeros((n, p)), np.arange(n, dtype=np.float64)
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(1 << 16))
    rec = _recorder()
    res = predictive_scores(_fit(rec), X, y, NormalLikelihood(1.0), random_seed=3)
    rows = 6 + 2 * 6                                                   # the default levels: 5 quantiles and one more end
    per_row = 8 * (p + (N_DRAWS + 1) + rows + 1)
    nb = max(64, (1 << 16) // per_row // 64 * 64)
    blocks = [(r0, min(n, r0 + nb)) for r0 in range(0, n, nb)]
    assert len(blocks) > 1
    calls = [ln for ln in rec.trace if ln.startswith("pgb_")]
    assert [ln.split()[0] for ln in calls] == ["pgb_predict", "pgb_ppc_draw", "pgb_row_score"] * len(blocks)
    back = [ln for ln in rec.trace if ln.startswith("to_host")]
    assert back == [f"to_host {rows * (r1 - r0)}" for r0, r1 in blocks]     # nothing of size draws x rows
    for (r0, r1), draw, score in zip(blocks, calls[1::3], calls[2::3]):
        b = r1 - r0
        md = f"dev:{N_DRAWS * b}+0"
        assert draw.split()[1:7] == [md, str(N_DRAWS), "1", str(b), str(b), str(r0)]
        assert draw.split()[8:11] == ["3", md, str(b)]                     # the seed; in place
        assert score.split()[1:] == [md, str(N_DRAWS), str(b), str(b), f"dev:{b}+0", "host", "6", f"dev:{rows * b}+0", "-"]
    assert res["crps"].shape == (n,) and res["quantiles"].shape == (5, n) and res["interval_score"].shape == (2, n)
    assert res["n_capped"] == 0 and res["n_exhausted"] == 0 and res["n_draws"] == N_DRAWS


# ------------------------------------------------------------------ 5. the library
@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_point(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    assert os.path.exists(path), "run __graft_entry__.build() first"
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    assert " pgb_row_score\n" in syms and "pgb_row_score" not in _abi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "pgbart.h")).read()
    assert "pgb_row_score" not in header


def test_the_kernel_is_budgeted_without_scratch():
    import json

    row = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]["k_rowscore"]
    assert row["max_scratch_bytes"] == 0 and row["max_vgpr_spills"] == 0 and row["min_wgs_per_cu"] >= 2


def test_the_timing_tool_answers_help_and_its_host_baseline_computes_the_same_scores(capsys, monkeypatch):
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import timing_scores as tool

    with pytest.raises(SystemExit) as e:
        tool.main(["--help"])
    assert e.value.code == 0 and capsys.readouterr().out.startswith("usage:")
    assert tool.QUANTILES == scores.DEFAULT_QUANTILES and tool.INTERVALS == scores.DEFAULT_INTERVALS
    assert len(tool.KERNEL_LEVELS) == 7
    # the baseline leg on a matrix given in place of posterior_predictive's: the numbers of the header, within rounding
    rng = np.random.default_rng(2)
    yrep = rng.normal(1.0, 2.0, (65, 40))
    y = rng.normal(1.0, 2.0, 40)
    import pymc_bart_amd

    monkeypatch.setattr(pymc_bart_amd, "posterior_predictive", lambda *a, **kw: yrep)
    crps, mean, var, pit, pinball, iscore = tool.on_the_host(None, None, y, None)
    want = host.public(yrep, y)
    for got, key in ((crps, "crps"), (mean, "mean"), (np.sqrt(var), "sd"), (pinball, "pinball"), (np.array(iscore), "interval_score")):
        assert np.allclose(got, want[key], rtol=1e-12, atol=1e-12), key
    assert np.array_equal(pit, want["pit"])
