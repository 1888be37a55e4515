"""Partial dependence sweeps (``include/pgbart_pdp.h``, ``pymc_bart_amd/pdp.py``) without a GPU: validation, the host
loop of a backend without ``pgb_predict_pdp`` against per-column ``_sample_posterior``, ``partial_dependence`` against
its earlier body restated, the library's export, and the slot argument of the profile route itself -- on the oracle
backend and in the exact arithmetic of ``_predict_exact.walk``."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _pdp_host as host
import _predict_exact as ex
from pymc_bart_amd import BARTOp, _abi, compiled, partial_dependence, pdp_sweep
from pymc_bart_amd.chains import sample_chain
from pymc_bart_amd.partial import pdp_grid
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler, _sample_posterior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1  # PGB_E_INVALID (include/pgbart.h)


@pytest.fixture(scope="module")
def fit(oracle):
    rng = np.random.default_rng(41)
    X = rng.uniform(-1, 1, size=(90, 3))
    Y = 2.0 * X[:, 0] + (X[:, 2] > 0) + rng.normal(0, 0.1, 90)
    op = BARTOp(X, Y, m=8)
    sample_chain(op, tune=20, draws=12, random_seed=5, backend=oracle)
    return op, X, _get_posterior_sampler(op, backend=oracle)


# ------------------------------------------------------------------ 1. validation
def test_refusals_of_pdp_sweep(fit, oracle):
    op, X, s = fit
    one = s._chain_samplers[0]

    def sweep(X=X, cols=(0, 1), picks=((0, 1), (2, 3)), route=0):
        return pdp_sweep(oracle, one.pool, one.forest_idx, one.m, 1, None, X, cols, picks, route)  # (predict is never reached)

    with pytest.raises(ValueError, match="X must be a matrix"):
        sweep(X=np.zeros((0, 3)))
    with pytest.raises(ValueError, match="cols must be a non-empty vector"):
        sweep(cols=[], picks=np.zeros((0, 2), int))
    with pytest.raises(ValueError, match="cols must index the 3 columns"):
        sweep(cols=[0, 3])
    with pytest.raises(ValueError, match="cols must index the 3 columns"):
        sweep(cols=[-1, 0])
    with pytest.raises(ValueError, match=r"picks must have shape \(n_cols, n_picks\) = \(2, n_picks\)"):
        sweep(picks=[[0, 1]])
    with pytest.raises(ValueError, match="picks must have shape"):
        sweep(picks=[0, 1])
    with pytest.raises(ValueError, match="no draws to predict"):
        sweep(picks=np.zeros((2, 0), int))
    with pytest.raises(ValueError, match="picks must index the 12 stored draws"):
        sweep(picks=[[0, 12], [1, 2]])
    with pytest.raises(ValueError, match="picks must index the 12 stored draws"):
        sweep(picks=[[0, -1], [1, 2]])
    for bad in (3, -1, "profile", True):
        with pytest.raises(ValueError, match="route must be 0"):
            sweep(route=bad)
    with pytest.raises(ValueError, match="route must be 0"):
        s.pdp_sweep(X, [0], [[1]], route=7)


def test_keep_pd_false_needs_a_summary(fit, oracle):
    op, X, _ = fit
    with pytest.raises(ValueError, match="keep_pd=False leaves nothing to return without summary="):
        partial_dependence(op, X, samples=5, backend=oracle, keep_pd=False)
    with pytest.raises(_abi.PGBError, match="HIP backend only"):      # (with one: the summaries are the device's)
        partial_dependence(op, X, samples=5, backend=oracle, keep_pd=False, summary={})


# ------------------------------------------------------------------ 2. the host loop and the public function
def test_the_host_loop_is_per_column_sample_posterior(fit):
    op, X, s = fit
    rng, again = np.random.default_rng(7), np.random.default_rng(7)
    cols = [2, 0, 2]
    picks = np.stack([rng.integers(0, s.n_draws, size=6) for _ in cols])
    got = s.pdp_sweep(X, cols, picks)
    assert got.shape == (3, 6, 1, 90)
    for c, j in enumerate(cols):
        want = _sample_posterior(s, X=X, rng=again, size=6, excluded=[v for v in range(3) if v != j])  # (6, 90, 1)
        assert np.array_equal(np.moveaxis(got[c], 1, 2), want), c
    for route in (1, 2):                                               # (a backend without the entry point ignores it)
        assert np.array_equal(s.pdp_sweep(X, cols, picks, route=route), got)
    one = s._chain_samplers[0]
    assert np.array_equal(one.pdp_sweep(X, cols, picks), got) and np.array_equal(host.yardstick(one, X, cols, picks), got)


def test_partial_dependence_is_the_per_covariate_loop(fit, oracle):
    op, X, s = fit
    kw = dict(xs_interval="quantiles", samples=9, random_seed=13, backend=oracle)
    got = partial_dependence(op, X, var_idx=[2, 0], func=lambda a: a + 1.0, **kw)
    rng = np.random.default_rng(13)
    grid = pdp_grid(X, "quantiles", None)
    means = []
    for j in (2, 0):
        want = _sample_posterior(s, X=grid, rng=rng, size=9, excluded=[v for v in range(3) if v != j]) + 1.0
        assert got["pd"][j].shape == (9, 9, 1) and np.array_equal(got["pd"][j], want)
        assert np.array_equal(got["x"][j], grid[:, j]) and got["labels"][j] == f"X_{j}"
        means.append(float(want[:, :, 0].mean()))
    assert got["reference"] == float(np.mean(means)) and list(got["pd"]) == [2, 0]
    empty = partial_dependence(op, X, var_idx=[], **kw)
    assert empty == {"x": {}, "pd": {}, "labels": {}, "reference": None}
    both = partial_dependence([op, op], X, var_idx=[1], **kw)          # a list: the outputs side by side, the same picks
    solo = partial_dependence(op, X, var_idx=[1], **kw)
    assert both["pd"][1].shape == (9, 9, 2)
    assert np.array_equal(both["pd"][1][:, :, 0], solo["pd"][1][:, :, 0]) and np.array_equal(both["pd"][1][:, :, 1], solo["pd"][1][:, :, 0])


# ------------------------------------------------------------------ 3. the library
@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_point(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    if not os.path.exists(path):
        pytest.skip(f"{so} has not been built")
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    assert " pgb_predict_pdp\n" in syms and " pgb_pdp_kernel_ms\n" in syms and "pgb_predict_pdp" not in _abi.SYMBOLS


def test_the_library_validates_before_it_touches_a_device():
    """Every check of ``pgb_predict_pdp`` precedes its first HIP call, so the library answers them without a GPU."""
    if not os.path.exists(_abi.hip_library_path()):
        pytest.skip("libpgbart_hip.so has not been built")
    lib = _abi.load_hip_library()
    call = lib.pdp_entry_point()
    pool = host.hand_pool()
    fidx = np.array([[0, 1, 2], [3, 4, 5], [6, 0, 2], [4, 5, 5]], np.int32)
    carr = pool.as_c()
    buf = np.zeros(64)                                            # stands in for device memory: never dereferenced
    cols = np.array([1], np.int32)
    picks = np.zeros((1, 3), np.int32)
    taken = np.zeros(1, np.int32)

    def run(**kw):
        a = dict(trees=C.byref(carr), fidx=fidx.ctypes.data, n_forests=4, m=3, X=buf.ctypes.data, n_rows=8, p=3, ldx=3,
                 cols=cols.ctypes.data, n_cols=1, picks=picks.ctypes.data, n_picks=3, route=0, out=buf.ctypes.data)
        a.update(kw)
        rc = call(a["trees"], a["fidx"], a["n_forests"], a["m"], a["X"], a["n_rows"], a["p"], a["ldx"], a["cols"],
                  a["n_cols"], a["picks"], a["n_picks"], a["route"], a["out"], taken.ctypes.data, None)
        return rc, lib.lib.pgb_last_error().decode()

    for name, arg in (("trees", "trees"), ("fidx", "forest_tree_idx"), ("X", "X_dev"), ("cols", "cols_host"),
                      ("picks", "picks_host"), ("out", "out_dev")):
        rc, msg = run(**{name: None})
        assert rc == E_INVALID and f"pgb_predict_pdp: {arg} is null" in msg, (name, msg)
    for name in ("n_cols", "n_picks", "n_rows", "n_forests", "m", "p"):
        for bad in (0, -1):
            rc, msg = run(**{name: bad})
            assert rc == E_INVALID and name in msg, (name, msg)
    rc, msg = run(ldx=2)
    assert rc == E_INVALID and "ldx must be >= p" in msg, msg
    for bad in (3, -1):
        rc, msg = run(route=bad)
        assert rc == E_INVALID and "route must be 0 (auto), 1 (direct) or 2 (profile)" in msg, msg
    for bad in (3, -1):
        cols[0] = bad
        rc, msg = run()
        assert rc == E_INVALID and "cols_host[0]" in msg and "outside [0, p = 3)" in msg, msg
    cols[0] = 1
    for bad in (4, -1):
        picks[0, 2] = bad
        rc, msg = run()
        assert rc == E_INVALID and "picks_host[2]" in msg and "outside [0, n_forests = 4)" in msg, msg
    picks[0, 2] = 0
    broken = fidx.copy()
    broken[2, 1] = 7                                              # the history, through pred_validate
    rc, msg = run(fidx=broken.ctypes.data)
    assert rc == E_INVALID and "forest_tree_idx entry outside" in msg, msg
    pool.var[0] = 5                                               # a split on a column X does not have
    rc, msg = run()
    assert rc == E_INVALID and "column X does not have" in msg, msg


def test_the_binding_mirrors_the_header():
    text = open(os.path.join(ROOT, "include", "pgbart_pdp.h")).read()
    assert int(re.search(r"#define PGB_PDP_LDS_MAXB (\d+)", text).group(1)) == _abi.PDP_LDS_MAXB
    budget = __import__("json").load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    for name in ("k_pdp_lookup<false>", "k_pdp_lookup<true>"):         # bound by its output stream: no scratch
        assert budget[name]["max_scratch_bytes"] == 0 and budget[name]["max_vgpr_spills"] == 0
    assert sum(k.startswith("k_pdp_walk<") for k in budget) == 4


# ------------------------------------------------------------------ 4. the slot argument
def _slots_hold(sampler, p, cols, draws):
    """Per (column, draw): the oracle's prediction at every probe of a slot is its prediction at the slot's
    representative, bit for bit; returns the number of slots seen."""
    seen = 0
    for j in cols:
        others = [v for v in range(p) if v != j]
        for d in draws:
            ok, b = host.breakpoints(sampler.pool, sampler.forest_idx[d], j)
            assert ok
            rep = host.representatives(b)
            for k, xs in enumerate(host.probes(b)):
                if not xs:
                    continue
                assert list(host.lookup(b, np.asarray(xs))) == [k] * len(xs), (j, d, k, xs)
                rows = np.full((len(xs) + 1, p), -7.5)
                rows[0, j] = rep[k]
                rows[1:, j] = xs
                pred = np.asarray(sampler.sample_posterior(rows, [int(d)], others))[0]      # (K, 1 + probes)
                assert np.array_equal(pred[:, 1:], np.repeat(pred[:, :1], len(xs), axis=1), equal_nan=True), (j, d, k)
                seen += 1
    return seen


def test_the_slot_argument_on_a_short_fit(fit):
    op, X, s = fit
    one = s._chain_samplers[0]
    assert _slots_hold(one, 3, [0, 1, 2], [0, 5, 11]) > 9
    rng = np.random.default_rng(3)
    Xp = X.copy()
    Xp[rng.random(90) < 0.1, 0] = np.nan
    Xp[:4, 2] = [np.inf, -np.inf, 0.0, -0.0]
    ok, b = host.breakpoints(one.pool, one.forest_idx[7], 0)
    Xp[4:4 + min(b.size, 5), 0] = b[:5]                                # values equal to a breakpoint
    picks = rng.integers(0, 12, size=(3, 4))
    picks[1, 3] = picks[1, 0]
    assert np.array_equal(host.profile_sweep(one, Xp, [0, 1, 2], picks), host.yardstick(one, Xp, [0, 1, 2], picks))


def test_the_slot_argument_on_hand_built_pools_and_in_exact_arithmetic(oracle):
    pool = host.hand_pool()
    table = np.array([[0, 1, 2, 3], [3, 4, 5, 5], [6, 0, 2, 1], [4, 5, 5, 4]], np.int32)
    s = PosteriorSampler(pool, table, 4, 2, backend=oracle)
    ok, b = host.breakpoints(pool, table[0], 0)
    assert ok and list(b) == [-1.25, 0.0, 0.5, math.inf]              # 0.0 and -0.0 are one breakpoint, 0.5 too
    assert list(host.breakpoints(pool, table[1], 0)[1]) == [0.0]      # B = 1
    assert host.breakpoints(pool, table[3], 0)[1].size == 0           # B = 0: no split on the column
    assert host.breakpoints(pool, table[0], 1) == (False, None)       # a leaf regresses on column 1 ...
    assert host.breakpoints(pool, table[3], 2) == (False, None)       # ... and one on column 2
    assert _slots_hold(s, 3, [0], [0, 1, 2, 3]) >= 6 + 3 + 2
    # the same in Fractions: the exact sum at every probe of a slot is the exact sum at its representative, and the
    # oracle returns that sum (no operation can round: exact_class)
    for d in range(4):
        b = host.breakpoints(pool, table[d], 0)[1]
        rep = host.representatives(b)
        for k, xs in enumerate(host.probes(b)):
            if not xs:
                continue
            rows = np.full((len(xs) + 1, 3), 0.375)
            rows[0, 0] = rep[k]
            rows[1:, 0] = xs
            exact = ex.walk(pool, table[d:d + 1], rows, excluded=[1, 2])
            want = exact.exact_class()                                 # (1, 2, 1 + probes)
            assert all(exact.R[0, o, i] == exact.R[0, o, 0] for o in range(2) for i in range(1, len(xs) + 1)), (d, k)
            got = np.asarray(s.sample_posterior(rows, [d], [1, 2]))
            assert np.array_equal(got, want), (d, k)
    # ... and the sweep put together from the profiles is the sweep
    X = np.array([[-2.0, 0.0, 1.0], [-1.25, 0.0, 1.0], [-0.0, 0.5, 1.0], [0.0, 0.5, 1.0], [5e-324, 1.0, 1.0], [0.5, 1.0, 2.0],
                  [0.75, 1.0, 2.0], [math.inf, 1.0, 2.0], [-math.inf, 1.0, 2.0], [math.nan, 1.0, 2.0]])
    picks = np.array([[0, 1, 2, 3, 0], [3, 3, 1, 0, 2]])
    assert np.array_equal(host.profile_sweep(s, X, [0, 0], picks), host.yardstick(s, X, [0, 0], picks))
    assert np.array_equal(s.pdp_sweep(X, [0, 2], picks), host.yardstick(s, X, [0, 2], picks))
