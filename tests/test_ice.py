"""ICE curves on the build box (no GPU): the public function and ``ice_mean`` on the oracle backend (whose library has
no ``pgb_predict_ice``: the probe-matrix loop) against the implementation the fused call replaced
(``tests/_ice_host.py``), the host-side validation, the library's own validation (it runs before anything touches a
device) and the kernel instances in the occupancy budget."""
import ctypes as C
import json
import os
import subprocess
import types

import numpy as np
import pytest

import _ice_host as host
from _oracle import NumpyMemory
from pymc_bart_amd import BARTOp, _abi, compiled, individual_conditional_expectation
from pymc_bart_amd.chains import sample_chain
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays
from pymc_bart_amd.utils import _get_posterior_sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pymc_bart_amd", "csrc")
E_INVALID = -1  # PGB_E_INVALID (include/pgbart.h)


@pytest.fixture(scope="module")
def fit(oracle):
    """The shape of test_oracle_behaviour's ICE case (a shorter chain), and a second BART variable for the list case."""
    rng = np.random.default_rng(8)
    X = rng.uniform(-1, 1, size=(300, 3))
    Y = 2.0 * X[:, 0] + (X[:, 2] > 0) + rng.normal(0, 0.1, 300)
    op = BARTOp(X, Y, m=20)
    sample_chain(op, tune=30, draws=25, random_seed=11, backend=oracle)
    op2 = BARTOp(X, -Y, m=10)
    sample_chain(op2, tune=10, draws=25, random_seed=12, backend=oracle)
    return X, op, op2


def _same(a, b):
    assert set(a) == set(b) and np.array_equal(a["instances"], b["instances"])
    assert set(a["ice"]) == set(b["ice"]) and a["labels"] == b["labels"]
    for j in a["ice"]:
        assert a["ice"][j].shape == b["ice"][j].shape
        assert np.array_equal(a["ice"][j], b["ice"][j]), j
        assert np.array_equal(a["x"][j], b["x"][j])


@pytest.mark.parametrize("kw", [dict(var_idx=[0, 1], instances=6, samples=15, random_seed=4),
                                dict(var_idx=[2], instances=3, samples=7, centered=False, random_seed=5),
                                dict(instances=2, samples=4, func=lambda a: 2 * a + 1, random_seed=6)])
def test_the_public_function_on_the_oracle_is_what_it_was(fit, oracle, kw):
    X, op, _ = fit
    _same(individual_conditional_expectation(op, X, backend=oracle, **kw),
          host.ice_by_probe_matrices(op, X, backend=oracle, **kw))


def test_a_list_of_bart_variables_contributes_its_outputs_side_by_side(fit, oracle):
    X, op, op2 = fit
    kw = dict(var_idx=[1, 0], instances=3, samples=5, random_seed=9, backend=oracle)
    got = individual_conditional_expectation([op, op2], X, **kw)
    _same(got, host.ice_by_probe_matrices([op, op2], X, **kw))
    assert got["ice"][0].shape == (3, 300, 2)
    alone = individual_conditional_expectation(op2, X, **kw)     # the same picks serve every variable of the list
    assert np.array_equal(got["ice"][0][:, :, 1:], alone["ice"][0])


def test_the_fallback_of_ice_mean_is_the_pick_order_loop(fit, oracle):
    X, op, _ = fit
    rng = np.random.default_rng(1)
    s = _get_posterior_sampler(op, backend=oracle)
    part = s._chain_samplers[0]
    cols = [2, 0]
    inst = X[[5, 17, 17]]
    picks = rng.integers(0, s.n_draws, size=(2, 3, 6))
    picks[0, 1] = picks[0, 1, 0]                                  # a repeated pick
    want = host.yardstick(part, X[:90], inst, cols, picks)
    for sampler in (part, s):
        got = sampler.ice_mean(X[:90], inst, cols, picks)
        assert got.shape == (2, 3, 1, 90) and np.array_equal(got, want)
    one = part.ice_mean(X[:90], inst, cols, picks[:, :, :1])      # one pick: the prediction itself
    assert np.array_equal(one[1, 0], part.sample_posterior(
        np.column_stack([X[:90, 0], np.tile(inst[0, 1:], (90, 1))]), [int(picks[1, 0, 0])])[0])


def _stumps(draws=5, m=3, K=1, backend=None):
    pool = TreeArrays.empty(m, m, K)
    pool.tree_id[:] = np.arange(m)
    pool.node_off[:] = np.arange(m + 1)
    pool.var[:] = -1
    pool.count[:] = 10
    if backend is None:  # every host-side check passes -> the first touch of the library raises AttributeError
        backend = types.SimpleNamespace(mem=NumpyMemory(), lib=None)
    return PosteriorSampler(pool, np.tile(np.arange(m, dtype=np.int32), (draws, 1)), m, K, backend=backend)


def test_argument_errors_are_raised_before_a_backend_is_touched():
    s = _stumps()
    X, inst = np.zeros((8, 2)), np.zeros((3, 2))
    picks = np.zeros((1, 3, 4), np.int64)
    with pytest.raises(ValueError, match="X must be a matrix"):
        s.ice_mean(np.zeros((2, 2, 2)), inst, [0], picks)
    with pytest.raises(ValueError, match="instances must have shape"):
        s.ice_mean(X, np.zeros((3, 3)), [0], picks)
    with pytest.raises(ValueError, match="cols must be a non-empty vector"):
        s.ice_mean(X, inst, [], picks[:0])
    with pytest.raises(ValueError, match="cols must index"):
        s.ice_mean(X, inst, [2], picks)
    with pytest.raises(ValueError, match="cols must index"):
        s.ice_mean(X, inst, [-1], picks)
    with pytest.raises(ValueError, match="picks must have shape"):
        s.ice_mean(X, inst, [0], picks[:, :2])
    with pytest.raises(ValueError, match="picks must have shape"):
        s.ice_mean(X, inst, [0, 1], picks)
    with pytest.raises(ValueError, match="picks must index the 5 stored draws"):
        s.ice_mean(X, inst, [0], picks + 5)
    with pytest.raises(ValueError, match="picks must index"):
        s.ice_mean(X, inst, [0], picks - 1)
    with pytest.raises(ValueError, match="no draws"):
        s.ice_mean(X, inst, [0], picks[:, :, :0])
    with pytest.raises(ValueError, match="no draws"):
        _stumps(draws=0).ice_mean(X, inst, [0], picks)
    with pytest.raises(AttributeError):                           # a call that passes every check reaches the backend
        s.ice_mean(X, inst, [0], picks)


def test_the_library_validates_before_it_touches_a_device():
    """Every check of ``pgb_predict_ice`` precedes its first HIP call, so the library answers them without a GPU."""
    if not os.path.exists(_abi.hip_library_path()):
        pytest.skip("libpgbart_hip.so has not been built")
    lib = _abi.load_hip_library()
    call = lib.ice_entry_point()
    s = _stumps(draws=4)
    carr = s.pool.as_c()
    fidx = s.forest_idx
    buf = np.zeros(64)                                            # stands in for device memory: never dereferenced
    cols = np.array([1], np.int32)
    picks = np.zeros((1, 2, 3), np.int32)

    def run(**kw):
        a = dict(trees=C.byref(carr), fidx=fidx.ctypes.data, n_forests=4, m=3, X=buf.ctypes.data, n_rows=8, p=2, ldx=2,
                 inst=buf.ctypes.data, n_inst=2, ldi=2, cols=cols.ctypes.data, n_cols=1, picks=picks.ctypes.data,
                 n_picks=3, out=buf.ctypes.data)
        a.update(kw)
        rc = call(a["trees"], a["fidx"], a["n_forests"], a["m"], a["X"], a["n_rows"], a["p"], a["ldx"], a["inst"],
                  a["n_inst"], a["ldi"], a["cols"], a["n_cols"], a["picks"], a["n_picks"], a["out"], None)
        return rc, lib.lib.pgb_last_error().decode()

    for name, arg in (("trees", "trees"), ("fidx", "forest_tree_idx"), ("X", "X_dev"), ("inst", "inst_dev"),
                      ("cols", "cols_host"), ("picks", "picks_host"), ("out", "out_dev")):
        rc, msg = run(**{name: None})
        assert rc == E_INVALID and f"{arg} is null" in msg, (name, msg)
    for name in ("n_inst", "n_cols", "n_picks", "n_rows"):
        for bad in (0, -1):
            rc, msg = run(**{name: bad})
            assert rc == E_INVALID and name in msg, (name, msg)
    for name in ("ldx", "ldi"):
        rc, msg = run(**{name: 1})
        assert rc == E_INVALID and name in msg, (name, msg)
    for bad in (2, -1):
        cols[0] = bad
        rc, msg = run()
        assert rc == E_INVALID and "cols_host[0]" in msg and "outside [0, p = 2)" in msg, msg
    cols[0] = 1
    for bad in (4, -1):
        picks[0, 1, 2] = bad
        rc, msg = run()
        assert rc == E_INVALID and "picks_host[5]" in msg and "outside [0, n_forests = 4)" in msg, msg
    picks[0, 1, 2] = 0
    broken = fidx.copy()
    broken[2, 1] = 7                                              # the history, through pred_validate
    rc, msg = run(fidx=broken.ctypes.data)
    assert rc == E_INVALID and "forest_tree_idx entry outside" in msg, msg
    s.pool.var[0], s.pool.left[0], s.pool.right[0] = 5, 0, 0      # a split on a column X does not have
    rc, msg = run()
    assert rc == E_INVALID and "column X does not have" in msg, msg


@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_point(so):
    path = os.path.join(CSRC, so)
    if not os.path.exists(path):
        pytest.skip(f"{so} has not been built")
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    assert " pgb_predict_ice\n" in syms and "pgb_predict_ice" not in _abi.SYMBOLS


def test_the_instances_are_in_the_occupancy_budget():
    """Every combination of (instance row in LDS, continuous rules only, one output) is built and budgeted as a
    one-wave workgroup; none spills beyond the walk's private stack, which is what k_predict carries."""
    budget = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    stack = budget["k_predict<true, true>"]["max_scratch_bytes"]
    for ldsi in ("true", "false"):
        for cont in ("true", "false"):
            for k1 in ("true", "false"):
                row = budget[f"k_ice<{ldsi}, {cont}, {k1}>"]
                assert row["max_vgpr_spills"] == 0 and row["max_scratch_bytes"] == stack, row
                assert row["min_wgs_per_cu"] >= 12, row           # (a one-wave workgroup: 12 = 3 waves per SIMD)
