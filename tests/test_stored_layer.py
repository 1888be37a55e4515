"""The Python layer of the stored-draw entry points, without a GPU: what every public function asks of the library.

Each scenario drives one public function with a sampler whose backend is ``_recording_backend.Recorder`` and compares
the trace -- every allocation, every library call with its scalars and the sizes of its buffers, every copy back, in
order -- with ``golden/stored_layer_traces.json``.  Every function runs with its block knob unset and with the knob
at its floor, where the rows (or columns) fall into at least three blocks with a ragged last one; some also with fewer
than 64 rows and with trees of two outputs.  The kernels are absent: buffers stay zero, results mean nothing.

The fixture is recorded by ``python tests/test_stored_layer.py --record`` and pins the layer as it was before it was
restated in ``pymc_bart_amd/_stored.py``: it is regenerated only when a change of behaviour is the point of a change.
The last tests pin ``_stored`` itself: the one block rule, the floors of the four knobs and the order of the checks.
"""

from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import pymc_bart_amd as pb  # noqa: E402
from _recording_backend import Recorder  # noqa: E402
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays  # noqa: E402
from pymc_bart_amd.utils import _MultiChainSampler  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "stored_layer_traces.json")
KNOBS = {"PW": ("PGB_PW_BLOCK_BYTES", 1 << 16), "SHAP": ("PGB_SHAP_BLOCK_BYTES", 1 << 12),
         "PDP": ("PGB_PDP_BLOCK_BYTES", 1 << 12), "ICE": ("PGB_ICE_BLOCK_BYTES", 1 << 16)}
N, P, M_TREES, PER_CHAIN = 450, 20, 3, 30   # rows, columns, trees, draws of a chain (two chains: 60 draws)
D = 2 * PER_CHAIN


def _stumps(K: int, n_trees: int = M_TREES) -> TreeArrays:
    pool = TreeArrays.empty(n_trees, n_trees, K)
    pool.tree_id[:] = np.arange(n_trees)
    pool.node_off[:] = np.arange(n_trees + 1)
    pool.var[:] = -1
    pool.count[:] = 10
    return pool


def _chain(rec, K: int):
    return PosteriorSampler(_stumps(K), np.tile(np.arange(M_TREES, dtype=np.int32), (PER_CHAIN, 1)), M_TREES, K, backend=rec)


def _fit(rec, K: int = 1, chains: int = 2):
    """Two chains behind one draw index (the cached ``pooled_history``), or one chain on its own (none)."""
    return _MultiChainSampler([_chain(rec, K) for _ in range(chains)]) if chains > 1 else _chain(rec, K)


class _Op:
    """What ``partial_dependence`` reads of a BART op: one chain of ``PER_CHAIN`` draws."""

    def __init__(self, K: int):
        batch = _stumps(K, 1)
        self.all_trees = [(_stumps(K), [batch] * PER_CHAIN)]
        self.m, self.n_outputs = M_TREES, K


def _data(n: int = N, p: int = P):
    rng = np.random.default_rng(7)
    return rng.normal(size=(n, p)), rng.normal(size=n)


def _matrix(n: int = 300):
    return np.random.default_rng(3).normal(size=(D, n))


def _scenarios() -> dict:
    """name -> (knob or None, call(rec)).  Every name runs with the knob unset and, given one, with it at its floor."""
    X, y = _data()
    Xs, ys = _data(37)
    norm, ms = pb.NormalLikelihood(1.0), pb.NormalMeanScaleLikelihood()
    off2 = np.zeros((2, N))
    cols5 = [0, 3, 7, 11, 19]
    picks_pdp = np.arange(5 * 4).reshape(5, 4) % PER_CHAIN
    picks_ice = np.arange(19 * 2 * 3).reshape(19, 2, 3) % PER_CHAIN  # (19 columns: ragged for 9 and for 4 a block)
    s = {
        "pointwise_log_likelihood": ("PW", lambda r: pb.pointwise_log_likelihood(_fit(r), X, y, norm, offset=np.zeros(N))),
        "pointwise_log_likelihood_small": ("PW", lambda r: pb.pointwise_log_likelihood(_fit(r, chains=1), Xs, ys, norm)),
        "pointwise_log_likelihood_K2": ("PW", lambda r: pb.pointwise_log_likelihood(_fit(r, 2), X, y, ms, draws=range(5, 45))),
        "log_predictive_density": ("PW", lambda r: pb.log_predictive_density(_fit(r), X, y, norm)),
        "loo": ("PW", lambda r: pb.loo(_fit(r), X, y, norm, reff=0.8)),
        "loo_pit": ("PW", lambda r: pb.loo_pit(_fit(r), X, y, norm, offset=np.zeros(N), random_seed=11)),
        "loo_predictive_mu": ("PW", lambda r: pb.loo_predictive(_fit(r), X, y, norm, kind="mu")),
        "loo_predictive_mu_K2": ("PW", lambda r: pb.loo_predictive(_fit(r, 2), X, y, ms, offset=off2, kind="mu")),
        "loo_predictive_y": ("PW", lambda r: pb.loo_predictive(_fit(r), X, y, norm, kind="y", random_seed=5)),
        "loo_predictive_y_K2": ("PW", lambda r: pb.loo_predictive(_fit(r, 2), X, y, ms, kind="y", random_seed=5)),
        "psis_loo_matrix": ("PW", lambda r: pb.psis_loo_matrix(_matrix(), backend=r)),
        "psis_expectation_matrix_value": ("PW", lambda r: pb.psis_expectation_matrix(_matrix(), _matrix(), backend=r)),
        "psis_expectation_matrix_pit": ("PW", lambda r: pb.psis_expectation_matrix(_matrix(), _matrix(), y=np.zeros(300),
                                                                                 kind="pit", backend=r)),
        "posterior_summary": ("PW", lambda r: pb.posterior_summary(_fit(r), X, offset=np.zeros(N), excluded=[2, 4])),
        "posterior_summary_small": ("PW", lambda r: pb.posterior_summary(_fit(r, chains=1), Xs, quantiles=None, hdi_prob=None)),
        "posterior_summary_K2": ("PW", lambda r: pb.posterior_summary(_fit(r, 2), X, draws=range(40), transform="exp")),
        "summarize_matrix": ("PW", lambda r: pb.summarize_matrix(_matrix(), backend=r)),
        "summarize_matrix_small": ("PW", lambda r: pb.summarize_matrix(_matrix(37), hdi_prob=None, backend=r)),
        "posterior_predictive": ("PW", lambda r: pb.posterior_predictive(_fit(r), X, norm, offset=np.zeros(N), random_seed=3)),
        "posterior_predictive_K2": ("PW", lambda r: pb.posterior_predictive(_fit(r, 2), X, ms, excluded=[1], random_seed=3)),
        "predictive_summary": ("PW", lambda r: pb.predictive_summary(_fit(r), X, norm, random_seed=3)),
        "predictive_summary_K2": ("PW", lambda r: pb.predictive_summary(_fit(r, 2), X, ms, random_seed=3)),
        "predictive_pit": ("PW", lambda r: pb.predictive_pit(_fit(r), X, y, norm, random_seed=3)),
        "predictive_pit_K2": ("PW", lambda r: pb.predictive_pit(_fit(r, 2), X, y, ms, random_seed=3)),
        "convergence": ("PW", lambda r: pb.convergence(_fit(r), X, offset=np.zeros(N))),
        "convergence_K2": ("PW", lambda r: pb.convergence(_fit(r, 2), X, draws_per_chain=20, excluded=[0])),
        "relative_efficiency": ("PW", lambda r: pb.relative_efficiency(_fit(r), X, y, norm)),
        "diagnose_matrix": ("PW", lambda r: pb.diagnose_matrix(_matrix(), 2, backend=r)),
        "shap_values": ("SHAP", lambda r: pb.shap_values(_fit(r), X, draws=range(6))),
        "shap_values_small": ("SHAP", lambda r: pb.shap_values(_fit(r, chains=1), Xs, samples=4, random_seed=1)),
        "shap_values_K2": ("SHAP", lambda r: pb.shap_values(_fit(r, 2), X, draws=[3, 3, 8])),
        "shap_summary": ("SHAP", lambda r: pb.shap_summary(_fit(r), X, draws=range(6))),
        "shap_interaction_values": ("SHAP", lambda r: pb.shap_interaction_values(_fit(r), X, cols=[7, 0, 3], draws=range(6))),
        "shap_interaction_values_all_cols": ("SHAP", lambda r: pb.shap_interaction_values(_fit(r, chains=1), Xs[:, :4], draws=[1, 2])),
        "shap_interaction_summary": ("SHAP", lambda r: pb.shap_interaction_summary(_fit(r, 2), X, cols=[7, 0, 3], draws=range(6))),
        "pdp_sweep": ("PDP", lambda r: _fit(r).pdp_sweep(X, cols5, picks_pdp)),
        "pdp_sweep_K2": ("PDP", lambda r: _fit(r, 2, chains=1).pdp_sweep(X, cols5, picks_pdp, route=1, taken=[])),
        "partial_dependence_summary": ("PDP", lambda r: pb.partial_dependence(
            _Op(1), X, var_idx=[0, 5, 9], xs_interval="insample", samples=8, random_seed=2, backend=r, summary={})),
        "partial_dependence_summary_K2_no_pd": ("PDP", lambda r: pb.partial_dependence(
            _Op(2), X, var_idx=[4], xs_interval="insample", samples=8, random_seed=2, backend=r,
            summary={"quantiles": [0.5], "hdi_prob": None, "transform": "logistic"}, keep_pd=False)),
        "ice_mean": ("ICE", lambda r: _fit(r).ice_mean(X, X[[5, 17]], list(range(19)), picks_ice)),
        "ice_mean_K2": ("ICE", lambda r: _fit(r, 2, chains=1).ice_mean(X, X[[5, 17]], list(range(19)), picks_ice)),
    }
    return s


#: name of the run -> (scenario, {env name: bytes}).  ``pdp_sweep`` at its floor takes rows of one column; the third
#: setting holds two whole columns (each is 8 * 4 picks * 450 rows bytes).
def _runs() -> dict:
    runs = {}
    for name, (knob, _) in _scenarios().items():
        runs[name + "/unset"] = (name, {})
        runs[name + "/floor"] = (name, {KNOBS[knob][0]: KNOBS[knob][1]})
    runs["pdp_sweep/two_columns"] = ("pdp_sweep", {"PGB_PDP_BLOCK_BYTES": 2 * 8 * 4 * N + 100})
    runs["pdp_sweep/below_floor"] = ("pdp_sweep", {"PGB_PDP_BLOCK_BYTES": 1})
    runs["posterior_summary/below_floor"] = ("posterior_summary", {"PGB_PW_BLOCK_BYTES": 1})
    return runs


RUNS = _runs()
SCENARIOS = _scenarios()


def _trace(run: str, setenv) -> list:
    name, env = RUNS[run]
    for _, (var, _) in KNOBS.items():
        setenv(var, None)
    for var, value in env.items():
        setenv(var, str(value))
    rec = Recorder()
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")  # (zeros everywhere: k = 0, ESS = 0, ...)
        SCENARIOS[name][1](rec)
    return rec.trace


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("run", sorted(RUNS))
def test_the_trace_of_every_entry_is_the_recorded_one(run, golden, monkeypatch):
    def setenv(var, value):
        monkeypatch.delenv(var, raising=False) if value is None else monkeypatch.setenv(var, value)

    got = _trace(run, setenv)
    want = golden[run]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{run}: line {i} of the trace differs"
    assert len(got) == len(want), run


@pytest.mark.parametrize("run", sorted(r for r in RUNS if r.endswith("/floor") and "small" not in r and "all_cols" not in r))
def test_at_its_floor_a_knob_gives_at_least_three_blocks_and_a_ragged_last_one(run, golden):
    """(Of the fixture alone: the floor cases are the ones that can tell two block rules apart.)"""
    trace = golden[run]
    first = next(line for line in trace if line.startswith("pgb_"))
    calls = [line for line in trace if line.split()[0] == first.split()[0]]
    assert len(calls) >= 3 and len(set(calls)) >= 2, (run, len(calls))
    assert calls[0] != calls[-1], run  # (the last block is smaller: another row count or buffer size)


# ---------------------------------------------------------------------------------------------- _stored itself
def test_row_blocks_is_the_old_expression():
    from pymc_bart_amd import _stored

    for n in (1, 2, 63, 64, 65, 127, 128, 129, 450, 640, 1000):
        for per_row in (8, 24, 152, 1000, 4096, 70000):
            for limit in (1, 100, 4095, 4096, 1 << 16, (1 << 16) + 1, 1 << 20, 1 << 30):
                block = max(64, min(n, limit // per_row // 64 * 64))
                want = [(r0, min(n, r0 + block)) for r0 in range(0, n, block)]
                assert _stored.row_blocks(n, per_row, limit) == want, (n, per_row, limit)
                rows = max(64, limit // per_row // 64 * 64)  # (shap.blocks and pdp.blocks had no min(n, .))
                assert want == [(r0, min(n, r0 + rows)) for r0 in range(0, n, rows)], (n, per_row, limit)


def test_col_blocks_is_the_old_expression():
    from pymc_bart_amd import _stored

    for n_cols in (1, 2, 5, 20):
        for per_col in (8, 7200, 1 << 16, 1 << 20):
            for limit in (1, 1 << 12, 1 << 16, 20000, 1 << 30):
                step = max(1, min(n_cols, limit // per_col))
                want = [(c0, min(n_cols, c0 + step)) for c0 in range(0, n_cols, step)]
                assert _stored.col_blocks(n_cols, per_col, limit) == want, (n_cols, per_col, limit)


@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_block_bytes_reads_its_knob_with_its_default_and_its_floor(knob, monkeypatch):
    from pymc_bart_amd import _stored

    var, floor = KNOBS[knob]
    monkeypatch.delenv(var, raising=False)
    assert _stored.block_bytes(var, floor) == 1 << 30
    for value, want in ((1, floor), (floor - 1, floor), (floor, floor), (floor + 1, floor + 1), (1 << 33, 1 << 33)):
        monkeypatch.setenv(var, str(value))
        assert _stored.block_bytes(var, floor) == want


def test_the_first_fault_reported_is_the_one_reported_before():
    """One doubly-bad input per job: the family is looked at before ``X`` by the scoring and the replicating job; the
    summarising job reaches its summary spec only after ``draws``; the seed comes last."""
    class NoBackend:
        pass

    s = PosteriorSampler(_stumps(1), np.tile(np.arange(M_TREES, dtype=np.int32), (5, 1)), M_TREES, 1, backend=NoBackend())
    X, y = np.zeros((8, 2)), np.zeros(8)
    cube = np.zeros((2, 2, 2))
    norm = pb.NormalLikelihood(1.0)
    callback = pb.CallbackLikelihood(lambda yy, mu: -(yy - mu) ** 2)
    with pytest.raises(ValueError, match="callback"):
        pb.pointwise_log_likelihood(s, cube, y, callback)
    with pytest.raises(ValueError, match="X must be a matrix"):
        pb.pointwise_log_likelihood(s, cube, np.zeros(7), norm)
    with pytest.raises(ValueError, match="y must hold one value per row"):
        pb.pointwise_log_likelihood(s, X, np.zeros(7), norm, offset=np.zeros(3))
    with pytest.raises(ValueError, match="offset must have shape"):
        pb.pointwise_log_likelihood(s, X, y, norm, offset=np.zeros(3), draws=[9])
    with pytest.raises(ValueError, match="no draws to score"):
        pb.pointwise_log_likelihood(s, X, y, pb.NormalLikelihood("sigma"), points=[], draws=[])
    with pytest.raises(ValueError, match="has a log density only"):
        pb.posterior_predictive(s, cube, callback)
    with pytest.raises(ValueError, match="X must be a matrix"):
        pb.predictive_pit(s, cube, np.zeros(7), norm)
    with pytest.raises(ValueError, match="y must hold one value per row"):
        pb.predictive_pit(s, X, np.zeros(7), norm, offset=np.zeros(3))
    with pytest.raises(ValueError, match="offset must have shape"):
        pb.posterior_predictive(s, X, norm, offset=np.zeros(3), excluded=[2])
    with pytest.raises(ValueError, match="excluded must index"):
        pb.posterior_predictive(s, X, norm, excluded=[2], draws=[9])
    with pytest.raises(ValueError, match="draws must index"):
        pb.posterior_predictive(s, X, norm, draws=[9], random_seed=-1)
    with pytest.raises(ValueError, match="no draws to replicate"):
        pb.posterior_predictive(s, X, norm, draws=[], random_seed=-1)
    with pytest.raises(ValueError, match="outside the normal family's domain"):
        pb.posterior_predictive(s, X, pb.NormalLikelihood(-1.0), random_seed=-1)
    with pytest.raises(ValueError, match="random_seed"):
        pb.posterior_predictive(s, X, norm, random_seed=-1)
    with pytest.raises(ValueError, match="X must be a matrix"):
        pb.posterior_summary(s, cube, transform="cube")
    with pytest.raises(ValueError, match="offset must have shape"):
        pb.posterior_summary(s, X, offset=np.zeros(3), excluded=[2])
    with pytest.raises(ValueError, match="excluded must index"):
        pb.posterior_summary(s, X, excluded=[2], draws=[9])
    with pytest.raises(ValueError, match="draws must index"):
        pb.posterior_summary(s, X, draws=[9], transform="cube")
    with pytest.raises(ValueError, match="unknown transform"):
        pb.posterior_summary(s, X, draws=[], transform="cube")
    with pytest.raises(ValueError, match="at least 2 draws"):
        pb.posterior_summary(s, X, draws=[])
    with pytest.raises(TypeError):
        pb.posterior_summary(object(), cube)


@pytest.mark.parametrize("call, noun", [
    (lambda be: pb.summarize_matrix(np.zeros((4, 3)), backend=be), "posterior summaries run"),
    (lambda be: pb.psis_loo_matrix(np.zeros((10, 3)), backend=be), "PSIS-LOO runs"),
    (lambda be: pb.diagnose_matrix(np.zeros((8, 3)), 2, backend=be), "chain diagnostics run"),
])
def test_the_hip_only_message_keeps_its_noun(call, noun):
    from pymc_bart_amd._abi import PGBError

    rec = Recorder()
    rec.lib.backend_name = "cpu-oracle"
    with pytest.raises(PGBError, match=f"{noun} on the HIP backend only, not on cpu-oracle"):
        call(rec)
    assert rec.trace == []


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_stored_layer.py --record"

    def _setenv(var, value):
        os.environ.pop(var, None) if value is None else os.environ.__setitem__(var, value)

    traces = {run: _trace(run, _setenv) for run in sorted(RUNS)}
    with open(GOLDEN, "w") as f:
        json.dump(traces, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{len(traces)} traces, {sum(len(t) for t in traces.values())} lines -> {GOLDEN}")
