"""Saturating steps -- CPU half: the oracle's count of fixed-point saturation events, and the host layer's error.

Every term of the sampler's sums is quantised by `pgb_quant` (include/pgbart_spec.h); a term beyond the declared range
2^range_exp is clamped to +-2^50 and counted in `counters.saturations`, and `PySampler._check_saturation` turns a
moved counter into an error.  The saturating cases of tests/_cases.py (SAT_CASES) make the counter move.  The GPU half
(tests/test_saturation_gpu.py) holds the HIP library to the oracle's counts and chains there; here

* every case reaches what it is for on the oracle (`check_sat_reach`) and reproduces its committed fingerprint
  (tests/golden/sat_runs.json, written by tests/golden/make_sat_golden.py);
* the oracle's counts are checked against NumPy written from the contract alone: the first tree update of every Normal
  case in closed form, every update of sat/normal_one_tree from the returned sum_trees and the exported trees, and
  -- inside check_sat_reach -- the sum_trees terms of every update of the per-row families;
* the error is raised once per saturating step with that step's own count, not on the clean steps after it, and by
  `sync()` with the total of an asynchronous span;
* a chain image carries its counter: a restored or unpickled chain does not report old events again.
"""
import functools
import json
import os
import pickle

import numpy as np
import pytest

from _cases import (SAT_CASES, check_sat_reach, make_sat, run_sat_case, sat_digest, sat_events, sat_recount_first,
                    sat_recount_run, sat_scales, sat_settings, step_keeping_outputs)
from _oracle import oracle_backend
from pymc_bart_amd import _abi
from pymc_bart_amd.image import ChainImage
from pymc_bart_amd.pgbart import PGBART, BARTOp, NormalLikelihood
from pymc_bart_amd.sampler import PySampler

SAT_GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "sat_runs.json")))
SAT_IDS = [name.split("/")[1] for name in SAT_CASES]
NORMAL = [name for name in SAT_CASES if make_sat(name).get("family", "normal") == "normal"]


@functools.lru_cache(maxsize=None)
def oracle_sat_run(name):
    """The oracle's run of a saturating case, computed once and shared (nobody changes it)."""
    c = make_sat(name)
    return c, run_sat_case(c, oracle_backend())


@pytest.mark.parametrize("name", SAT_CASES, ids=SAT_IDS)
def test_sat_case_reaches_its_counting_sites_and_reproduces_its_fingerprint(name):
    c, res = oracle_sat_run(name)
    check_sat_reach(c, res)
    assert sat_digest(res) == SAT_GOLD[name]
    assert res["counters"]["saturations"] == res["sat"][-1] > 0


# ------------------------------------------------------------------ recounts from the contract
@pytest.mark.parametrize("name", NORMAL, ids=[n.split("/")[1] for n in NORMAL])
def test_first_update_equals_the_closed_form_recount(name):
    """The first update of a Normal chain: sum_trees is init_sum and the tree being replaced predicts init_leaf in
    every row, so noi, r and e follow from y alone."""
    c, res = oracle_sat_run(name)
    cnt = sat_recount_first(c, res["settings"])[0]
    assert cnt == sat_events(res)[0]
    assert cnt > 0 or 0 not in (range(c["steps"]) if c["sat_steps"] == "all" else c["sat_steps"])


def test_edge_exact_counts_the_neighbours_beyond_the_range_and_nothing_else():
    """With one tree and init_leaf = 0: noi = 0, r = y, e = y - init_leaf = y.  A term is counted when it is strictly
    beyond 2^50: x c1 for |x| > 2^range_exp, x^2 c2 likewise (frac = 50 at n = 130)."""
    c, res = oracle_sat_run("sat/edge_exact")
    st = res["settings"]
    n = c["X"].shape[0]
    frac, c1, c2 = sat_scales(n, st.range_exp)
    assert frac == 50 and st.init_leaf == 0.0 and st.init_sum == 0.0 and c["m"] == 1
    y = c["Y"]
    top = 2.0 ** st.range_exp
    assert [y[i] for i in (0, 1)] == [top, -top] and y[2] > top > y[64] and y[3] < -top < y[129]
    per_row = np.zeros(n, np.int64)
    for x, scale in ((np.full(n, st.init_sum), c1), (y, c1), (y * y, c2), ((y - st.init_leaf) ** 2, c2)):
        per_row += (np.abs(x * scale) > 2.0 ** 50)
    want = np.zeros(n, np.int64)
    want[[2, 3]] = 3            # r, r^2 and e^2 of the two neighbours beyond; +-2^range_exp and the neighbours inside: none
    assert np.array_equal(per_row, want)
    assert res["sat"][0] == 6 == sat_recount_first(c, st)[0]
    assert res["raised"][0] and res["raised_count"][0] == 6


def test_every_update_of_one_tree_equals_the_numpy_recount():
    """sat/normal_one_tree, no tuning: the events of every step recounted from the previous step's returned sum_trees,
    the previous export of the tree being replaced (rows routed in NumPy) and y.  Exact: the returned sum_trees is the
    sampler's own buffer bit for bit (the chain image holds the same bits)."""
    c, res = oracle_sat_run("sat/normal_one_tree")
    got = sat_events(res)
    assert np.array_equal(sat_recount_run(c, res), got)
    assert len(set(got.tolist())) >= 3     # (the count moves with the forest: a fixed number per row would not follow it)
    image = ChainImage.parse(res["sampler"].checkpoint())
    assert image.sum_trees.tobytes() == np.asarray(res["sum_trees"][-1]).tobytes()
    assert int(image.header.ctr.saturations) == res["sat"][-1]


def test_all_rows_top_sums_sit_at_n_times_the_limit():
    """n saturated terms still fit an int64 (include/pgbart_spec.h): B, C and E0 of the first update are n 2^50
    exactly, and the chain goes on from them."""
    c, res = oracle_sat_run("sat/normal_all_rows_top")
    n = c["X"].shape[0]
    cnt, A, B, Cq, E0 = sat_recount_first(c, res["settings"])
    assert (B, Cq, E0) == (n << 50,) * 3 and abs(A) < n << 50 and n << 50 < 2 ** 62
    assert cnt == 3 * n == res["sat"][0]
    assert np.all(np.isfinite(res["sum_trees"])) and sat_events(res)[2:].sum() == 0


# ------------------------------------------------------------------ the host contract of the error
def _sampler(c, backend):
    p = c["X"].shape[1]
    return PySampler(sat_settings(c), c["X"], c["Y"], np.zeros(p, np.int32), np.ones(p), backend=backend)


def test_error_is_raised_once_per_saturating_step_with_its_own_count(oracle):
    """PySampler.step itself on sat/normal_outliers: step 3 raises with the events of that step and names itself; the
    clean steps after it run."""
    c, res = oracle_sat_run("sat/normal_outliers")
    ev = sat_events(res)
    s = _sampler(c, oracle)
    sig_rng = np.random.default_rng(99)
    for it in range(c["steps"]):
        if it in c["responses"]:
            s.set_response(c["responses"][it])
        s.set_likelihood([float(0.5 + sig_rng.random())])
        if it == 3:
            with pytest.raises(_abi.PGBError, match=rf"^{ev[3]} fixed-point saturation events by astep 4:"):
                s.step(it < c["steps"] // 2)
        else:
            stv, _ = s.step(it < c["steps"] // 2)
            assert np.array_equal(stv, res["sum_trees"][it])
        assert s.counters.saturations == res["sat"][it]


def test_every_saturating_step_raises_with_its_own_count(oracle):
    c, res = oracle_sat_run("sat/normal_one_tree")
    ev = sat_events(res)
    s = _sampler(c, oracle)
    sig_rng = np.random.default_rng(99)
    for it in range(c["steps"]):
        s.set_likelihood([float(0.5 + sig_rng.random())])
        with pytest.raises(_abi.PGBError, match=rf"^{ev[it]} fixed-point saturation events by astep {it + 1}:"):
            s.step(False)


def test_sync_raises_with_the_total_of_an_asynchronous_span(oracle):
    """Three clean steps, then a span of two under the outlying response (both saturate), then clean steps."""
    c, _ = oracle_sat_run("sat/normal_outliers")
    a, b = _sampler(c, oracle), _sampler(c, oracle)
    for s in (a, b):
        s.set_likelihood([0.8])
        for _ in range(3):
            s.step(True)
        s.set_response(c["responses"][3])
    errs = [step_keeping_outputs(a, True)[2] for _ in range(2)]
    assert all(e is not None for e in errs)
    total = int(a.counters.saturations)
    assert total > 0
    b.step_async(True, 2)
    with pytest.raises(_abi.PGBError, match=rf"^{total} fixed-point saturation events by astep 5:"):
        b.sync()
    for s in (a, b):
        s.set_response(c["Y"])
    for _ in range(2):   # judged on their own: no error, and the same chain
        assert np.array_equal(a.step(False)[0], b.step(False)[0])
    assert a.counters.saturations == b.counters.saturations == total


# ------------------------------------------------------------------ the counter travels with the chain image
def test_restored_chain_does_not_report_old_events_again(oracle):
    """After a saturating step and a clean one: checkpoint, restore into a fresh PySampler, a clean step must not
    raise (the counter in the image did not move); a step that does saturate raises with its own count."""
    c, res = oracle_sat_run("sat/normal_outliers")
    ev = sat_events(res)
    s = _sampler(c, oracle)
    sig_rng = np.random.default_rng(99)
    sig = [float(0.5 + sig_rng.random()) for _ in range(c["steps"])]
    for it in range(5):                       # step 3 saturates, step 4 is clean
        if it in c["responses"]:
            s.set_response(c["responses"][it])
        s.set_likelihood([sig[it]])
        err = step_keeping_outputs(s, it < 4)[2]
        assert (err is not None) == (it == 3)
    blob = s.checkpoint()
    assert int(ChainImage.parse(blob).header.ctr.saturations) == ev[3] > 0
    t = _sampler(c, oracle)
    t.restore(blob)
    for it in (5, 6):
        t.set_likelihood([sig[it]])
        stv, _ = t.step(False)                # (raised "18 ... by astep 1" before the counter was taken from the image)
        assert np.array_equal(stv, res["sum_trees"][it])
        assert t.counters.saturations == ev[3]
    # the outlying response again: the uninterrupted chain tells what that step counts
    for it in (5, 6):
        s.set_likelihood([sig[it]])
        s.step(False)
    for q in (s, t):
        q.set_response(c["responses"][3])
        q.set_likelihood([sig[7]])
    own = step_keeping_outputs(s, False)[2]
    count = int(s.counters.saturations) - int(ev[3])
    assert own is not None and str(own).startswith(f"{count} fixed-point saturation events")
    with pytest.raises(_abi.PGBError, match=rf"^{count} fixed-point saturation events by astep 3:"):
        t.step(False)
    assert t.counters.saturations == s.counters.saturations


def test_saturating_case_resumes_from_checkpoints_with_the_same_flags(oracle):
    """run_sat_case through restores right before, right after and two steps after the saturating step: the same
    fingerprint, raised flags included."""
    c, _ = oracle_sat_run("sat/normal_outliers")
    assert sat_digest(run_sat_case(c, oracle, checkpoint_at=(3, 4, 6))) == SAT_GOLD[c["name"]]
    c, _ = oracle_sat_run("sat/probit_small_range")
    assert sat_digest(run_sat_case(c, oracle, checkpoint_at=(1, 5, 9))) == SAT_GOLD[c["name"]]


def test_unpickled_step_method_does_not_report_old_events_again(oracle, monkeypatch):
    """PGBART.__setstate__ restores the image into a fresh sampler on every unpickle."""
    from pymc_bart_amd import sampler as sampler_mod

    monkeypatch.setattr(sampler_mod, "_DEFAULT_BACKEND", oracle)  # what default_backend() returns
    rng = np.random.default_rng(5)
    X = rng.normal(size=(300, 3))
    Y = X[:, 0] - X[:, 1] + rng.normal(0, 0.2, 300)
    far, none = np.full(300, 1.0e4), np.zeros(300)

    def run(pickle_at):
        step = PGBART([BARTOp(X, Y, m=10)], num_particles=5, likelihood=NormalLikelihood(1.0), random_seed=3,
                      backend=oracle)
        out = []
        for it, off in enumerate([none, far, none, none, far, none]):
            if it in pickle_at:
                step = pickle.loads(pickle.dumps(step))
            try:
                out.append(step.astep(None, offset=off)[0])
            except _abi.PGBError as e:
                out.append(str(e).split(" by astep")[0])
        return out

    plain = run(())
    assert [isinstance(o, str) for o in plain] == [False, True, False, False, True, False]
    again = run((3,))
    for a, b in zip(plain, again):
        assert (a == b) if isinstance(a, str) else np.array_equal(a, b)
