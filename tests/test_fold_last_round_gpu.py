"""The folded last round of a tree (k_ctrl): a PH_ROUND slot whose proposed round is empty and final ends the tree
itself, so a tree update takes one control launch and one row pass fewer.  PGB_FOLD_LAST (read when a sampler is
created; default on, 0 = the unfolded path) must change NOTHING but the count of working slots:

  * per step, sum_trees, the variable-inclusion counts and the exported trees; the tuned leaf_sd and split weights;
    every counter but `slots`; the chain image at the end -- bit for bit between the folded run, the unfolded run and
    the CPU oracle (each GPU setting runs its own sampler);
  * STAR cases (tests/_fold_cases.py; held on the CPU by tests/test_fold_last_round.py): every tree update folds --
    slots(unfolded) - slots(folded) == tree_updates;
  * where attempts can fail (missing values, one-valued one-hot / subset columns) the last proposed round is not
    always free of attempts: strictly fewer folds than tree updates, the same results.
"""
import numpy as np
import pytest

from _cases import run_case
from _fold_cases import NO_STAR, NOT_ALWAYS, OTHER_INSTANCES, STAR, fold_case, oracle_run, settings_of
from pymc_bart_amd.image import ChainImage, differing_fields
from pymc_bart_amd.sampler import PySampler

pytestmark = pytest.mark.gpu


def _same(a, b, what):
    assert np.array_equal(a["sum_trees"], b["sum_trees"]), what
    assert np.array_equal(a["vi"], b["vi"]), what
    assert len(a["trees"]) == len(b["trees"])
    for x, y in zip(a["trees"], b["trees"]):
        assert np.array_equal(x, y), what
    for k in ("particle_steps", "tree_updates", "rows_touched", "rounds", "partitions", "saturations"):
        assert a["counters"][k] == b["counters"][k], (what, k, a["counters"], b["counters"])
    assert np.array_equal(a["split_weights"], b["split_weights"]), what
    assert np.array_equal(a["state"]["leaf_sd"], b["state"]["leaf_sd"]), what
    assert a["state"]["iter"] == b["state"]["iter"] and a["state"]["lower"] == b["state"]["lower"], what
    ia, ib = ChainImage.parse(a["sampler"].checkpoint()), ChainImage.parse(b["sampler"].checkpoint())
    assert differing_fields(ia, ib) == [], what


def _slots(res):
    return int(res["sampler"].counters.as_dict()["slots"])


def _three_runs(name, hip, oracle, monkeypatch):
    c = fold_case(name)
    monkeypatch.setenv("PGB_FOLD_LAST", "1")
    folded = run_case(c, hip)
    monkeypatch.setenv("PGB_FOLD_LAST", "0")
    unfolded = run_case(c, hip)
    monkeypatch.delenv("PGB_FOLD_LAST")
    o = oracle_run(name, oracle)
    _same(folded, o, f"{name}: folded run against the oracle")
    _same(unfolded, o, f"{name}: unfolded run against the oracle")
    _same(folded, unfolded, f"{name}: folded against unfolded")
    saved = _slots(unfolded) - _slots(folded)
    print(f"{name}: tree_updates {o['counters']['tree_updates']}, slots unfolded {_slots(unfolded)}, folded {_slots(folded)}")
    return saved, int(o["counters"]["tree_updates"])


@pytest.mark.parametrize("name", STAR)
def test_every_tree_update_folds_and_nothing_else_changes(hip, oracle, monkeypatch, name):
    saved, updates = _three_runs(name, hip, oracle, monkeypatch)
    assert saved == updates


@pytest.mark.parametrize("name", NO_STAR)
def test_limits_and_ties_give_the_same_chain(hip, oracle, monkeypatch, name):
    """The node table full / leaves of fewer than two rows (no attempt although a node is popped), and a constant
    response (every particle ties: the resampling thresholds meet the cumulative weights at equality)."""
    saved, updates = _three_runs(name, hip, oracle, monkeypatch)
    assert 0 <= saved <= updates


@pytest.mark.parametrize("name", NOT_ALWAYS)
def test_no_fold_where_the_last_round_has_an_attempt(hip, oracle, monkeypatch, name):
    saved, updates = _three_runs(name, hip, oracle, monkeypatch)
    assert 0 <= saved < updates


@pytest.mark.parametrize("name", OTHER_INSTANCES)
def test_kvector_and_linear_instances_keep_the_unfolded_path(hip, oracle, monkeypatch, name):
    saved, _ = _three_runs(name, hip, oracle, monkeypatch)
    assert saved == 0


def test_default_is_folded(hip, oracle, monkeypatch):
    c = fold_case("p5")
    monkeypatch.delenv("PGB_FOLD_LAST", raising=False)
    d = run_case(c, hip)
    monkeypatch.setenv("PGB_FOLD_LAST", "0")
    u = run_case(c, hip)
    assert _slots(u) - _slots(d) == d["counters"]["tree_updates"]


def test_several_steps_in_one_async_call_fold_into_the_lone_final(hip, oracle, monkeypatch):
    """One tree per step: every tree is the last of its step.  Stepwise (the last tree of the last requested step:
    the folded slot issues the lone CMD_FINAL and publishes the progress word) against several steps in one
    pgb_step_async call (only the very last tree has no successor), folded and unfolded."""
    c = fold_case("one_tree_per_step")
    st = settings_of(c)
    p = c["X"].shape[1]
    runs = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("PGB_FOLD_LAST", fold)
        a = PySampler(st, c["X"], c["Y"], np.zeros(p, np.int32), np.ones(p), backend=hip)
        b = PySampler(st, c["X"], c["Y"], np.zeros(p, np.int32), np.ones(p), backend=hip)
        for s in (a, b):
            s.set_likelihood([0.8])
        for _ in range(12):
            sa, va = a.step(True)
        b.step_async(True, 7)
        b.step_async(True, 4)
        sb, vb = b.step(True)
        ca, cb = a.sync(), b.sync()
        assert np.array_equal(sa, sb) and np.array_equal(va, vb)
        for k in ("particle_steps", "tree_updates", "rows_touched", "rounds", "partitions"):
            assert ca[k] == cb[k], (fold, k, ca, cb)
        assert differing_fields(ChainImage.parse(a.checkpoint()), ChainImage.parse(b.checkpoint())) == []
        runs[fold] = (sa, va, ca, a)
    monkeypatch.delenv("PGB_FOLD_LAST")
    o = PySampler(st, c["X"], c["Y"], np.zeros(p, np.int32), np.ones(p), backend=oracle)
    o.set_likelihood([0.8])
    for _ in range(12):
        so, vo = o.step(True)
    co = o.sync()
    for fold in ("1", "0"):
        sa, va, ca, a = runs[fold]
        assert np.array_equal(sa, so) and np.array_equal(va, vo)
        for k in ("particle_steps", "tree_updates", "rows_touched", "rounds", "partitions"):
            assert ca[k] == co[k], (fold, k, ca, co)
        assert differing_fields(ChainImage.parse(a.checkpoint()), ChainImage.parse(o.checkpoint())) == []
    assert runs["0"][2]["slots"] - runs["1"][2]["slots"] == co["tree_updates"] == 12
