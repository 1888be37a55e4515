"""What the cases of the folded last round (tests/_fold_cases.py) are there for, held on the CPU with the oracle:
the GPU test (tests/test_fold_last_round_gpu.py) asserts a fold for every tree update of a STAR case, which holds
when no tree of the run has an empty round 0 and no attempt of the run can fail."""
import numpy as np
import pytest

from _cases import step_trees
from _fold_cases import ALL, STAR, fold_case, oracle_run, settings_of, trees_with_an_empty_round0


@pytest.mark.parametrize("name", STAR)
def test_star_cases_have_no_tree_with_an_empty_round0_and_no_failing_attempt(oracle, name):
    c = fold_case(name)
    assert not np.isnan(c["X"]).any() and c["rules"] is None          # an attempt finds its row and grows
    assert 130 <= c["X"].shape[0] <= 2100 and 3 <= c["X"].shape[1] <= 6 and 1 <= c["m"] <= 10 and 10 <= c["steps"] <= 30
    ctr = oracle_run(name, oracle)["counters"]
    assert trees_with_an_empty_round0(c, oracle, ctr["tree_updates"]) == []
    assert ctr["rounds"] >= 2 * ctr["tree_updates"] and ctr["partitions"] >= ctr["tree_updates"]
    assert ctr["saturations"] == 0


def test_every_case_is_small():
    for name in ALL:
        c = fold_case(name)
        assert 130 <= c["X"].shape[0] <= 2100 and 3 <= c["X"].shape[1] <= 6 and 1 <= c["m"] <= 10 and 10 <= c["steps"] <= 30


def test_the_tuned_case_rebuilds_its_sampler(oracle):
    c = fold_case("normal_p40_tuned")
    bt, _ = settings_of(c).batch_sizes()
    assert (c["steps"] // 2) * bt > 2 * c["m"]                        # tuned iterations beyond m: `rebuild`
    r = oracle_run("normal_p40_tuned", oracle)
    assert not np.array_equal(r["split_weights"], r["split_weights_init"])
    assert r["state"]["leaf_sd"][0] != settings_of(c).init_leaf_sd


def test_the_deep_case_runs_well_over_eight_rounds_a_tree(oracle):
    ctr = oracle_run("deep", oracle)["counters"]
    assert ctr["rounds"] > 12 * ctr["tree_updates"]                   # (the label ring has 8 generations)


def test_the_caps_case_fills_the_node_table_and_runs_out_of_rows(oracle):
    c = fold_case("caps_n130")
    r = oracle_run("caps_n130", oracle)
    full = short = 0
    for packed in r["trees"]:
        for var, left, right, count in step_trees(c, packed):
            full += len(var) == 255
            short += int(((var < 0) & (count < 2)).sum())
    assert full > 0 and short > 0


def test_the_failing_case_has_attempts_that_fail(oracle):
    c = fold_case("nan_onehot_subset")
    assert np.isnan(c["X"][:, 1]).mean() > 0.8 and list(c["rules"]) == [0, 0, 1, 2]
    ctr = oracle_run("nan_onehot_subset", oracle)["counters"]
    assert ctr["tree_updates"] > 0
    vars_used = np.concatenate(oracle_run("nan_onehot_subset", oracle)["split_vars"])
    assert not np.isin(vars_used, [2, 3]).any()                       # no grow on the one-valued columns ever succeeds
