"""The sampler at the ends of the double range -- GPU half (tests/test_extremes.py states the properties and holds
the CPU oracle to them).

Every check of that file is repeated on the HIP library, and the HIP chain on the TRANSFORMED data is held to the
oracle's per step: sum_trees, the exported trees, the counters.  The device has code here that the oracle does not
share -- the order-key build (k_key_stage, the radix sort of float32 bit patterns, k_key_bounds, k_key_assign with
its (float)x conversions), the F32 instances of k_rows / k_rows_mk, which fall back to the float64 value only on
equal keys, and k_ctrl reading the key of a split value with the value -- so the same chains run with the order keys
forced on: a column of neighbouring doubles is ONE key (every lane fetches the float64 value), a column beyond the
float32 range is two keys, the six levels put -inf / +inf next to the key of a missing value."""
import numpy as np
import pytest

import _extreme_cases as E
import test_extremes as T
from _cases import step_keeping_outputs
from pymc_bart_amd import _abi
from test_caps_gpu import _p128

pytestmark = pytest.mark.gpu

FAMILIES = ["normal", "bernoulli_probit", "categorical"]    # categorical: K = 3, the row pass of K-vector leaves
TWINS = list(E.LADDERS) + ["six_level"]


def _twin(backend, twin, family, base=None):
    if twin == "six_level":
        return T.check_six_level(backend, family, base)
    return T.check_ladder(backend, twin, family, base)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("twin", TWINS)
def test_float64_row_pass_on_extreme_columns(hip, oracle, twin, family):
    c, Xt, g = _twin(hip, twin, family)
    assert g["sampler"].backend.lib.backend_name == "hip-gfx950"
    E.assert_same_run(g, E.run_chain(c, oracle, Xt), (twin, family))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("twin", TWINS)
def test_order_keys_forced_on_extreme_columns(hip, oracle, monkeypatch, twin, family):
    make = E.six_level_case if twin == "six_level" else E.ladder_case
    base = T.base_run(("six" if twin == "six_level" else "ladder", family), lambda: E.with_family(make(), family), hip)
    c, Xt, plain = _twin(hip, twin, family, base)                 # without keys (the data are far below the threshold)
    monkeypatch.setenv("PGB_X32_MIN_MB", "0")                     # read when the data are set
    c, Xt, keyed = _twin(hip, twin, family, base)                 # ... equals the untransformed chain
    E.assert_same_run(keyed, plain, (twin, family, "keys against none"))
    E.assert_same_run(keyed, E.run_chain(c, oracle, Xt), (twin, family, "keys against the oracle"))
    kb = E.run_chain(c, hip)                                      # the untransformed data with keys, for completeness
    E.assert_same_run(kb, base[1], (twin, family, "base with keys"))


@pytest.mark.parametrize("family", ["normal", "bernoulli_probit"])
@pytest.mark.parametrize("keys", [False, True], ids=["float64", "keys"])
def test_onehot_and_signed_zero_twins(hip, oracle, monkeypatch, family, keys):
    T.base_run(("onehot", family), lambda: E.with_family(E.onehot_case(), family), hip)
    T.base_run(("ladder", family), lambda: E.with_family(E.ladder_case(), family), hip)
    if keys:
        monkeypatch.setenv("PGB_X32_MIN_MB", "0")
    for check in (T.check_onehot, T.check_signed_zeros):
        c, Xt, g = check(hip, family)
        E.assert_same_run(g, E.run_chain(c, oracle, Xt), (check.__name__, family, keys))


@pytest.mark.parametrize("family", ["normal", "bernoulli_probit"])
@pytest.mark.parametrize("twin", ["full", "six_level"])
def test_hundred_particles_on_extreme_columns(hip, oracle, twin, family):
    big = _p128(hip)
    make = E.six_level_case if twin == "six_level" else E.ladder_case
    c = dict(E.with_family(make(), family), P=100)
    r = E.run_chain(c, big)
    E.assert_alive(r)
    assert r["sampler"].backend.lib.max_particles == 128
    c, Xt, g = _twin(big, twin, family, (c, r))
    E.assert_same_run(g, E.run_chain(c, oracle, Xt), (twin, family, "P = 100"))


@pytest.mark.parametrize("k", [64, -64, 1000, -1000])
@pytest.mark.parametrize("response,family", T.LINEAR)
def test_regressed_column_scales_exactly_on_the_device(hip, oracle, response, family, k):
    c, g = T.check_column_scale(hip, response, family, k)
    E.assert_same_run(g, E.run_chain(c, oracle, E.scale_column(c["X"], 0, k)), (response, family, k))


def test_refusals_and_the_low_end_as_the_oracle(hip, oracle):
    assert T.check_column_refusals(hip) == T.check_column_refusals(oracle)       # the same codes, the same text
    assert T.check_range_exp_refusals(hip) == T.check_range_exp_refusals(oracle)
    c, Xt, g = T.check_tiny_column(hip)
    E.assert_same_run(g, E.run_chain(c, oracle, Xt), "a regressed column of subnormals")


@pytest.mark.parametrize("k", [300, -300, "MIN_RANGE_EXP", "MAX_RANGE_EXP"])
def test_normal_chain_scales_exactly_with_the_response_on_the_device(hip, oracle, k):
    ck, g = T.check_response_scale(hip, range_exp=getattr(_abi, k)) if isinstance(k, str) else T.check_response_scale(hip, k=k)
    E.assert_same_run(g, E.run_chain(ck, oracle), ("response scale", k))


@pytest.mark.parametrize("how", ["host", "async"])
def test_six_levels_through_every_stepping_entry_point(hip, oracle, how):
    """pgb_step_host called directly, and pgb_step_async / pgb_sync with sum_trees read from the chain image."""
    def stepper(s, tune):
        st, _, err = step_keeping_outputs(s, tune, how)
        assert err is None
        return st

    c, Xt, g = T.check_six_level(hip, "normal", stepper=stepper)
    E.assert_same_run(g, E.run_chain(c, oracle, Xt), ("six_level", how))
