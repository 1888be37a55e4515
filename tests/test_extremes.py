"""The sampler at the ends of the double range, on the CPU oracle (tests/test_extremes_gpu.py repeats every check on
the device and compares the two).

Constant leaves see a continuous column only through the ORDER of its values and a one-hot column only through
EQUALITY: any order-preserving (injective) recoding of the covariates -- onto neighbouring doubles, onto values far
beyond the float32 range, onto subnormals and infinities -- must leave the chain where it was, bit for bit.  Linear
leaves see a regressed column through u = x 2^-ex and must scale exactly with a power of two; a Normal chain must
scale exactly with a power-of-two rescaling of the response over the whole accepted range_exp interval; and what lies
beyond either (a column at 2^1022 or more, a range_exp outside [PGB_MIN_RANGE_EXP, PGB_MAX_RANGE_EXP]) is refused
with a message that names it (include/pgbart_spec.h, pgb_pow2's domain).
"""
import dataclasses

import numpy as np
import pytest

import _extreme_cases as E
from pymc_bart_amd import _abi
from pymc_bart_amd.sampler import PyBartSettings, PySampler

FAMILIES = ["normal", "bernoulli_probit"]
COLUMN_K = [64, -64, 512, -512, 1000, -1000]
RESPONSE_K = [64, -64, 300, -300]
BASES = {}


def base_run(key, make, backend):
    """One base chain per (case, family, backend), shared by the tests that compare twins with it; never changed."""
    key = (key, backend.lib.backend_name, backend.lib.max_particles)
    if key not in BASES:
        c = make()
        r = E.run_chain(c, backend)
        E.assert_alive(r)
        r.pop("sampler")                      # (the native handle goes with the run: only its record is kept)
        BASES[key] = (c, r)
    return BASES[key]


# ------------------------------------------------------------------ the builders themselves
def test_ladders_are_strictly_increasing_and_what_they_say():
    for kind in E.LADDERS:
        for k in (1, 2, 6, 9, 10, 11, 1025):
            E.ladder(kind, k)
    with np.errstate(over="ignore", under="ignore"):
        assert len(np.unique(E.ladder("adjacent", 1025).astype(np.float32))) == 1
        assert np.all(np.isinf(E.ladder("f32_overflow", 1025).astype(np.float32)))
        assert np.all(E.ladder("f32_underflow", 1025).astype(np.float32) == 0)
    assert np.all(np.abs(E.ladder("f32_overflow", 1025)) > 1e39) and np.all(np.abs(E.ladder("f32_underflow", 1025)) < 1e-50)
    full = E.ladder("full", 1025)
    for v in (-np.inf, -E.DBL_MAX, -E.DBL_MIN, -1e-310, -5e-324, 5e-324, 1e-310, E.DBL_MIN, E.DBL_MAX, np.inf):
        assert v in full
    c = E.ladder_case()
    Xt, maps = E.remap(c["X"], ["full"] * 4)
    assert np.array_equal(np.isnan(Xt), np.isnan(c["X"])) and len(maps[0][0]) == 1025 and len(maps[3][0]) < 12
    for j in range(4):   # order kept: ranks are the same
        ok = ~np.isnan(Xt[:, j])
        assert np.array_equal(np.argsort(np.argsort(Xt[ok, j], kind="stable")), np.argsort(np.argsort(c["X"][ok, j], kind="stable")))


# ------------------------------------------------------------------ rank invariance, constant leaves
def check_ladder(backend, kind, family, base=None):
    c, r = base_run(("ladder", family), lambda: E.with_family(E.ladder_case(), family), backend) if base is None else base
    Xt, maps = E.remap(c["X"], [kind] * 4)
    t = E.run_chain(c, backend, Xt)
    E.assert_same_chain(r, t, maps, (kind, family))
    E.assert_splits_on(t, range(4), (kind, family))
    return c, Xt, t


def check_six_level(backend, family, base=None, stepper=None):
    c, r = base_run(("six", family), lambda: E.with_family(E.six_level_case(), family), backend) if base is None else base
    Xt, maps = E.six_level_twin(c)
    t = E.run_chain(c, backend, Xt, stepper=stepper)
    E.assert_same_chain(r, t, maps, ("six_level", family))
    var, split = E.inner_splits(t)
    on3 = split[var == 3]
    assert np.any(np.isinf(on3)), "no accepted split at an infinite value"
    assert np.any((on3 != 0) & (np.abs(on3) < E.DBL_MIN)), "no accepted split at a subnormal value"
    return c, Xt, t


def check_onehot(backend, family):
    c, r = base_run(("onehot", family), lambda: E.with_family(E.onehot_case(), family), backend)
    Xt, maps = E.onehot_twin(c)
    t = E.run_chain(c, backend, Xt)
    E.assert_same_chain(r, t, maps, ("onehot", family))
    E.assert_splits_on(t, [3], ("onehot", family))
    return c, Xt, t


def check_signed_zeros(backend, family):
    c, r = base_run(("ladder", family), lambda: E.with_family(E.ladder_case(), family), backend)
    Xt = E.signed_zero_twin(c)
    t = E.run_chain(c, backend, Xt)
    E.assert_same_chain(r, t, None, ("signed zeros", family), equal_splits=True)
    var, split = E.inner_splits(t)
    assert np.any(split[var == 3] == 0.0), "no accepted split at the zero group"
    return c, Xt, t


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", E.LADDERS)
def test_chain_sees_only_the_order_of_a_continuous_column(oracle, kind, family):
    check_ladder(oracle, kind, family)


@pytest.mark.parametrize("family", FAMILIES)
def test_six_levels_from_minus_infinity_to_infinity(oracle, family):
    check_six_level(oracle, family)


@pytest.mark.parametrize("family", FAMILIES)
def test_onehot_column_recoded_injectively_not_monotonically(oracle, family):
    check_onehot(oracle, family)


@pytest.mark.parametrize("family", FAMILIES)
def test_half_of_a_zero_group_as_negative_zero(oracle, family):
    check_signed_zeros(oracle, family)


# ------------------------------------------------------------------ linear / mix leaves: a regressed column times 2^k
LINEAR = [("linear", "normal"), ("mix", "normal"), ("linear", "categorical")]


def check_column_scale(backend, response, family, k):
    c, r = base_run(("lin", response, family), lambda: E.linear_case(response, family), backend)
    slope, xbar = E.slopes_on(r, 0)
    assert np.count_nonzero(slope) >= 10, "the base chain hardly regresses on the scaled column"
    t = E.run_chain(c, backend, E.scale_column(c["X"], 0, k))
    what = (response, family, k)
    assert np.array_equal(r["sum_trees"], t["sum_trees"]), what
    for f in ("var", "count", "value", "svar"):
        assert np.array_equal(r[f], t[f]), (what, f)
    on0 = r["var"] == 0
    assert np.array_equal(np.ldexp(r["split"][on0], k), t["split"][on0]) and np.array_equal(r["split"][~on0], t["split"][~on0], equal_nan=True), what
    tslope, txbar = E.slopes_on(t, 0)
    assert np.array_equal(tslope, np.ldexp(slope, -k)) and np.array_equal(txbar, np.ldexp(xbar, k)), what
    assert np.all(np.isfinite(tslope)) and np.count_nonzero(tslope) == np.count_nonzero(slope), what
    other = r["svar"] != 0
    assert np.array_equal(r["slope"][other], t["slope"][other]) and np.array_equal(r["xbar"][other], t["xbar"][other]), what
    assert r["counters"] == t["counters"] and t["counters"][-1]["saturations"] == 0, what
    return c, t


@pytest.mark.parametrize("k", COLUMN_K)
@pytest.mark.parametrize("response,family", LINEAR)
def test_regressed_column_scales_exactly_with_a_power_of_two(oracle, response, family, k):
    check_column_scale(oracle, response, family, k)


# ------------------------------------------------------------------ the response times 2^k
def check_response_scale(backend, k=None, range_exp=None):
    c, r = base_run(("ladder", "normal"), lambda: E.with_family(E.ladder_case(), "normal"), backend)
    ck = E.scale_response(c, k, range_exp)
    k = ck["k"]
    t = E.run_chain(ck, backend)
    assert t["settings"].range_exp == r["settings"].range_exp + k
    assert np.array_equal(t["sum_trees"], np.ldexp(r["sum_trees"], k)), k
    for f in ("var", "split", "count"):
        assert np.array_equal(r[f], t[f], equal_nan=True), (k, f)
    assert np.array_equal(t["value"], np.ldexp(r["value"], k)), k
    assert t["state"]["leaf_sd"][0] == np.ldexp(r["state"]["leaf_sd"][0], k), k
    assert r["counters"] == t["counters"] and t["counters"][-1]["saturations"] == 0, k
    return ck, t


@pytest.mark.parametrize("k", RESPONSE_K)
def test_normal_chain_scales_exactly_with_the_response(oracle, k):
    check_response_scale(oracle, k=k)


@pytest.mark.parametrize("end", ["MIN_RANGE_EXP", "MAX_RANGE_EXP"])
def test_both_ends_of_the_range_exp_interval_run_the_exactly_scaled_chain(oracle, end):
    check_response_scale(oracle, range_exp=getattr(_abi, end))


# ------------------------------------------------------------------ refusals, and the documented low end
def check_column_refusals(backend):
    """A regressed column needs max|x| < 2^1022: 2^-ex would be 0.0 (7.4e307, 1.5e308) or ex out of pgb_pow2's
    domain altogether (inf).  Refused by pgb_set_data, naming the column; the same data under constant leaves run."""
    msgs = []
    for response in ("linear", "mix"):
        c = E.linear_case(response)
        for big in (7.4e307, 1.5e308, np.inf):
            Xt = c["X"].copy()
            Xt[17, 1] = -big
            with pytest.raises(_abi.PGBError, match=r"pgb_set_data failed \(code -1\).*column 1 .*max\|x\| = .*2\^1022") as ei:
                E.run_chain(c, backend, Xt)
            assert f"{big:g}" in str(ei.value)
            msgs.append(str(ei.value))
            ok = dict(c, response="constant")
            r = E.run_chain(ok, backend, Xt)
            assert np.all(np.isfinite(r["sum_trees"])) and r["counters"][-1]["saturations"] == 0
            E.assert_alive(r)
    # the largest column that is regressed on: just below 2^1022
    c = E.linear_case("linear")
    Xt = E.scale_column(c["X"], 1, 1019)
    Xt[17, 1] = np.nextafter(2.0 ** 1022, 0.0)
    r = E.run_chain(c, backend, Xt)
    assert np.all(np.isfinite(r["sum_trees"])) and r["counters"][-1]["saturations"] == 0
    assert np.count_nonzero(E.slopes_on(r, 1)[0]) > 0
    return msgs


def check_range_exp_refusals(backend):
    c = E.ladder_case()
    st = E.settings(c)
    msgs = []
    for bad in (_abi.MIN_RANGE_EXP - 1, _abi.MAX_RANGE_EXP + 1, 517, -490, 1030, -1100):
        with pytest.raises(_abi.PGBError, match=rf"pgb_create failed \(code -1\).*range_exp = {bad} is outside \[-480, 480\]") as ei:
            PySampler(dataclasses.replace(st, range_exp=bad), c["X"], c["Y"], c["rules"], np.ones(4), backend=backend)
        msgs.append(str(ei.value))
    for good in (_abi.MIN_RANGE_EXP, _abi.MAX_RANGE_EXP):
        PySampler(dataclasses.replace(st, range_exp=good), c["X"], c["Y"], c["rules"], np.ones(4), backend=backend)
    return msgs


def check_tiny_column(backend):
    """max|x| = 2^-1040 on a regressed column: the exponent clamp at -1000 leaves u = x 2^1000 under pgb_lin_fit's
    spread test -- every slope on the column is exactly 0, nothing saturates, nothing is refused."""
    c, r0 = base_run(("lin", "linear", "normal"), lambda: E.linear_case("linear", "normal"), backend)
    Xt = c["X"].copy()
    Xt[:, 0] = np.ldexp(Xt[:, 0] / np.abs(Xt[:, 0]).max(), -1040)     # subnormals; the ORDER of the column is kept
    assert np.abs(Xt[:, 0]).max() == 2.0 ** -1040 and len(np.unique(Xt[:, 0])) > 1000
    r = E.run_chain(c, backend, Xt)
    assert np.any(r["var"] == 0) and np.all(np.isfinite(r["sum_trees"]))
    assert np.all(r["svar"] != 0) and np.all(E.slopes_on(r, 0)[0] == 0.0)
    assert np.count_nonzero(r["slope"][r["svar"] == 1]) > 0            # the other columns are still regressed on
    assert r["counters"][-1]["saturations"] == 0
    E.assert_alive(r)
    return c, Xt, r


def test_regressed_column_beyond_two_to_the_1022_is_refused_by_name(oracle):
    check_column_refusals(oracle)


def test_range_exp_beyond_either_end_is_refused_by_pgb_create(oracle):
    check_range_exp_refusals(oracle)


def test_from_data_refuses_a_response_beyond_the_range_before_anything_is_created(oracle, monkeypatch):
    c = E.ladder_case()
    created = []
    monkeypatch.setattr(oracle.lib.lib, "pgb_create", lambda *a: created.append(a) or 0, raising=False)
    big = np.ldexp(c["Y"], 478)                                   # max|y| ~ 2^480: range exponent 483
    with pytest.raises(ValueError, match=r"max\|y\| = [0-9.]+e\+14\d.*2\^48\d is outside \[2\^-480, 2\^480\]"):
        PyBartSettings.from_data(c["X"], big, m=E.M)
    with pytest.raises(ValueError, match=r"max\|y\| = 1e\+200"):
        PyBartSettings.from_data(c["X"], c["Y"], m=E.M, y_obs=np.where(np.arange(E.N) == 5, -1e200, c["Y"]))
    for bad in (-481, 481):
        with pytest.raises(ValueError, match=rf"range_exp = {bad} is outside \[-480, 480\]"):
            PyBartSettings.from_data(c["X"], c["Y"], m=E.M, range_exp=bad)
    assert PyBartSettings.from_data(c["X"], np.ldexp(c["Y"], 470), m=E.M).range_exp <= _abi.MAX_RANGE_EXP
    assert PyBartSettings.from_data(c["X"], c["Y"], m=E.M, range_exp=-480).range_exp == -480
    assert not created


def test_regressed_column_below_the_exponent_clamp_has_constant_leaves(oracle):
    check_tiny_column(oracle)
