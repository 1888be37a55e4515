"""Saturating steps -- GPU half: the HIP library counts fixed-point saturation events as the oracle does.

The cases of tests/_cases.py (SAT_CASES) move `counters.saturations`, which every other GPU test only sees at 0.  On
the device the count is made where the values are produced: by the writer group of a chunk in the row pass that starts
a tree (`k_rows`: st, r, r^2 and (r - o)^2; `k_rows_mk`: st of every output), pad rows skipped; for the running sd of
a tree's predictions while tuning, in the same pass when it also ends the previous tree of the step, and in the lone
FINAL pass that ends a step.  A count dropped, doubled per particle group or taken over pad rows changes the per-step
counts below; a clamp that differs changes the chain.  Every comparison with the oracle is exact; what each case
reaches is pinned on the oracle in tests/test_saturation.py."""
import numpy as np
import pytest

from _cases import run_sat_case, sat_digest, sat_events
from pymc_bart_amd import _abi
from pymc_bart_amd.image import ChainImage, differing_fields
from pymc_bart_amd.pgbart import PGBART, BARTOp, NormalLikelihood
from test_caps_gpu import KNOBS, _p128, _same_image
from test_parity_gpu import _assert_same
from test_saturation import SAT_CASES, SAT_GOLD, SAT_IDS, oracle_sat_run

pytestmark = pytest.mark.gpu


def _same_sat_run(g, o):
    _assert_same(g, o)
    assert g["sat"] == o["sat"], (sat_events(g).tolist(), sat_events(o).tolist())
    assert g["raised"] == o["raised"] and g["raised_count"] == o["raised_count"]


@pytest.mark.parametrize("name", SAT_CASES, ids=SAT_IDS)
def test_sat_hip_equals_oracle_and_golden(hip, name):
    c, o = oracle_sat_run(name)
    g = run_sat_case(c, hip)
    lib = g["sampler"].backend.lib
    assert lib.backend_name == "hip-gfx950" and lib.max_particles == (128 if c["P"] > 64 else 64)
    _same_sat_run(g, o)
    assert sat_digest(g) == SAT_GOLD[name]
    assert g["counters"]["saturations"] > 0
    _same_image(g["sampler"], o["sampler"])


@pytest.mark.parametrize("name", ["sat/normal_outliers", "sat/categorical_k3"])
def test_sat_two_particles_per_lane_build_gives_the_same_counts(hip, name):
    c, o = oracle_sat_run(name)
    assert c["P"] <= 64
    g = run_sat_case(c, _p128(hip))
    assert g["sampler"].backend.lib.max_particles == 128
    _same_sat_run(g, o)
    assert sat_digest(g) == SAT_GOLD[name]


@pytest.mark.parametrize("knob", list(KNOBS))
@pytest.mark.parametrize("name", ["sat/normal_outliers", "sat/poisson_small_range", "sat/categorical_k3",
                                  "sat/normal_all_rows_top"])
def test_sat_counts_do_not_depend_on_the_knobs(hip, monkeypatch, name, knob):
    """The odd and the wide launch geometry change which group of a chunk writes and how many blocks share a chunk;
    the forced order keys take the other instances of the row passes."""
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)
    c, o = oracle_sat_run(name)
    g = run_sat_case(c, hip)
    assert g["sampler"].backend.lib.backend_name == "hip-gfx950"
    _same_sat_run(g, o)
    assert sat_digest(g) == SAT_GOLD[name]


def _prefix(c, steps):
    return dict(c, steps=int(steps), tune_steps=c.get("tune_steps", c["steps"] // 2))


@pytest.mark.parametrize("cut", [3, 4])
def test_sat_chain_migrates_at_the_saturating_step(hip, oracle, cut):
    """sat/normal_outliers, whose step 3 saturates: the chain moves GPU -> oracle and oracle -> GPU right before and
    right after that step and continues identically -- the restored handle takes the counter from the image, so the
    raised flags are the uninterrupted chain's.  The images written at the cut agree field for field."""
    c, o = oracle_sat_run("sat/normal_outliers")
    for first, then in ((hip, oracle), (oracle, hip)):
        g = run_sat_case(c, first, checkpoint_at={cut: then})
        _same_sat_run(g, o)
        assert sat_digest(g) == SAT_GOLD[c["name"]]
        _same_image(g["sampler"], o["sampler"])
    stopped = _prefix(c, cut)
    ia = _same_image(run_sat_case(stopped, hip)["sampler"], run_sat_case(stopped, oracle)["sampler"])
    assert int(ia.header.ctr.saturations) == (0 if cut == 3 else sat_events(o)[3])
    if cut == 4:
        assert int(ia.header.ctr.saturations) > 0


@pytest.mark.parametrize("how", ["device", "async"])
@pytest.mark.parametrize("name", ["sat/normal_outliers", "sat/categorical_k3", "sat/probit_two_per_step"])
def test_sat_step_variants_give_the_same_counts(hip, name, how):
    """pgb_step (device output) and pgb_step_async + pgb_sync against pgb_step_host: the same counter after every
    step, the same errors, the same sum_trees (read from the device buffer / from the chain image) and trees."""
    c, o = oracle_sat_run(name)
    g = run_sat_case(c, hip, how=how)
    assert g["sat"] == o["sat"] and g["raised"] == o["raised"] and g["raised_count"] == o["raised_count"]
    assert np.array_equal(g["sum_trees"], o["sum_trees"])
    for x, y in zip(g["trees"], o["trees"]):
        assert np.array_equal(x, y)
    assert g["counters"] == o["counters"]
    if how == "device":
        assert np.array_equal(g["vi"], o["vi"])


def test_sat_sync_raises_with_the_total_of_a_span_on_gpu(hip, oracle):
    """One asynchronous span over all steps of sat/normal_one_tree (every step saturates, no input moves): `sync`
    raises once, with the oracle's total."""
    from test_saturation import _sampler

    c, o = oracle_sat_run("sat/normal_one_tree")
    s = _sampler(c, hip)
    s.set_likelihood([0.8])
    t = _sampler(c, oracle)
    t.set_likelihood([0.8])
    t.step_async(False, c["steps"])
    with pytest.raises(_abi.PGBError) as eo:
        t.sync()
    s.step_async(False, c["steps"])
    with pytest.raises(_abi.PGBError) as eg:
        s.sync()
    assert str(eg.value) == str(eo.value) and str(eg.value).startswith(f"{int(t.counters.saturations)} fixed-point")
    assert s.counters.saturations == t.counters.saturations > 0
    assert differing_fields(ChainImage.parse(s.checkpoint()), ChainImage.parse(t.checkpoint())) == []


def test_sat_public_layer_reports_the_step_and_goes_on(hip, oracle):
    """PGBART.astep on the HIP backend, as tests/test_host_logic.py runs it on the oracle: an offset that leaves the
    range raises naming its astep, the next asteps run, and the chain is the oracle's."""
    rng = np.random.default_rng(5)
    X = rng.normal(size=(300, 3))
    Y = X[:, 0] - X[:, 1] + rng.normal(0, 0.2, 300)
    far, none = np.full(300, 1.0e4), np.zeros(300)
    out = {}
    for name, be in (("hip", hip), ("oracle", oracle)):
        step = PGBART([BARTOp(X, Y, m=10)], num_particles=5, likelihood=NormalLikelihood(1.0), random_seed=3, backend=be)
        got = [step.astep(None)[0]]
        assert step.sampler.backend.lib.backend_name == ("hip-gfx950" if name == "hip" else "oracle-cpu")
        with pytest.raises(_abi.PGBError, match="by astep 2") as e:
            step.astep(None, offset=far)
        got.append(str(e.value))
        got.append(step.astep(None, offset=none)[0])      # the chain is usable again
        got.append(step.astep(None)[0])
        got.append(int(step.sampler.counters.saturations))
        out[name] = got
    for a, b in zip(out["hip"], out["oracle"]):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert out["hip"][-1] > 0
