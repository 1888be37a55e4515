"""A handle's history leaves no trace -- CPU half: the oracle's own setters.

The GPU half (tests/test_handle_history_gpu.py) holds the HIP library to the oracle on schedules that move the
inputs at every astep, the way PGBART.astep drives a handle inside a PyMC model (set_response(y - other terms) for a
Normal model, set_offset(other terms) for a per-row family).  That comparison leans on the oracle's setters; here
they are pinned on their own: at every cut of a schedule a FRESH oracle handle -- built with the inputs in force at
the cut, then restore(image) -- continues bit for bit to the end and ends with the same image bytes.  Likewise for
pgb_set_data called again (before any step, and between a checkpoint() and the restore() of that image) and for a
call that is refused.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from _cases import (apply_inputs, assert_same_run, check_schedule, history_sampler, make_history_case, moving_inputs,
                    run_schedule, set_data_rc, step_record, end_record)
from pymc_bart_amd import _abi

PGB_E_INVALID = -1  # include/pgbart.h
CUTS = (1, 5, 6, 9)   # while tuning, the last tuning step, the first draw, in the draws (None / zero steps: 4 and 8)

SCHEDULES = [
    ("normal", {}),
    ("bernoulli_probit", {}), ("bernoulli_logit", {}), ("poisson_log", {}), ("negbin_log", {}), ("gamma_log", {}),
    ("asymmetric_laplace", {}), ("student_t", {}),
    ("categorical:3", {}), ("categorical:5", {}), ("normal_meanscale:2", {}),
    ("bernoulli_probit/linear", {"rules": "mixed"}), ("categorical:3/mix", {"rules": "mixed"}),
]
IDS = [k + ("+" + "+".join(f"{a}={b}" for a, b in kw.items()) if kw else "") for k, kw in SCHEDULES]


@pytest.mark.parametrize("kind,kw", SCHEDULES, ids=IDS)
def test_moving_inputs_leave_no_trace_on_the_oracle(oracle, kind, kw):
    c = make_history_case(kind, **kw)
    full = check_schedule(c, moving_inputs(c), oracle, CUTS)
    if c["family"] != "normal":
        # offset None and an all-zero offset are the same inputs: exchanging the two steps changes nothing
        assert_same_run(run_schedule(c, moving_inputs(c, swap=True), oracle), full, f"{kind}: None <-> zeros")
        # ... and the offsets do matter: the chain without them is another chain
        still = run_schedule(c, lambda it: {"lik": moving_inputs(c)(it)["lik"]}, oracle)
        assert still["steps"][-1]["sum_trees"] != full["steps"][-1]["sum_trees"]


# ------------------------------------------------------------------ pgb_set_data again
def set_data_sequences(kind, n=1025):
    """{name: (case, [(X, rules, env) ...])}: the calls of each sequence in order; the LAST one is the data the chain
    runs on.  env: the value of PGB_X32_MIN_MB during the call (None: unset), which only the HIP library reads."""
    c = make_history_case(kind, n=n)
    X = c["X"].copy()
    X[:, 3] = np.random.default_rng(5).integers(0, 9, n)  # whole numbers: a continuous column or category codes
    c["X"] = X
    cont = np.zeros(5, np.int32)
    subset = np.array([0, 0, 0, 2, 0], np.int32)
    X2 = X.copy()
    X2[:, 0] = np.random.default_rng(6).uniform(-2, 2, n)
    X2[::7, 2] = np.nan
    bad = X.copy()
    bad[n // 2, 3] = 52.0  # one category code past PGB_SUBSET_BITS - 1
    return c, {
        "a_keys_then_subset": [(X, cont, "0"), (X, subset, "0")],
        "b_keys_then_no_keys": [(X, cont, "0"), (X, cont, None)],
        "c_keys_then_other_matrix": [(X, cont, "0"), (X2, cont, "0")],
        "d_refused_then_good": [(X, cont, None), (bad, subset, None), (X, subset, None)],
    }


SEQ_NAMES = ["a_keys_then_subset", "b_keys_then_no_keys", "c_keys_then_other_matrix", "d_refused_then_good"]


def _call(s, c, call, monkeypatch):
    X, rules, env = call
    if env is None:
        monkeypatch.delenv("PGB_X32_MIN_MB", raising=False)
    else:
        monkeypatch.setenv("PGB_X32_MIN_MB", env)
    return set_data_rc(s, X, rules, c["prior"])


def run_set_data_sequence(c, calls, backend, monkeypatch, cut=4):
    """The chain on a handle that saw the whole sequence before its first step, saw it AGAIN between the checkpoint
    before step `cut` and the restore of that image -- against the handle that was only ever given the last call's
    data.  Returns the latter's run."""
    sched = moving_inputs(c)
    half = c["steps"] // 2
    Xl, rl, envl = calls[-1]

    def fresh():
        if envl is None:
            monkeypatch.delenv("PGB_X32_MIN_MB", raising=False)
        else:
            monkeypatch.setenv("PGB_X32_MIN_MB", envl)
        return history_sampler(c, backend, {"X": Xl, "rules": rl, **{k: v for k, v in sched(0).items() if k == "response"}})

    ref = fresh()
    want = []
    for it in range(c["steps"]):
        apply_inputs(c, ref, sched(it))
        want.append(step_record(c, ref, it < half))
    want = dict(steps=want, end=end_record(ref))

    X0, r0, env0 = calls[0]
    if env0 is None:
        monkeypatch.delenv("PGB_X32_MIN_MB", raising=False)
    else:
        monkeypatch.setenv("PGB_X32_MIN_MB", env0)
    s = history_sampler(c, backend, {"X": X0, "rules": r0, **{k: v for k, v in sched(0).items() if k == "response"}})

    def replay(these):
        for call in these:
            rc, msg = _call(s, c, call, monkeypatch)
            refused = call[1][3] == 2 and np.nanmax(call[0][:, 3]) > 51
            assert (rc == PGB_E_INVALID and "SubsetSplit column 3" in msg) if refused else rc == _abi.PGB_OK, (rc, msg)

    replay(calls[1:])
    got = []
    for it in range(c["steps"]):
        if it == cut:
            blob = s.checkpoint()
            replay(calls)
            s.restore(blob)
        apply_inputs(c, s, sched(it))
        got.append(step_record(c, s, it < half))
    assert_same_run(dict(steps=got, end=end_record(s)), want, f"{c['name']}: set_data sequence against a fresh handle")
    return want


@pytest.mark.parametrize("seq", SEQ_NAMES)
@pytest.mark.parametrize("kind", ["normal", "categorical:3"])
def test_set_data_again_leaves_no_trace_on_the_oracle(oracle, monkeypatch, kind, seq):
    c, seqs = set_data_sequences(kind)
    run_set_data_sequence(c, seqs[seq], oracle, monkeypatch)


def refused_set_data_leaves_no_data(c, bad_call, backend, monkeypatch):
    """After a refused pgb_set_data with no good one following, every pgb_step* answers PGB_E_INVALID."""
    sched = moving_inputs(c)
    s = history_sampler(c, backend, {k: v for k, v in sched(0).items() if k == "response"})
    apply_inputs(c, s, sched(0))
    step_record(c, s, True)  # a handle that has data and has stepped
    rc, msg = _call(s, c, bad_call, monkeypatch)
    assert rc == PGB_E_INVALID and "SubsetSplit column 3" in msg
    lib = s.backend.lib.lib
    K, n = c["K"], c["X"].shape[0]
    host = np.zeros(K * n)
    dev = s.backend.mem.empty((K * n,), np.float64)
    vi = np.zeros(5, np.int32)
    ctr = _abi.Counters()
    for what, call in (("pgb_step", lambda: lib.pgb_step(s._h, 1, s.backend.mem.ptr(dev), vi.ctypes.data, C.byref(ctr))),
                       ("pgb_step_host", lambda: lib.pgb_step_host(s._h, 1, host.ctypes.data, vi.ctypes.data, C.byref(ctr))),
                       ("pgb_step_async", lambda: lib.pgb_step_async(s._h, 1, 2))):
        rc = call()
        assert rc == PGB_E_INVALID, (what, rc)
        assert "set_data" in lib.pgb_last_error().decode(), what
    return s


def test_a_refused_set_data_leaves_the_oracle_without_data(oracle, monkeypatch):
    c, seqs = set_data_sequences("normal")
    refused_set_data_leaves_no_data(c, seqs["d_refused_then_good"][1], oracle, monkeypatch)


def padded_matrix_chain(c, backend, ldx_pad):
    """The chain of `c` with X handed over as the first p columns of a wider row-major matrix (ldx = p + ldx_pad; the
    pad columns hold NaN and 1e300: a loader that read them would see missing values and a huge range)."""
    sched = moving_inputs(c)
    half = c["steps"] // 2
    s = history_sampler(c, backend, {k: v for k, v in sched(0).items() if k == "response"})
    if ldx_pad:
        n, p = c["X"].shape
        wide = np.full((n, p + ldx_pad), np.nan)
        wide[:, p + 1::2] = 1e300
        wide[:, :p] = c["X"]
        lib, mem = s.backend.lib, s.backend.mem
        xd = mem.from_host(wide)
        lib.check(lib.lib.pgb_set_data(s._h, mem.ptr(xd), p + ldx_pad, np.ascontiguousarray(c["rules"], np.int32).ctypes.data,
                                       np.ascontiguousarray(c["prior"], np.float64).ctypes.data), "pgb_set_data")
    out = []
    for it in range(c["steps"]):
        apply_inputs(c, s, sched(it))
        out.append(step_record(c, s, it < half))
    return dict(steps=out, end=end_record(s))


@pytest.mark.parametrize("kind,kw", [("normal", {}), ("bernoulli_probit/linear", {"rules": "mixed"})], ids=["normal", "probit-linear-mixed"])
def test_a_padded_matrix_is_the_same_data_on_the_oracle(oracle, kind, kw):
    """ldx = p + 3: X[:, 1] has missing values (col_nan), the pad columns must not be read."""
    c = make_history_case(kind, **kw)
    assert np.isnan(c["X"][:, 1]).any()
    assert_same_run(padded_matrix_chain(c, oracle, 3), padded_matrix_chain(c, oracle, 0), f"{kind}: ldx = p + 3")
