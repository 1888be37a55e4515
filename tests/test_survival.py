"""Discrete-time survival curves, the parts that need no GPU: the header ``include/pgbart_surv.h`` against NumPy's
sequential ``accumulate`` bit for bit, its accuracy against SciPy, its edges, ``person_period``, and the Python layer on
a backend made of the host references (``_surv_host.HostBackend``) -- its blocking, its chunking, the composition the
test assembles itself, the exact pool against plain predictions of the expanded matrix, its refusals."""
import json
import os

import numpy as np
import pytest
from scipy.special import expit, ndtr

import _arms_host as arms_host
import _ice_host as ice_host
import _permimp_host as permimp
import _predict_exact as ex
import _rowreduce_host as rr
import _rowsummary_host as rs
import _surv_host as host
from pymc_bart_amd import BARTOp, BernoulliLikelihood, person_period, survival_curves, survival_matrix
from pymc_bart_amd import decision as dec
from pymc_bart_amd import survival as surv
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 7.0e77
PER_ROW = tuple(a + b for a in ("surv", "rmst") for b in ("_mean", "_sd", "_quantiles", "_hdi")) + ("time_quantiles",)
PER_DRAW = tuple(a + b for a in ("surv_avg", "rmst_avg") for b in ("", "_mean", "_sd", "_hdi"))
OTHER = ("group_weight", "n_list_trees", "times")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same(got, want, keys=PER_ROW + PER_DRAW + OTHER):
    for key in keys:
        assert np.array_equal(bits(got[key]), bits(want[key])), (key, got[key], want[key])
    assert got["n_nonfinite"] == want["n_nonfinite"] and got["beyond"] == want["beyond"]


# ------------------------------------------------------------------ 1. the header against NumPy, bit for bit
def test_the_constants_of_the_header_are_the_modules():
    L = host.lib()
    assert L.surv_max_levels() == surv.MAX_LEVELS == 4 and L.surv_max_times() == dec.MAX_ARMS == 64


def _padded(rng, A, D, nb, scale=1.5):
    """Predictions ``(A, D, nb)`` as a view of a wider poisoned buffer: ldd = nb + 3, lda = (D + 1) ldd."""
    wide = np.full((A, D + 1, nb + 3), POISON)
    f = wide[:, :D, :nb]
    f[...] = rng.normal(0, scale, (A, D, nb))
    return wide, f


@pytest.mark.parametrize("link", ["probit", "logistic"])
@pytest.mark.parametrize("A,D,nb", [(1, 1, 1), (2, 3, 130), (7, 1, 130), (64, 3, 1), (7, 3, 130), (64, 1, 130)])
def test_the_header_equals_numpys_sequential_accumulate_bit_for_bit(link, A, D, nb):
    rng = np.random.default_rng(1000 + A + D + nb)
    t, dt, beyond = host.grid(A, origin=-0.5, rng=rng)
    u = [1.0, 0.75, 0.5, 0.05]
    for off in (None, rng.normal(0, 0.4, nb)):
        wide, f = _padded(rng, A, D, nb, scale=0.8 if A == 64 else 1.5)
        want_S, want_R, want_T = host.numpy_curves(f.copy(), t, dt, u, beyond, link, off)
        state, count = host.block(f, t, dt, u, beyond, link, off)
        assert count == 0 and np.array_equal(bits(f), bits(want_S)) and np.array_equal(bits(state[0]), bits(want_S[-1]))
        assert np.array_equal(bits(state[1]), bits(want_R)) and np.array_equal(bits(state[2:]), bits(want_T))
        assert np.all(wide[:, D] == POISON) and np.all(wide[:, :, nb:] == POISON)         # only the cells of f are written
        assert np.all(state[2] == t[0])                                                    # S_0 <= 1.0 always
        if A >= 7 and nb > 1:
            assert len(np.unique(state[2:])) > 3 and (A > 7 or np.any(state[2:] == beyond))


def test_seven_times_in_chunks_of_one_two_and_four_equal_one_call():
    rng = np.random.default_rng(7)
    D, nb = 3, 130
    t, dt, beyond = host.grid(7, rng=rng)
    u, off = [0.9, 0.3], rng.normal(0, 0.3, nb)
    for link in ("probit", "logistic"):
        f = rng.normal(0.3, 1.2, (7, D, nb))
        f[2, 1, 5] = np.nan if link == "logistic" else np.inf
        whole = f.copy()
        state, count = host.block(whole, t, dt, u, beyond, link, off)
        cut, st, cnt = f.copy(), None, 0
        for c0, c1 in ((0, 1), (1, 3), (3, 7)):
            st, cnt = host.block(cut[c0:c1], t[c0:c1], dt[c0:c1], u, beyond, link, off, state=st, count=cnt)
        assert np.array_equal(whole, cut, equal_nan=True) and np.array_equal(state, st, equal_nan=True) and cnt == count
        assert count == (1 if link == "logistic" else 0)


# ------------------------------------------------------------------ 2. accuracy
@pytest.mark.parametrize("link", ["probit", "logistic"])
def test_the_curve_against_scipy_within_the_bound_of_its_factors(link):
    """``S_j`` against ``np.cumprod`` of SciPy's ``ndtr(-s)`` / ``expit(-s)`` with ``s`` in [-30, 30], within the relative
    ``J (8 rho + 2^-52)``: ``rho`` is the link's ``max_rel_diff`` of ``profiles/rowsummary_accuracy.json`` (the header's
    function against the same SciPy functions over the same range) -- every factor is off by at most ``rho`` and every
    product rounds once, on either side.  A relative bound speaks of normal numbers: entries whose reference lies
    below 1e-290 (products of several factors near ``Phi(-30)`` = 5e-198) are compared as absolute values against the
    bound times 1e-290.  Nothing is tuned on the code under test."""
    rho = json.load(open(os.path.join(ROOT, "profiles", "rowsummary_accuracy.json")))["max_rel_diff"][link]
    ref = ndtr if link == "probit" else expit
    rng = np.random.default_rng(5)
    cases = [np.linspace(-30.0, 30.0, 4001)[None, None, :]]                                # J = 1: every factor alone
    cases += [rng.uniform(-30.0, 30.0, (7, 2, 500)), rng.uniform(-30.0, 2.0, (64, 2, 200)), rng.uniform(-3.0, 0.0, (64, 1, 200))]
    for s in cases:
        J = s.shape[0]
        t, dt, beyond = host.grid(J)
        got = s.copy()
        host.block(got, t, dt, [], beyond, link)
        want = np.cumprod(ref(-s), axis=0)
        bound = J * (8.0 * rho + 2.0 ** -52)
        err = np.abs(got - want) / np.maximum(np.abs(want), 1e-290)
        print(f"{link} J={J}: max relative error {err.max():.3e}, bound {bound:.3e}; {int((want >= 1e-290).sum())} of {want.size} normal")
        assert err.max() <= bound, (J, err.max(), bound)
        assert (want >= 1e-290).mean() > 0.15


# ------------------------------------------------------------------ 3. edges
@pytest.mark.parametrize("link", ["probit", "logistic"])
def test_predictions_at_minus_and_plus_forty_and_a_curve_that_never_rises(link):
    rng = np.random.default_rng(31)
    assert host.link_q(-40.0, link) == 1.0
    t, dt, beyond = host.grid(6)
    f = rng.normal(0, 1, (6, 2, 70))
    f[2], f[4, 1] = -40.0, 40.0
    S = f.copy()
    state, count = host.block(S, t, dt, [0.5, 1e-15], beyond, link)
    assert count == 0 and np.array_equal(bits(S[2]), bits(S[1]))                          # q == 1.0: S is unchanged
    assert np.all(S[4, 1] < 1e-17) and np.all(S[5, 1] <= S[4, 1]) and np.all(S[4, 0] > 1e-6)   # the collapse, and it stays
    assert np.all(np.diff(np.concatenate([np.ones((1, 2, 70)), S]), axis=0) <= 0.0)       # non-increasing from 1.0
    assert np.all(state[3, 1] == np.where(S[3, 1] <= 1e-15, t[3], t[4])) and np.all(state[3, 0] == beyond)
    big = rng.uniform(-30, 30, (64, 3, 130))
    host.block(big, *host.grid(64)[:2], [], 65.0, link)
    assert np.all(np.diff(big, axis=0) <= 0.0) and np.all(big >= 0.0) and np.all(big[0] <= 1.0)


def test_a_nan_propagates_reaches_no_level_and_is_counted():
    """Under the logistic link a NaN prediction is a NaN factor: it is counted once, every later S of that (draw, row) is
    a NaN, and a NaN S reaches no level.  Under the probit link the predictor must not be a NaN (``pgb_lphi_t`` reads the
    clamp row of the NaN's sign bit, which compilers do not agree on: the factor is 0.0 or 1.0, never a NaN, and nothing
    is counted) -- but a NaN S that arrives with the stored state propagates and reaches no level under either link."""
    t, dt, beyond = host.grid(5)
    f = np.full((5, 2, 3), 1.0)
    f[2, 1, 0] = np.nan
    S = f.copy()
    state, count = host.block(S, t, dt, [1.0, 0.05, 0.002], beyond, "logistic")
    assert count == 1 and np.all(np.isnan(S[2:, 1, 0])) and not np.any(np.isnan(S[:2])) and np.isnan(state[0, 1, 0])
    assert np.isnan(S).sum() == 3 and np.isnan(state[1:]).sum() == 1                       # R took one NaN term; T is never NaN
    assert state[2:, 1, 0].tolist() == [1.0, beyond, beyond]                              # 0.269, 0.072, NaN, ..: 0.05 was not reached
    assert state[2:, 0, 0].tolist() == [1.0, 3.0, 5.0]                                     # .., 0.0195, 0.0052, 0.0014
    inf = np.full((2, 1, 1), np.inf)
    assert host.block(inf, t[:2], dt[:2], [0.5], beyond, "logistic")[1] == 2              # 1 / (1 + exp(inf)): the link's own NaN
    S = f.copy()
    state, count = host.block(S, t, dt, [0.01], beyond, "probit")                          # 0.159, 0.025, then 0.0
    assert count == 0 and not np.any(np.isnan(S)) and (np.all(S[2:, 1, 0] == 0.0) or np.all(S[2:, 1, 0] == S[1, 1, 0]))
    inf = np.stack([np.full((1, 1), np.inf), np.full((1, 1), -np.inf)])[::-1].copy()    # -inf, then +inf: the limits 1.0 and 0.0
    assert host.block(inf, t[:2], dt[:2], [0.5], beyond, "probit")[1] == 0 and inf.ravel().tolist() == [1.0, 0.0]
    for link in ("probit", "logistic"):
        start = np.stack([np.full((2, 3), np.nan), np.zeros((2, 3)), np.full((2, 3), beyond)])
        S = np.zeros((5, 2, 3))
        state, count = host.block(S, t, dt, [1.0], beyond, link, state=start)
        assert count == 0 and np.all(np.isnan(S)) and np.all(state[2] == beyond) and np.all(np.isnan(state[:2]))


def test_levels_at_the_first_time_at_the_last_time_and_never_and_monotone_in_u():
    rng = np.random.default_rng(33)
    t, dt, beyond = host.grid(6, origin=0.5, rng=rng)
    f = np.full((6, 1, 4), -40.0)                                                          # q == 1.0 everywhere ...
    f[0, 0, 0] = 0.0                                                                       # ... row 0 halves at the first time
    f[5, 0, 1] = 0.0                                                                       # ... row 1 at the last; rows 2, 3 never
    for link in ("probit", "logistic"):
        S = f.copy()
        state, _ = host.block(S, t, dt, [0.5], beyond, link)
        assert state[2, 0].tolist() == [t[0], t[5], beyond, beyond] and S[5, 0].tolist() == [0.5, 0.5, 1.0, 1.0]
        assert state[1, 0, 2] == np.add.accumulate(dt)[-1] and state[1, 0, 0] == np.add.accumulate(np.concatenate([dt[:1], 0.5 * dt[1:]]))[-1]
        u = [1.0, 0.8, 0.5, 0.2]
        S = rng.normal(-0.5, 1.0, (6, 3, 130))
        state, _ = host.block(S, t, dt, u, beyond, link)
        T = state[2:]
        assert np.all(np.diff(T, axis=0) >= 0.0) and np.all(T[0] == t[0]) and np.any(T[3] == beyond) and np.any(T[3] < beyond)
        assert np.all(np.isin(T, np.concatenate([t, [beyond]])))


# ------------------------------------------------------------------ 4. person_period
def test_person_period_on_a_hand_example_and_its_refusals():
    X = np.array([[10.0, 0.5], [20.0, 1.5], [30.0, 2.5]])
    got = person_period([2.0, 1.0, 3.0], [True, False, True], X)                         # subject 1 is censored at 1
    assert got["times"].tolist() == [1.0, 2.0, 3.0] and got["subject"].tolist() == [0, 0, 1, 2, 2, 2]
    assert got["y"].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    assert got["X"].tolist() == [[1.0, 10.0, 0.5], [2.0, 10.0, 0.5], [1.0, 20.0, 1.5], [1.0, 30.0, 2.5], [2.0, 30.0, 2.5], [3.0, 30.0, 2.5]]
    wide = person_period([2.0, 1.0, 3.0], [1, 0, 0], times=[0.5, 1.0, 2.0, 3.0, 4.0])   # a grid of one's own, no covariates
    assert wide["X"].shape == (9, 1) and wide["X"][:, 0].tolist() == [0.5, 1.0, 2.0, 0.5, 1.0, 0.5, 1.0, 2.0, 3.0]
    assert wide["y"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0] and wide["y"].dtype == np.float64
    assert person_period([5.0], [1], [7.0])["X"].tolist() == [[5.0, 7.0]]
    cases = [
        (dict(time=[1.0, np.nan, 2.0]), "time must be finite"), (dict(time=[]), "time must be a non-empty vector"),
        (dict(time=[[1.0, 2.0, 3.0]]), "time must be a non-empty vector"), (dict(event=[1, 0]), "event must hold one value per subject"),
        (dict(event=[1, 2, 0]), "event must hold booleans"), (dict(event=["a", "b", "c"]), "event must hold booleans"),
        (dict(X=np.zeros((2, 2))), r"X must hold one row per subject: shape \(3, p\)"),
        (dict(times=[1.0, 2.0]), r"time\[2\] = 3.0 is not on the grid of times"), (dict(times=[1.0, 2.5, 3.0]), r"time\[0\] = 2.0 is not on the grid"),
        (dict(times=[1.0, 3.0, 2.0]), "times must be finite and strictly increasing"), (dict(times=[1.0, 2.0, np.inf]), "times must be finite"),
        (dict(times=[]), "times must be a non-empty vector"),
    ]
    for change, msg in cases:
        with pytest.raises(ValueError, match=msg):
            person_period(**dict(dict(time=[2.0, 1.0, 3.0], event=[1, 0, 1], X=X), **change))


# ------------------------------------------------------------------ 5. the Python layer on the host backend
def _sampler(oracle, pool, table):
    table = np.ascontiguousarray(table, np.int32)
    be = host.HostBackend(oracle, pool)
    return be, PosteriorSampler(pool, table, table.shape[1], pool.n_outputs, backend=be)


@pytest.fixture(scope="module")
def small(oracle):
    """A hand-built pool: three draws of one output, the time in column 2, missing values in the rows."""
    rng = np.random.default_rng(41)
    pool = ice_host.random_pool(rng, 14, 4, depth=4, linear=[1])
    be = host.HostBackend(oracle, pool)
    s = ice_host.pool_sampler(rng, pool, 6, 3, be)
    X = rng.normal(size=(150, 4))
    X[rng.random((150, 4)) < 0.04] = np.nan
    kw = dict(times=np.cumsum(rng.uniform(0.2, 0.6, 7)) - 1.0, time_col=2, link="logistic", offset=rng.normal(-1.0, 0.3, 150),
              origin=-1.5, levels=(0.9, 0.5), weights=rng.uniform(0.5, 2.0, 150))
    return be, s, pool, X, kw


@pytest.fixture(scope="module")
def chain(oracle):
    """A short chain of the oracle on person-period rows (probit): 60 subjects, 2 covariates, 4 times, m = 5, three draws
    (the partial sums of 5 x 3 draws x 2 groups and a block of 64 rows fit the floor of ``PGB_PW_BLOCK_BYTES``)."""
    rng = np.random.default_rng(42)
    Z = rng.normal(size=(60, 2))
    time = rng.integers(1, 5, 60).astype(np.float64)
    pp = person_period(time, rng.random(60) < 0.7, Z)
    op = BARTOp(pp["X"], pp["y"], m=5)
    attach_history(op, [sample_chain(op, 6, 3, num_particles=5, random_seed=3, backend=oracle, keep_draws=False,
                                     likelihood=BernoulliLikelihood("probit"))])
    s = _get_posterior_sampler(op, backend=oracle)
    pool, table = (s.pooled_history() if hasattr(s, "pooled_history") else (s.pool, s.forest_idx))
    pool = pool.decoded() if hasattr(pool, "decoded") else pool
    be, s = _sampler(oracle, pool, np.asarray(table))
    X = np.column_stack([np.zeros(60), Z])
    return be, s, pool, X, dict(times=pp["times"], levels=(0.75, 0.5), groups=np.where(Z[:, 0] > 0, "b", "a"))


@pytest.mark.parametrize("which", ["small", "chain"])
def test_blocks_of_64_rows_and_time_chunks_of_1_and_4_change_no_bit(which, request, monkeypatch):
    be, s, pool, X, kw = request.getfixturevalue(which)
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    monkeypatch.delenv("PGB_SURV_TIME_CHUNK", raising=False)
    n, J = X.shape[0], len(kw["times"])
    del be.calls[:], be.surv_calls[:]
    whole = survival_curves(s, X, **kw)
    matrix = survival_matrix(s, X, **{k: v for k, v in kw.items() if k not in ("levels", "weights", "groups")})
    assert be.calls == [n, n] and be.surv_calls == [(n, J, 1)] * 2 and matrix.shape == (s.forest_idx.shape[0], n, J)
    assert np.array_equal(bits(whole["surv_mean"][:, -1]), bits(rs.summary(matrix[:, :, -1])[0]))
    assert np.all(np.diff(matrix, axis=2) <= 0.0) and np.all(whole["rmst_mean"] > 0.0) and whole["n_nonfinite"] == 0
    assert whole["time_quantiles"].shape == (3, n, 2) and whole["surv_quantiles"].shape == (3, n, J) and whole["surv_hdi"].shape == (2, n, J)
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")                  # blocks of 64 rows
    del be.calls[:], be.surv_calls[:]
    blocked = survival_curves(s, X, **kw)
    assert len(be.calls) == -(-n // 64) and all(nb == 64 for nb in be.calls[:-1]) and sum(be.calls) == n
    same(blocked, whole)
    assert np.array_equal(bits(survival_matrix(s, X, **{k: v for k, v in kw.items() if k not in ("levels", "weights", "groups")})), bits(matrix))
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    for chunk in (1, 4):
        monkeypatch.setenv("PGB_SURV_TIME_CHUNK", str(chunk))
        del be.surv_calls[:]
        same(survival_curves(s, X, **kw), whole)
        want = [(n, min(chunk, J - c0), int(c0 == 0)) for c0 in range(0, J, chunk)]
        assert be.surv_calls == want
        assert np.array_equal(bits(survival_matrix(s, X, **{k: v for k, v in kw.items() if k not in ("levels", "weights", "groups")})), bits(matrix))
    monkeypatch.setenv("PGB_SURV_TIME_CHUNK", "4")
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")
    same(survival_curves(s, X, **kw), whole)


@pytest.mark.parametrize("which", ["small", "chain"])
def test_the_call_equals_the_composition_of_the_references(which, request, oracle, monkeypatch):
    """``_arms_host.reference_block`` with the times as the arms, the header on its output, then the host builds of the
    row summary (over the draws) and of the row reduce (over the rows) per slab."""
    be, s, pool, X, kw = request.getfixturevalue(which)
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    monkeypatch.delenv("PGB_SURV_TIME_CHUNK", raising=False)
    got = survival_curves(s, X, quantiles=(0.1, 0.5), hdi_prob=0.8, **kw)
    table = np.asarray(s.forest_idx, np.int32)
    D, n = table.shape[0], X.shape[0]
    t = np.asarray(kw["times"], np.float64)
    dt = np.diff(np.concatenate([[kw.get("origin", 0.0)], t]))
    beyond = float(t[-1] + dt[-1])
    out, lens = arms_host.reference_block(oracle, pool, table, X, [kw.get("time_col", 0)], t[:, None], np.arange(D))
    S = np.ascontiguousarray(out[:, :, 0])                                                # (J, D, n)
    state, count = host.block(S, t, dt, kw["levels"], beyond, kw.get("link", "probit"), kw.get("offset"))
    w = np.ones(n) if kw.get("weights") is None else kw["weights"]
    labels, gid = (np.zeros(1), np.zeros(n, np.int64)) if kw.get("groups") is None else np.unique(kw["groups"], return_inverse=True)
    G, q, k = labels.size, np.array([0.1, 0.5]), rs.hdi_k(D, 0.8)
    assert got["beyond"] == beyond and got["n_nonfinite"] == count and got["n_list_trees"].tolist() == lens.tolist() and lens.max() > 0
    assert got["group_labels"].tolist() == labels.tolist() and got["n_draws"] == D
    for j in range(t.size):
        st = rs.summary(S[j], q, k)
        for key, want in (("surv_mean", st[0]), ("surv_sd", np.sqrt(st[1])), ("surv_quantiles", st[2:4]), ("surv_hdi", st[4:6])):
            assert np.array_equal(bits(got[key][..., j]), bits(want)), (key, j)
        red = rr.reduce(S[j][:, None, :], w, gid, G)
        assert np.array_equal(bits(got["surv_avg"][:, :, j]), bits(red["out"][0][:, 0])), j
        assert np.array_equal(bits(got["group_weight"]), bits(red["W"]))
    st = rs.summary(state[1], q, k)
    for key, want in (("rmst_mean", st[0]), ("rmst_sd", np.sqrt(st[1])), ("rmst_quantiles", st[2:4]), ("rmst_hdi", st[4:6])):
        assert np.array_equal(bits(got[key]), bits(want)), key
    assert np.array_equal(bits(got["rmst_avg"]), bits(rr.reduce(state[1][:, None, :], w, gid, G)["out"][0][:, 0]))
    for l in range(len(kw["levels"])):
        assert np.array_equal(bits(got["time_quantiles"][:, :, l]), bits(rs.summary(state[2 + l], q, 0)[2:4]))
    for key in ("surv_avg", "rmst_avg"):
        assert np.array_equal(bits(got[key + "_mean"]), bits(got[key].mean(axis=0))) and got[key + "_hdi"].shape == got[key].shape[1:] + (2,)
    assert got["surv_avg"].shape == (D, G, t.size) and got["rmst_avg"].shape == (D, G)
    few = survival_curves(s, X, draws=[2, 0], **kw)                                       # the per-draw results are paired
    for key in ("surv_avg", "rmst_avg"):
        assert np.array_equal(bits(few[key]), bits(survival_curves(s, X, **kw)[key][[2, 0]])), key
    one = survival_curves(s, X, draws=[1], **kw)                                          # one draw: no summary over the draws
    assert "surv_mean" not in one and "time_quantiles" not in one and np.array_equal(bits(one["rmst_avg"]), bits(got["rmst_avg"][[1]]))


def _exact_tree(rng, K, depth, cols, level=0):
    """Leaf values that are multiples of 2^-10 within +-0.5; continuous splits."""
    if level >= depth or (level > 0 and rng.random() > 0.8):
        return ex.Leaf(ex.dyadic(rng, 10, 0.5, K))
    j = int(rng.choice(cols))
    return ex.Split(j, float(rng.normal(0, 0.7)), _exact_tree(rng, K, depth, cols, level + 1), _exact_tree(rng, K, depth, cols, level + 1))


@pytest.mark.parametrize("link", ["probit", "logistic"])
def test_the_exact_pool_equals_the_header_on_plain_predictions_of_the_expanded_matrix(oracle, link, monkeypatch):
    """Every leaf is a multiple of 2^-10, so every sum of leaves is exact and ``f + (A_a - A_self)`` IS the prediction at
    the copy: ``survival_matrix`` must equal, in bits, the header applied to the oracle's ``pgb_predict`` on the n J rows
    a user would build by hand."""
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    monkeypatch.setenv("PGB_SURV_TIME_CHUNK", "3")
    rng = np.random.default_rng(51)
    K, p, n, J = 2, 5, 90, 8
    pool = ex.build_pool([_exact_tree(rng, K, 4, [0, 1, 3, 3]) for _ in range(20)], K)
    table = np.stack([rng.choice(20, size=8, replace=False) for _ in range(5)]).astype(np.int32)
    be, s = _sampler(oracle, pool, table)
    X = rng.normal(size=(n, p))
    times = np.sort(rng.normal(0, 1.0, J))
    off = ex.dyadic(rng, 6, 1.0, n)
    expanded = np.repeat(X, J, axis=0)
    expanded[:, 3] = np.tile(times, n)
    plain = permimp.predict(oracle, pool, table, expanded).reshape(5, K, n, J)          # what sample_posterior returns
    dt = np.diff(np.concatenate([[times[0] - 1.0], times]))
    for output in (0, 1):
        want = np.ascontiguousarray(np.moveaxis(plain[:, output], 2, 0))                  # (J, D, n)
        state, _ = host.block(want, times, dt, [0.5], float(times[-1] + dt[-1]), link, off)
        got = survival_matrix(s, X, times, time_col=3, output=output, link=link, offset=off, origin=times[0] - 1.0)
        assert got.shape == (5, n, J) and np.array_equal(bits(got), bits(np.moveaxis(want, 0, 2)))
        res = survival_curves(s, X, times, time_col=3, output=output, link=link, offset=off, origin=times[0] - 1.0)
        assert np.array_equal(bits(res["rmst_mean"]), bits(rs.summary(state[1])[0]))
        assert np.array_equal(bits(res["time_quantiles"][1, :, 0]), bits(rs.summary(state[2], [0.5])[2]))
    assert len(np.unique(got[:, :, -1])) > 50 and 0.0 < got.min() and got.max() < 1.0


def test_every_refusal_of_the_python_layer(small, monkeypatch):
    be, s, pool, X, kw = small
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    monkeypatch.delenv("PGB_SURV_TIME_CHUNK", raising=False)
    del be.calls[:], be.surv_calls[:]
    n = X.shape[0]
    zero_group = kw["weights"].copy()
    zero_group[:75] = 0.0
    cases = [
        (dict(time_col=4), r"time_col must be an integer in \[0, 4\)"), (dict(time_col=-1), "time_col must be an integer"),
        (dict(time_col=1.0), "time_col must be an integer"), (dict(times=[]), "times must be a non-empty vector"),
        (dict(times=[[1.0, 2.0]]), "times must be a non-empty vector"), (dict(times=[0.0, 1.0, 1.0]), "times must be finite and strictly increasing"),
        (dict(times=[0.0, np.nan]), "times must be finite and strictly increasing"), (dict(times=["a"]), "times must be a vector of numbers"),
        (dict(times=np.arange(4097.0)), "at most 4096 times per call, got 4097"),
        (dict(origin=kw["times"][0]), r"origin must be finite and < times\[0\]"), (dict(origin=np.nan), "origin must be finite"),
        (dict(times=[0.0, 1e308], origin=-1e308), "the widths of the grid"),
        (dict(output=1), r"output must be an integer in \[0, 1\)"), (dict(output=0.0), "output must be an integer"),
        (dict(link="identity"), "unknown link 'identity': use one of probit, logistic"), (dict(link="logit"), "unknown link 'logit'"),
        (dict(offset=np.zeros(n - 1)), "offset must hold one value per row"), (dict(offset=np.full(n, np.inf)), "offset must be finite"),
        (dict(draws=[3]), "draws must index the 3 stored draws"), (dict(draws=[]), "a survival curve needs at least 1 draw"),
        (dict(quantiles=[0.5, 1.5]), r"quantiles must be in \[0, 1\]"), (dict(quantiles=np.linspace(0, 1, 17)), "at most 16 quantiles"),
        (dict(hdi_prob=1.0), "hdi_prob must lie in"), (dict(hdi_prob=0.0), "hdi_prob must be in"),
        (dict(levels=[0.5, 0.4, 0.3, 0.2, 0.1]), "levels must be a vector of at most 4 survival levels"),
        (dict(levels=[[0.5]]), "levels must be a vector of at most 4"), (dict(levels=[0.0]), r"levels must lie in \(0, 1\]"),
        (dict(levels=[1.5]), "levels must lie in"), (dict(levels=[np.nan]), "levels must lie in"),
        (dict(weights=np.ones(n - 1)), "weights must hold one value per row"), (dict(weights=-np.ones(n)), "weights must be finite and >= 0"),
        (dict(weights=zero_group, groups=np.arange(n) // 75), "group 0 has total weight 0"),
        (dict(groups=np.zeros(n + 1)), "groups must hold one label per row"),
    ]
    for change, msg in cases:
        with pytest.raises(ValueError, match=msg):
            survival_curves(s, X, **dict(kw, **change))
    with pytest.raises(ValueError, match="X must be a matrix"):
        survival_matrix(s, np.zeros((3, 2, 2)), [1.0])
    with pytest.raises(ValueError, match="unknown link"):
        survival_matrix(s, X, [1.0], link="cloglog")
    with pytest.raises(TypeError):
        survival_curves(s, X, [1.0], 2)                                                    # (keyword-only beyond the grid)
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", "65536")
    with pytest.raises(ValueError, match=r"the partial sums of 7 times \+ 1 x 3 draws x 150 groups take \d+ bytes and a block of 64 rows \d+, "
                                         r"more than a block may take \(65536, PGB_PW_BLOCK_BYTES\)"):
        survival_curves(s, X, **dict(kw, groups=np.arange(n)))
    assert be.calls == [] and be.surv_calls == []
    assert survival_curves(s, X, **dict(kw, levels=()))["time_quantiles"].shape == (3, n, 0)   # no level is legal


def test_the_time_chunk_knob(monkeypatch):
    for text, want in (("1", 1), ("0", 1), ("-5", 1), ("17", 17), ("64", 64), ("1000", 64)):
        monkeypatch.setenv("PGB_SURV_TIME_CHUNK", text)
        assert surv.time_chunk() == want
    monkeypatch.delenv("PGB_SURV_TIME_CHUNK")
    assert surv.time_chunk() == 64


def test_the_cpu_oracle_is_refused_naming_the_entry_point(oracle, small):
    be, s, pool, X, kw = small
    with pytest.raises(NotImplementedError, match="pgb_surv_curves"):
        survival_curves(s, X, backend=oracle, **kw)
    with pytest.raises(NotImplementedError, match="pgb_surv_curves"):
        survival_matrix(s, X, [1.0], backend=oracle)
    with pytest.raises(NotImplementedError, match="pgb_surv_kernel_ms"):
        oracle.lib.surv_kernel_ms()


# ------------------------------------------------------------------ 6. the budget and the timing tool
def test_the_instances_are_in_the_occupancy_budget_with_no_scratch():
    budget = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    for Q in range(5):
        name = f"k_surv<{Q}>"
        assert budget[name]["max_scratch_bytes"] == 0 and budget[name]["max_vgpr_spills"] == 0, name


def test_the_timing_tool_answers_help():
    import subprocess
    import sys

    tool = os.path.join(ROOT, "tools", "timing_survival.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--baseline-root" in r.stdout
