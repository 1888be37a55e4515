"""Discrete-time survival curves on the MI355X: ``pgb_surv_curves`` (``k_surv``) against the host build of
``include/pgbart_surv.h`` (``tests/_surv_host.py``) bit for bit, with guards behind every buffer, over the row counts,
grid sizes, draws, levels, links and strides at which the kernel takes another path; the carry of the state from call to
call; the edge values; every refusal; then ``survival_curves`` and ``survival_matrix`` end to end on a two-chain probit
fit on person-period rows.

Everything is ``np.array_equal`` on the bits; a NaN on both sides counts as equal (the sign and payload of a NaN an
operation GENERATES are the hardware's, not the contract's: ``tests/test_rowreduce_gpu.py``)."""
import numpy as np
import pytest

import _surv_host as host
from pymc_bart_amd import BARTOp, BernoulliLikelihood, person_period, survival_curves, survival_matrix
from pymc_bart_amd import survival as surv
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler

pytestmark = pytest.mark.gpu

GUARD = -7.75e300    # behind every buffer, and in the state before a call: no refused call may touch it
INT_GUARD = -77
E_INVALID = -1
PER_ROW = tuple(a + b for a in ("surv", "rmst") for b in ("_mean", "_sd", "_quantiles", "_hdi")) + ("time_quantiles",)
PER_DRAW = tuple(a + b for a in ("surv_avg", "rmst_avg") for b in ("", "_mean", "_sd", "_hdi"))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_bits(got, want) -> bool:
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


# ------------------------------------------------------------------ pgb_surv_curves
def _curves(hip, f, k, t, dt, u, beyond, link, off=None, state=None, count=0, pad=0, change=None):
    """The entry point on output ``k`` of ``f`` ``(A, D, K, nb)``, handed over through ``lda`` / ``ldd`` without a copy
    (``pad``: extra doubles between the arms).  ``state``: ``None`` starts it (over a buffer full of ``GUARD``),
    otherwise the call continues from it.  ``change``: arguments replaced after everything is laid out.  ->
    ``(rc, f after the call, state (2 + Q, D, nb), the counter, guards untouched)``."""
    mem = hip.mem
    A, D, K, nb = f.shape
    lda = D * K * nb + pad
    wide = np.full((A, lda), GUARD)
    wide[:, :D * K * nb] = f.reshape(A, -1)
    fd = mem.from_host(np.concatenate([wide.ravel(), np.full(64, GUARD)]))
    t, dt, u = (np.ascontiguousarray(v, np.float64) for v in (t, dt, u))
    Q = u.size
    cells = (2 + Q) * D * nb
    init = state is None
    sd = mem.from_host(np.concatenate([np.full(cells, GUARD) if init else np.ascontiguousarray(state, np.float64).ravel(),
                                       np.full(64, GUARD)]))
    cd = mem.from_host(np.array([count, INT_GUARD, INT_GUARD], np.int64))
    offd = None if off is None else mem.from_host(np.concatenate([np.ascontiguousarray(off, np.float64), np.full(8, GUARD)]))
    a = dict(f=mem.ptr(fd[k * nb:]), lda=lda, ldd=K * nb, D=D, A=A, nb=nb, off=None if offd is None else mem.ptr(offd),
             transform=host.LINKS[link] if isinstance(link, str) else link, t=t.ctypes.data, dt=dt.ctypes.data,
             u=u.ctypes.data if Q else None, Q=Q, beyond=float(beyond), init=int(init), state=mem.ptr(sd), cnt=mem.ptr(cd))
    a.update(change or {})
    rc = hip.lib.surv_entry_points()(a["f"], a["lda"], a["ldd"], a["D"], a["A"], a["nb"], a["off"], a["transform"], a["t"], a["dt"],
                                     a["u"], a["Q"], a["beyond"], a["init"], a["state"], a["cnt"], mem.stream_ptr)
    got_f, got_s, got_c = mem.to_host(fd), mem.to_host(sd), mem.to_host(cd)
    body = got_f[:A * lda].reshape(A, lda)
    guards = bool(np.all(got_f[A * lda:] == GUARD) and np.all(body[:, D * K * nb:] == GUARD) and np.all(got_s[cells:] == GUARD)
                  and np.all(got_c[1:] == INT_GUARD))
    return rc, body[:, :D * K * nb].reshape(A, D, K, nb).copy(), got_s[:cells].reshape(2 + Q, D, nb).copy(), int(got_c[0]), guards


def _reference(f, k, t, dt, u, beyond, link, off=None, state=None, count=0):
    """The host header on the same cells: -> ``(f after, state, counter)``."""
    want = f.copy()
    st, cnt = host.block(want[:, :, k], t, dt, u, beyond, link, off, None if state is None else state.copy(), count)
    return want, st, cnt


def _check(hip, f, k, t, dt, u, beyond, link, off=None, pad=0):
    rc, got_f, got_s, got_c, guards = _curves(hip, f, k, t, dt, u, beyond, link, off, pad=pad)
    hip.lib.check(rc, "pgb_surv_curves")
    want_f, want_s, want_c = _reference(f, k, t, dt, u, beyond, link, off)
    assert guards and got_c == want_c, (got_c, want_c)
    assert same_bits(got_f, want_f), int((bits(got_f) != bits(want_f)).sum())             # the other outputs included: untouched
    assert same_bits(got_s, want_s), int((bits(got_s) != bits(want_s)).sum())
    return got_f, got_s, got_c


LEVELS = [1.0, 0.7, 0.4, 0.05]


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("A,D,Q,link", [(1, 1, 0, "probit"), (64, 3, 4, "logistic"), (2, 5, 1, "probit")])
def test_row_counts_grids_draws_levels_and_links_through_padded_strides(hip, nb, A, D, Q, link):
    """K = 3 with output 1: ldd = 3 nb, lda = 3 D nb (+ 5 in the padded call); the cells of outputs 0 and 2 and the
    padding must come back as they went in."""
    rng = np.random.default_rng(100 + nb + A + D)
    t, dt, beyond = host.grid(A, origin=-0.25, rng=rng)
    f = rng.normal(-0.8 if A == 64 else 0.0, 1.0, (A, D, 3, nb))
    for off, pad in ((None, 0), (rng.normal(0, 0.3, nb), 5)):
        got_f, got_s, _ = _check(hip, f, 1, t, dt, LEVELS[:Q], beyond, link, off, pad)
        assert np.array_equal(bits(got_f[:, :, [0, 2]]), bits(f[:, :, [0, 2]])) and np.all(got_f[:, :, 1] <= 1.0)
    if Q == 4 and nb >= 63:
        assert np.all(got_s[2] == t[0]) and len(np.unique(got_s[3:])) > 5


def test_two_calls_that_continue_the_state_equal_one(hip):
    rng = np.random.default_rng(200)
    A, D, K, nb = 7, 3, 2, 130
    t, dt, beyond = host.grid(A, rng=rng)
    f, off, u = rng.normal(0.2, 1.0, (A, D, K, nb)), rng.normal(0, 0.3, nb), [0.9, 0.3]
    for link in ("logistic", "probit"):
        # counted in either half under the logistic link; the probit link gives an infinity its limit and takes no NaN
        f[1, 2, 0, 7], f[5, 0, 0, 100] = (np.nan if link == "logistic" else -np.inf), np.inf
        whole_f, whole_s, whole_c = _check(hip, f, 0, t, dt, u, beyond, link, off)
        rc1, f1, s1, c1, g1 = _curves(hip, f[:3], 0, t[:3], dt[:3], u, beyond, link, off)
        rc2, f2, s2, c2, g2 = _curves(hip, f[3:], 0, t[3:], dt[3:], u, beyond, link, off, state=s1, count=c1)
        assert rc1 == 0 and rc2 == 0 and g1 and g2 and c2 == whole_c == (2 if link == "logistic" else 0)
        assert same_bits(np.concatenate([f1, f2]), whole_f) and same_bits(s2, whole_s)
        want_f, want_s, want_c = _reference(f[3:], 0, t[3:], dt[3:], u, beyond, link, off, state=s1, count=c1)
        assert same_bits(f2, want_f) and same_bits(s2, want_s) and c2 == want_c


@pytest.mark.parametrize("link", ["probit", "logistic"])
def test_the_edge_values(hip, link):
    """-40 leaves S unchanged, +40 collapses it for good, a curve never rises; a NaN and the infinities under the logistic
    link (NaN factors, counted), the infinities under the probit link (their limits 0.0 and 1.0; its predictor must not be
    a NaN); a level reached at the first time, at the last time and never; T monotone in u."""
    rng = np.random.default_rng(300)
    A, D, nb = 6, 2, 70
    t, dt, beyond = host.grid(A, origin=0.5, rng=rng)
    f = rng.normal(0, 1, (A, D, 1, nb))
    f[2], f[4, 1] = -40.0, 40.0
    f[:, 0, 0, 0], f[:, 0, 0, 1], f[:, 0, 0, 2] = -40.0, -40.0, -40.0
    f[0, 0, 0, 0], f[5, 0, 0, 1] = 0.0, 0.0                                               # 0.5 at the first time; at the last; never
    f[3, 0, 0, 5], f[1, 0, 0, 6], f[1, 0, 0, 7] = (np.nan if link == "logistic" else np.inf), np.inf, -np.inf
    u = [1.0, 0.5, 0.2, 1e-15]
    got_f, got_s, got_c = _check(hip, f, 0, t, dt, u, beyond, link)
    S = got_f[:, :, 0]
    assert np.array_equal(bits(S[2, 1]), bits(S[1, 1])) and np.all(S[4, 1] < 1e-17) and np.all(S[5, 1] <= S[4, 1])
    assert got_s[3, 0, :3].tolist() == [t[0], t[5], beyond] and S[5, 0, :3].tolist() == [0.5, 0.5, 1.0]
    clean = np.ones(nb, bool)
    clean[5:8] = False
    assert np.all(np.diff(np.concatenate([np.ones((1, D, nb)), S])[:, :, clean], axis=0) <= 0.0)
    T = got_s[2:]
    assert np.all(np.diff(T, axis=0) >= 0.0) and np.all(np.isin(T, np.concatenate([t, [beyond]])))
    if link == "logistic":
        assert got_c == 3 and np.all(np.isnan(S[3:, 0, 5])) and np.all(np.isnan(S[1:, 0, 6:8])) and np.all(T[3, 0, 5:8] == beyond)
    else:
        assert got_c == 0 and np.all(S[3:, 0, 5] == 0.0) and T[3, 0, 5] == t[3] and np.all(S[1:, 0, 6] == 0.0) and S[1, 0, 7] == S[0, 0, 7]


def test_every_refusal_leaves_the_predictions_the_state_and_the_counter_untouched(hip):
    rng = np.random.default_rng(400)
    A, D, K, nb = 3, 2, 2, 70
    t, dt, beyond = host.grid(A, rng=rng)
    f, off, u = rng.normal(size=(A, D, K, nb)), rng.normal(0, 0.3, nb), np.array([0.9, 0.5])
    vec = lambda *v: np.array(v, np.float64)  # noqa: E731
    keep = {"t_nan": vec(t[0], np.nan, t[2]), "t_inf": vec(t[0], t[1], np.inf), "t_eq": vec(t[0], t[0], t[2]), "t_down": vec(t[0], t[2], t[1]),
            "dt_0": vec(dt[0], 0.0, dt[2]), "dt_neg": vec(-1.0, dt[1], dt[2]), "dt_nan": vec(dt[0], dt[1], np.nan), "dt_inf": vec(np.inf, dt[1], dt[2]),
            "u_0": vec(0.9, 0.0), "u_big": vec(1.5, 0.5), "u_nan": vec(0.9, np.nan), "long": np.arange(1.0, 66.0)}
    p = lambda name: keep[name].ctypes.data  # noqa: E731
    cases = [
        (dict(f=None), "f_dev is null"), (dict(t=None), "t_host is null"), (dict(dt=None), "dt_host is null"),
        (dict(state=None), "state_dev is null"), (dict(cnt=None), "n_nonfinite_dev is null"), (dict(u=None), "u_host is null"),
        (dict(D=0), "D must be >= 1"), (dict(A=0), "A must be >= 1"), (dict(nb=0), "nb must be >= 1"), (dict(nb=-3), "nb must be >= 1"),
        (dict(A=65, t=p("long"), dt=p("long")), "A must be <= PGB_ARMS_MAX = 64"),
        (dict(Q=5), "Q must be in [0, PGB_SURV_MAX_LEVELS = 4]"), (dict(Q=-1), "Q must be in [0, PGB_SURV_MAX_LEVELS = 4]"),
        (dict(ldd=nb - 1), "ldd must be >= nb"), (dict(lda=K * nb + nb - 1), "lda must be >= (D - 1) ldd + nb"),
        (dict(lda=1 << 51), "lda or ldd overflows the index arithmetic"), (dict(ldd=1 << 46, lda=1 << 50), "lda or ldd overflows"),
        (dict(nb=(1 << 38) + 1, ldd=1 << 39, lda=1 << 41), "nb must be <= 2^38"),
        (dict(transform=0), "transform must be PGB_ROWSUM_LOGISTIC or PGB_ROWSUM_PROBIT"), (dict(transform=1), "transform must be"),
        (dict(transform=4), "transform must be"), (dict(transform=-1), "transform must be"),
        (dict(t=p("t_nan")), "t_host[1] is not finite"), (dict(t=p("t_inf")), "t_host[2] is not finite"),
        (dict(t=p("t_eq")), "t_host[1] must be > t_host[0]"), (dict(t=p("t_down")), "t_host[2] must be > t_host[1]"),
        (dict(dt=p("dt_0")), "dt_host[1] must be finite and > 0"), (dict(dt=p("dt_neg")), "dt_host[0] must be finite and > 0"),
        (dict(dt=p("dt_nan")), "dt_host[2] must be finite and > 0"), (dict(dt=p("dt_inf")), "dt_host[0] must be finite and > 0"),
        (dict(u=p("u_0")), "u_host[1] must lie in (0, 1]"), (dict(u=p("u_big")), "u_host[0] must lie in (0, 1]"),
        (dict(u=p("u_nan")), "u_host[1] must lie in (0, 1]"),
        (dict(beyond=float(t[-1])), "beyond must be finite and > t_host[A - 1]"), (dict(beyond=float("inf")), "beyond must be finite"),
        (dict(beyond=float("nan")), "beyond must be finite"), (dict(beyond=float(t[0])), "beyond must be finite and > t_host[A - 1]"),
    ]
    for change, msg in cases:
        rc, got_f, got_s, got_c, guards = _curves(hip, f, 1, t, dt, u, beyond, "probit", off, count=5, change=change)
        text = hip.lib.lib.pgb_last_error().decode()
        assert rc == E_INVALID and msg in text and text.startswith("pgb_surv_curves: "), (change, rc, text)
        assert guards and np.array_equal(bits(got_f), bits(f)) and np.all(got_s == GUARD) and got_c == 5, change
    rc, _, got_s, _, guards = _curves(hip, f, 1, t, dt, [], beyond, "probit", change=dict(u=None))   # Q == 0: no levels, no u
    assert rc == 0 and guards and same_bits(got_s, _reference(f, 1, t, dt, [], beyond, "probit")[1])


# ------------------------------------------------------------------ end to end
N_SUBJECTS, M_FIT, J_FIT = 300, 10, 6


def simulate(rng):
    """300 subjects, three covariates; the hazard of every period is 0.5 where the first covariate is positive and 0.05
    elsewhere; follow-up ends with period 6."""
    Z = rng.normal(size=(N_SUBJECTS, 3))
    high = Z[:, 0] > 0
    first = rng.geometric(np.where(high, 0.5, 0.05))                                      # the period of the event
    event = first <= J_FIT
    return Z, high, np.minimum(first, J_FIT).astype(np.float64), event


def fit_on(backend):
    """Two chains of 8 draws (probit, m = 10) on the person-period rows -> ``(X (one row per subject, the time column
    empty), the group of every subject, the grid, the sampler)``."""
    Z, high, time, event = simulate(np.random.default_rng(71))
    pp = person_period(time, event, Z, times=np.arange(1.0, J_FIT + 1))
    op = BARTOp(pp["X"], pp["y"], m=M_FIT)
    attach_history(op, [sample_chain(op, 30, 8, random_seed=5, chain=c, backend=backend, keep_draws=False, batch=(1.0, 1.0),
                                     likelihood=BernoulliLikelihood("probit")) for c in (0, 1)])
    X = np.column_stack([np.zeros(N_SUBJECTS), Z])
    return X, np.where(high, "high", "low"), pp["times"], _get_posterior_sampler(op, backend=backend)


@pytest.fixture(scope="module")
def fit(hip):
    return fit_on(hip)


def _history(s):
    pool, table = s.pooled_history() if hasattr(s, "pooled_history") else (s.pool, s.forest_idx)
    return (pool.decoded() if hasattr(pool, "decoded") else pool), np.asarray(table)


def _same_results(got, want):
    for key in PER_ROW + PER_DRAW + ("group_weight", "n_list_trees", "times"):
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    assert got["n_nonfinite"] == want["n_nonfinite"] and got["group_labels"].tolist() == want["group_labels"].tolist()
    assert got["beyond"] == want["beyond"]


def test_survival_curves_under_blocking_under_chunking_and_against_the_host_backend(hip, oracle, fit, monkeypatch):
    X, groups, times, s = fit
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    monkeypatch.delenv("PGB_SURV_TIME_CHUNK", raising=False)
    kw = dict(levels=(0.75, 0.5), groups=groups, weights=np.random.default_rng(72).uniform(0.5, 2.0, N_SUBJECTS))
    whole = survival_curves(s, X, times, **kw)
    assert whole["n_draws"] == 16 and whole["n_nonfinite"] == 0 and whole["group_labels"].tolist() == ["high", "low"]
    assert whole["surv_mean"].shape == (N_SUBJECTS, J_FIT) and whole["surv_avg"].shape == (16, 2, J_FIT) and whole["beyond"] == 7.0
    assert 0 < whole["n_list_trees"].max() <= M_FIT                                        # (the hazard is flat: few trees use the time)
    matrix = survival_matrix(s, X, times)
    assert matrix.shape == (16, N_SUBJECTS, J_FIT) and np.all(np.diff(matrix, axis=2) <= 0.0) and np.all(matrix[:, :, 0] <= 1.0)
    assert np.allclose(matrix.mean(axis=0), whole["surv_mean"], rtol=1e-12)
    job = surv.SurvJob(s, X, times, 0, 0, "probit", None, 0.0, None, None)
    job.take_summaries((0.03, 0.5, 0.97), 0.94, kw["levels"], kw["weights"], kw["groups"])
    monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(job.ws_bytes + 100 * job.curves_row_bytes()))   # blocks of 64 rows
    _same_results(survival_curves(s, X, times, **kw), whole)
    assert np.array_equal(bits(survival_matrix(s, X, times)), bits(matrix))
    for chunk in ("1", "4"):
        monkeypatch.setenv("PGB_SURV_TIME_CHUNK", chunk)                                  # (still in blocks of 64 rows)
        _same_results(survival_curves(s, X, times, **kw), whole)
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    _same_results(survival_curves(s, X, times, **kw), whole)                              # chunks of 4, one block
    monkeypatch.delenv("PGB_SURV_TIME_CHUNK", raising=False)
    draws = [1, 6, 9, 15]
    few = survival_curves(s, X, times, draws=draws, **kw)
    for key in ("surv_avg", "rmst_avg"):
        assert np.array_equal(bits(few[key]), bits(whole[key][draws])), key
    pool, table = _history(s)
    on_host = PosteriorSampler(pool, np.ascontiguousarray(table, np.int32), M_FIT, 1, backend=host.HostBackend(oracle, pool))
    _same_results(survival_curves(on_host, X, times, **kw), whole)
    # the one sanity check: half of the high-hazard group is gone after one period, a twentieth of the other
    last = whole["surv_avg_mean"][:, -1]
    print("surv_avg_mean at the last time (high, low):", last, "rmst_avg_mean:", whole["rmst_avg_mean"])
    assert last[0] < last[1]
