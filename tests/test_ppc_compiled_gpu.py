"""Sampler bodies of compiled likelihoods on the MI355X: ``k_ppc_compiled`` through ``pgb_ppc_draw_compiled`` against the
host build of the same text (``CompiledSampler.host_draw``) -- bit for bit, across the chunk and workgroup edges, in
place and out of place, the PIT counts, the refusals -- against ``pgb_ppc_draw`` for the bodies that restate a built-in
family, and end to end through the five public calls on a short real chain.

"Bit for bit" is the 64-bit pattern of every value, as in ``test_rowsummary_gpu.same``."""
import ctypes as C
import warnings

import numpy as np
import pytest

import _ppc_compiled_cases as cases
import _rowsummary_host as rowsum
from pymc_bart_amd import (BARTOp, CompiledLikelihood, NormalLikelihood, _abi, loo_pit, loo_predictive,
                           pointwise_log_likelihood, posterior_predictive, predictive_pit, predictive_summary,
                           psis_expectation_matrix)
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.compiled import compile_loglik
from pymc_bart_amd.sampler import PyBartSettings, PySampler
from pymc_bart_amd.utils import _get_posterior_sampler
from test_ppc_gpu import PIT_SENTINEL, ROW0, SENTINEL, device, inputs, padded
from test_rowsummary_gpu import same

pytestmark = pytest.mark.gpu

SHAPES = [(D, 65) for D in (1, 2, 31, 32, 33, 65)] + [(33, n) for n in (1, 63, 64, 257)]


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)


def draw(hip, build, mu, params, n, row0=0, seed=5, offset=None, aux=None, y=None, out="apart", D=None, K=None, ld=None,
         ld_out=None, n_params=None, code=None, null=()):
    """pgb_ppc_draw_compiled on the device copy of ``mu`` (D, K, ld) -> (rc, out (D, ld_out) or None, pit (2 n + 8,) or
    None, flags, the device copy of mu afterwards).  ``code``: other bytes than the build's; ``null``: arguments passed
    as null pointers."""
    mem, lib = hip.mem, hip.lib
    DD, KK, LD = mu.shape
    md = mem.from_host(np.ascontiguousarray(mu))
    blob = build.code if code is None else code
    buf = C.create_string_buffer(blob, len(blob))
    lik = _abi.PpcCode()
    lik.code_object, lik.code_bytes = C.cast(buf, C.c_void_p), len(blob)
    par = np.ascontiguousarray(params, np.float64)
    lik.n_params = par.shape[1] if n_params is None else n_params
    lik.params_host = par.ctypes.data if par.size else None
    offd = None if offset is None else mem.from_host(np.ascontiguousarray(offset))
    lik.offset_dev = None if offd is None else mem.ptr(offd)
    auxd = None if aux is None else mem.from_host(np.ascontiguousarray(aux, np.float64))
    lik.aux_dev = None if auxd is None else mem.ptr(auxd)
    lo = LD if ld_out is None else ld_out
    outd = {"apart": lambda: mem.from_host(np.full((DD, lo), SENTINEL)), "in place": lambda: md, None: lambda: None}[out]()
    yd = None if y is None else mem.from_host(np.ascontiguousarray(y, np.float64))
    pd = None if y is None else mem.from_host(np.concatenate([np.zeros(2 * n, np.int32), np.full(8, PIT_SENTINEL, np.int32)]))
    flags = (C.c_int64 * 2)(-1, -1)
    rc = lib.ppc_compiled_entry_point()(None if "mu" in null else mem.ptr(md), DD if D is None else D, KK if K is None else K, n,
                                        LD if ld is None else ld, row0, None if "code" in null else C.byref(lik), seed,
                                        None if outd is None else mem.ptr(outd), lo, None if yd is None else mem.ptr(yd),
                                        None if pd is None or "pit" in null else mem.ptr(pd),
                                        None if "flags" in null else flags, mem.stream_ptr)
    return (rc, None if out != "apart" else mem.to_host(outd).reshape(DD, -1), None if pd is None else mem.to_host(pd),
            (int(flags[0]), int(flags[1])), mem.to_host(md).reshape(mu.shape))


def other_inputs(name: str, D: int, n: int, seed: int):
    """-> (build, mu (D, K, n), params, offset (K, n), aux (n,) or None) of the bodies no family has."""
    rng = np.random.default_rng(seed)
    if name == "zip_aux":
        return (cases.build(cases.ZIP_AUX), rng.normal(1.0, 1.5, (D, 1, n)), np.array([[0.1 + 0.01 * (d % 30)] for d in range(D)]),
                rng.normal(0.0, 0.5, (1, n)), rng.uniform(0.0, 0.5, n))
    if name == "hetero":
        return (cases.build(cases.HETERO, 2), rng.normal(1.0, 1.5, (D, 2, n)), np.array([[0.5 + 0.02 * d] for d in range(D)]),
                rng.normal(0.0, 0.5, (2, n)), None)
    assert name == "loop3"
    return cases.build(cases.LOOP3), rng.normal(1.0, 1.5, (D, 1, n)), np.zeros((D, 0)), rng.normal(0.0, 0.5, (1, n)), None


# ------------------------------------------------------------------ 1. the device equals the host build
@pytest.mark.parametrize("case", list(cases.RESTATED) + ["zip_aux", "hetero", "loop3"])
def test_device_equals_the_host_build(case, hip):
    for j, (D, n) in enumerate(SHAPES):
        if case in cases.RESTATED:
            build = cases.restated(case)
            family, mu, params, off = inputs(case, D, n, seed=100 * D + n)
            aux = None
        else:
            family = None
            build, mu, params, off, aux = other_inputs(case, D, n, seed=100 * D + n)
        row0 = ROW0[j % 2]
        for offset in (None, off):
            y = np.round(mu[0, 0]) if offset is None else None       # (the counts ride along on half the calls)
            want, wpit, wflags = build.host_draw(mu if offset is None else mu + offset[None], params, aux, seed=5, row0=row0, y=y)
            rc, got, pit, flags, mu_after = draw(hip, build, padded(mu), params, n, row0, 5,
                                                 None if offset is None else padded(off), aux, y)
            what = (case, D, n, row0, offset is not None)
            assert rc == 0, what
            assert same(got[:, :n], want), what
            assert np.all(got[:, n:] == SENTINEL) and same(mu_after, padded(mu)), what   # the padding, the input
            assert flags == wflags, what
            if y is not None:
                assert np.array_equal(pit[:2 * n].reshape(2, n), wpit) and np.all(pit[2 * n:] == PIT_SENTINEL), what
            if family is not None:   # a restated body: also the built-in kernel on the same device matrix
                rc, builtin, bpit, bflags, _ = device(hip, family, padded(mu), params, n, row0, 5,
                                                      None if offset is None else padded(off), y)
                assert rc == 0 and same(builtin[:, :n], got[:, :n]) and bflags == flags, what
                assert y is None or np.array_equal(bpit, pit), what


# ------------------------------------------------------------------ 2. in place, counts
@pytest.mark.parametrize("case", ["normal", "negbin_log"])
def test_in_place_gives_the_same_bits(case, hip):
    D, n = 65, 257
    build = cases.restated(case)
    _, mu, params, off = inputs(case, D, n, seed=8)
    rc, apart, _, flags, _ = draw(hip, build, padded(mu), params, n, 9, 5, padded(off))
    rc2, _, _, flags2, inplace = draw(hip, build, padded(mu), params, n, 9, 5, padded(off), out="in place")
    assert rc == 0 and rc2 == 0 and flags == flags2
    assert same(inplace[:, 0, :n], apart[:, :n]) and np.all(inplace[:, 0, n:] == SENTINEL)


def test_pit_counts_without_a_matrix(hip):
    D, n = 65, 257
    build, mu, params, off, aux = other_inputs("zip_aux", D, n, seed=3)
    yrep, _, _ = build.host_draw(mu + off[None], params, aux, seed=6, row0=ROW0[1])
    y = yrep[np.random.default_rng(4).integers(0, D, n), np.arange(n)]
    _, wpit, wflags = build.host_draw(mu + off[None], params, aux, seed=6, row0=ROW0[1], y=y)
    assert np.array_equal(wpit[0], (yrep < y).sum(0)) and np.array_equal(wpit[1], (yrep == y).sum(0))
    rc, out, pit, flags, _ = draw(hip, build, padded(mu), params, n, ROW0[1], 6, padded(off), aux, y, out=None)
    assert rc == 0 and out is None and flags == wflags
    assert np.array_equal(pit[:2 * n].reshape(2, n), wpit) and np.all(pit[2 * n:] == PIT_SENTINEL)


def test_the_cap_and_the_call_cap_are_counted_on_the_device(hip):
    D, n = 3, 70
    none = np.zeros((D, 0))
    build = cases.build(cases.OVERFLOW)
    aux = (np.arange(n) % 2).astype(np.float64)
    want, _, wflags = build.host_draw(np.ones((D, 1, n)), None, aux, seed=2)
    rc, got, _, flags, _ = draw(hip, build, np.ones((D, 1, n)), none, n, seed=2, aux=aux)
    assert rc == 0 and same(got, want) and flags == wflags == (D * n, 0)
    assert np.all(np.abs(got) == 1.7976931348623157e308)
    build = cases.build(cases.LOOP1025)
    want, _, wflags = build.host_draw(np.ones((D, 1, n)), None, seed=2)
    rc, got, _, flags, _ = draw(hip, build, np.ones((D, 1, n)), none, n, seed=2)
    assert rc == 0 and same(got, want) and flags == wflags == (0, D * n)


# ------------------------------------------------------------------ 3. refusals
def _refused(hip, msg, build, mu, params, n, **kw):
    rc, out, pit, flags, mu_after = draw(hip, build, mu, params, n, **kw)
    assert rc == -1, msg                                                 # PGB_E_INVALID
    with pytest.raises(_abi.PGBError, match=msg):
        hip.lib.check(rc, "pgb_ppc_draw_compiled")
    assert out is None or np.all(out == SENTINEL), msg
    assert pit is None or (np.all(pit[:2 * n] == 0) and np.all(pit[2 * n:] == PIT_SENTINEL)), msg
    assert same(mu_after, mu) and flags == (-1, -1), msg


def test_refusals_before_any_launch(hip):
    D, n = 4, 20
    mu = np.zeros((D, 1, n + 5))
    one = np.ones((D, 1))
    none = np.zeros((D, 0))
    normal = cases.restated("normal")
    density = "double z = (y - mu) / s; return -0.5 * z * z - log(s);"
    # the other two kinds of code object
    _refused(hip, "built without pointwise=True.*mark 0: pgb_ppc_draw_compiled takes one built from a sampler body",
             normal, mu, one, n, code=compile_loglik(density, ["s"]).code)
    _refused(hip, "built with pointwise=True.*mark 1: pgb_ppc_draw_compiled takes one built from a sampler body",
             normal, mu, one, n, code=compile_loglik(density, ["s"], pointwise=True).code)
    _refused(hip, "not a gfx950 code object", normal, mu, one, n, code=b"\0" * 4096)
    _refused(hip, "compiled for 1 params, the call gives n_params = 0", normal, mu, none, n)
    _refused(hip, "compiled for 1 params, the call gives n_params = 2", normal, mu, np.ones((D, 2)), n)
    _refused(hip, "compiled for 1 outputs, the call has K = 2", normal, np.zeros((D, 2, n)), one, n)
    _refused(hip, "compiled for 2 outputs, the call has K = 1", cases.build(cases.HETERO, 2), mu, one, n)
    _refused(hip, "K must be in", normal, mu, one, n, K=17)
    for bad in (np.nan, np.inf):
        _refused(hip, "params must be finite: param 0 of draw 2", normal, mu, np.array([[1.0], [1.0], [bad], [bad]]), n)
    # the rules of pgb_ppc_draw
    _refused(hip, "D must be >= 1", normal, mu, one, n, D=0)
    _refused(hip, "n_rows must be >= 1", normal, mu, one, 0)
    _refused(hip, "ld must be >= n_rows", normal, mu, one, n, ld=n - 1)
    _refused(hip, "ld_out must be >= n_rows", normal, mu, one, n + 5, ld_out=n)
    _refused(hip, "row0 must be >= 0", normal, mu, one, n, row0=-1)
    _refused(hip, "no output", normal, mu, one, n, out=None)
    _refused(hip, "out_dev overlaps mu_dev", cases.build(cases.HETERO, 2), np.zeros((D, 2, n)), one, n, out="in place")
    _refused(hip, "out_dev overlaps mu_dev", normal, mu, one, n, out="in place", ld_out=n)
    _refused(hip, "mu_dev is null", normal, mu, one, n, null=("mu",))
    _refused(hip, "lik is null", normal, mu, one, n, null=("code",))
    _refused(hip, "y_dev and pit_counts_dev come together", normal, mu, one, n, y=np.zeros(n), null=("pit",))
    rc, *_ = draw(hip, normal, mu, one, n, null=("flags",))
    with pytest.raises(_abi.PGBError, match="flags_host is null"):
        hip.lib.check(rc, "pgb_ppc_draw_compiled")
    # pgb_ppc_draw keeps its words for the family
    rc, *_ = device(hip, 11, mu, none, n)
    with pytest.raises(_abi.PGBError, match="the compiled family has a log density only"):
        hip.lib.check(rc, "pgb_ppc_draw")


def test_a_sampler_object_is_refused_by_the_other_entry_points(hip):
    rng = np.random.default_rng(3)
    n, p = 300, 3
    X = rng.uniform(0, 1, (n, p))
    y = X[:, 0] + rng.normal(0, 0.3, n)
    density = "double z = (y - mu) / s; return -0.5 * z * z - log(s);"
    lik = CompiledLikelihood(density, {"s": 1.0}, sampler="return mu + s * normal();")
    blob = lik.compiled_sampler().code
    # pgb_set_loglik_code: refused, and the handle still steps
    st = PyBartSettings.from_data(X, y, m=5, num_particles=10, seed=1, family="compiled")
    s = PySampler(st, X, y, np.zeros(p, np.int32), np.ones(p), backend=hip)
    set_code, _ = s.backend.lib.compiled_entry_points()
    rc = set_code(s._h, blob, len(blob), 1)
    assert rc == -1
    with pytest.raises(_abi.PGBError, match="built from a sampler body.*mark 2: pgb_set_loglik_code takes one built without pointwise=True "
                                             r"\(a sampler's pass kernel"):
        s.backend.lib.check(rc, "pgb_set_loglik_code")
    with pytest.raises(_abi.PGBError, match="pgb_set_loglik_code first"):
        s.step(True)                                                      # nothing was installed
    s.set_compiled_likelihood(lik)
    s.set_likelihood([1.0])
    a, _ = s.step(True)
    assert np.all(np.isfinite(a))
    # pgb_pointwise_loglik: refused by the mark
    op = BARTOp(X, y, m=5)
    chain = sample_chain(op, 4, 4, random_seed=1, chain=0, backend=hip, keep_draws=False)
    attach_history(op, [chain])
    fit = _get_posterior_sampler(op, backend=hip)
    lik._builds[(64, False, True)] = lik.compiled_sampler()
    with pytest.raises(_abi.PGBError, match="built from a sampler body.*mark 2: pgb_pointwise_loglik takes one built with pointwise=True"):
        pointwise_log_likelihood(fit, X, y, lik)


# ------------------------------------------------------------------ 4. end to end
N, P, M_TREES, TUNE, DRAWS = 300, 4, 10, 12, 12


@pytest.fixture(scope="module")
def fit(hip):
    """One short chain of a Normal fit; the censored likelihood with its latent-response sampler reads it."""
    rng = np.random.default_rng(41)
    X = rng.uniform(0, 1, (N, P))
    f = 2.0 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 1.5 * (X[:, 2] - 0.5) + X[:, 3]
    y = f + rng.normal(0, 0.5, N)
    op = BARTOp(X, y, m=M_TREES)
    chain = sample_chain(op, TUNE, DRAWS, random_seed=2, chain=0, backend=hip, keep_draws=False)
    attach_history(op, [chain])
    multi = _get_posterior_sampler(op, backend=hip)
    sigma = np.asarray(chain["sigma"], np.float64)
    pred = multi.sample_posterior(X, list(range(DRAWS)), None)
    aux = (rng.uniform(size=N) < 0.2).astype(np.float64)                # the censored rows
    lik = CompiledLikelihood(cases.CENSORED_DENSITY, {"s": "sigma"}, aux=aux, sampler=cases.LATENT)
    return X, y, multi, lik, {"sigma": sigma}, sigma[:, None], pred


def _quiet(f, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return f(*a, **kw)


def test_end_to_end_on_a_short_chain(fit, hip, monkeypatch):
    X, y, multi, lik, points, params, pred = fit
    assert pred.shape == (DRAWS, 1, N)
    build = lik.compiled_sampler()
    off = np.random.default_rng(5).normal(0, 0.3, (1, N))
    for kw in ({"random_seed": 7}, {"random_seed": 8, "offset": off}):
        seed = kw["random_seed"]
        mu = pred if "offset" not in kw else pred + off[None]
        want, _, wflags = build.host_draw(mu, params, lik.aux, seed=seed)
        assert wflags == (0, 0)
        results = []
        for blk in (None, str(1 << 16)):                                 # one block, blocks of 64 rows
            monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
            if blk:
                monkeypatch.setenv("PGB_PW_BLOCK_BYTES", blk)
            yrep, info = posterior_predictive(multi, X, lik, points=points, return_info=True, **kw)
            summ = predictive_summary(multi, X, lik, points=points, **kw)
            pit = predictive_pit(multi, X, y, lik, points=points, **kw)
            lpit = _quiet(loo_pit, multi, X, y, lik, points=points, **kw)
            ly = _quiet(loo_predictive, multi, X, y, lik, points=points, kind="y", **kw)
            results.append((yrep, info, summ, pit, lpit, ly))
        monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
        yrep, info, summ, pit, lpit, ly = results[0]
        assert yrep.shape == (DRAWS, N) and same(yrep, want) and info == {"n_capped": 0, "n_exhausted": 0}
        ref = rowsum.public(want, (0.03, 0.5, 0.97), 0.94)
        for key in ("mean", "var", "sd", "quantiles", "hdi"):
            assert summ[key].shape == ref[key].shape and same(summ[key], ref[key]), key
        assert summ["n_draws"] == DRAWS and summ["n_capped"] == 0 and summ["n_exhausted"] == 0
        assert np.array_equal(pit["n_below"], (want < y).sum(0)) and np.array_equal(pit["n_equal"], (want == y).sum(0))
        assert np.array_equal(pit["pit"], ((want < y).sum(0) + 0.5 * (want == y).sum(0)) / DRAWS) and pit["n_draws"] == DRAWS
        # the PSIS-weighted calls: psis_expectation_matrix of the two host matrices
        ll = pointwise_log_likelihood(multi, X, y, lik, points=points, offset=kw.get("offset"))
        wp = _quiet(psis_expectation_matrix, ll, want, y=y, kind="pit", backend=hip)
        wv = _quiet(psis_expectation_matrix, ll, want, backend=hip)
        assert same(lpit["loo_pit"], wp["loo_pit"]) and same(lpit["pareto_k_i"], wp["pareto_k_i"])
        assert same(ly["loo_mean"], wv["loo_mean"]) and same(ly["loo_sd"], wv["loo_sd"])
        assert same(ly["loo_residual"], y - wv["loo_mean"])
        for res in (lpit, ly):
            assert res["n_capped"] == 0 and res["n_exhausted"] == 0
        # ... whatever the blocking
        for a, b in zip(results[1], results[0]):
            if isinstance(a, np.ndarray):
                assert same(a, b)
                continue
            assert a.keys() == b.keys()
            for key in a:
                assert same(a[key], b[key]) if isinstance(a[key], np.ndarray) else a[key] == b[key], key
    # the Normal body against the built-in Normal family
    normal = posterior_predictive(multi, X, NormalLikelihood("sigma"), points=points, random_seed=7, offset=off)
    body = posterior_predictive(multi, X, lik, points=points, random_seed=7, offset=off)
    assert same(body, normal)
