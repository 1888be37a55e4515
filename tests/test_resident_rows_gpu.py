"""Rows that already live in HBM, on the MI355X: every stored-draw consumer that takes a device matrix --
``sample_posterior``, ``ice_mean``, ``pdp_sweep``, ``shap``, ``shap_interactions`` -- against the same call on the host
``ndarray`` of the same values.  Both run the same kernels on the same doubles, so the comparison is ``np.array_equal``
on the ``uint64`` views: tolerance 0.  What differs is where the doubles come from: a handle from ``resident_rows``, a
tensor torch made, and the views a caller gets by slicing one (a column slice, a row step, a transpose), whose flat read
from ``data_ptr()`` is another matrix.  The memory around a view holds 7.0e77, which must reach no output.

No test here builds a view whose flat read of ``n p`` doubles from its data pointer would leave the view's own storage
(no ``expand``, no zero stride): a consumer that mis-reads a view gives wrong numbers, never an out-of-bounds access."""
import os
import re

import numpy as np
import pytest
import torch

import _ice_host as ice_host
from pymc_bart_amd import BARTOp, importance, partial, pdp, shap
from pymc_bart_amd.chains import sample_chain
from pymc_bart_amd.utils import _MultiChainSampler, _resident_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAXP = int(re.search(r"#define PRED_LDS_MAXP (\d+)", open(os.path.join(ROOT, "pymc_bart_amd", "csrc", "pgb_pred_walk.h")).read()).group(1))
POISON = 7.0e77
FORMS = ["handle", "torch", "column-slice", "row-step", "transpose"]
CONSUMERS = ["sample_posterior", "ice_mean", "pdp_sweep", "shap", "shap_interactions", "shap_interactions_cols"]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same(got, want):
    """Tuples of arrays, equal in shape and in every bit."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == np.float64 and g.shape == w.shape
        assert np.array_equal(_bits(g), _bits(w)), f"{np.count_nonzero(_bits(g) != _bits(w))} of {g.size} entries differ"
        assert not (np.abs(g) > 1e60).any()                           # nothing of the poison around a view


def _data(rng, n, p, nan_rate=0.08):
    X = rng.normal(size=(n, p))
    X[rng.random((n, p)) < nan_rate] = np.nan
    return X


def _calls(s, p, full_interactions=True):
    """The consumers as functions of ``X`` alone, each returning a tuple of arrays; arguments fixed per sampler."""
    D = s.n_draws
    rng = np.random.default_rng(17)
    picks = [1, D - 1, 1, 0]                                          # repeated picks
    cols = [p - 1, 0, p // 2] if p > 2 else [0]
    sub = [4, 1] if p == 5 else cols
    inst = rng.normal(size=(3, p))
    ipicks = rng.integers(0, D, size=(len(cols), 3, 4))
    ppicks = rng.integers(0, D, size=(len(cols), 8))
    calls = {
        "sample_posterior": lambda X: (s.sample_posterior(X, picks, None), s.sample_posterior(X, picks, [p // 2])),
        "ice_mean": lambda X: (s.ice_mean(X, inst, cols, ipicks),),
        "pdp_sweep": lambda X: (s.pdp_sweep(X, cols, ppicks),),
        "shap": lambda X: tuple(s.shap(X, picks)),
        "shap_interactions_cols": lambda X: tuple(s.shap_interactions(X, picks, sub)),
    }
    if full_interactions:
        calls["shap_interactions"] = lambda X: tuple(s.shap_interactions(X, picks))
    return calls


def _form(name, hip, s, X):
    """``(what is passed as X, the tensor that owns its storage)`` for the host matrix ``X (n, p)``."""
    n, p = X.shape
    dev = hip.mem.device
    if name == "handle":
        t = s.resident_rows(X)
        return t, t
    if name == "torch":
        t = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        return t, t
    if name == "column-slice":                                        # n p doubles from offset 2 of n (p + 3)
        W = np.full((n, p + 3), POISON)
        W[:, 2:p + 2] = X
        Wd = torch.from_numpy(W).to(dev)
        return Wd[:, 2:p + 2], Wd
    if name == "row-step":                                            # n p doubles of 2 n p
        W2 = np.full((2 * n, p), POISON)
        W2[::2] = X
        W2d = torch.from_numpy(W2).to(dev)
        return W2d[::2], W2d
    assert name == "transpose"                                        # n p doubles of n p
    Td = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
    return Td.T, Td


def _call_and_leave_alone(call, t, owner, X):
    """``call(t)``; afterwards ``t`` is the view it was, on the bits it had."""
    assert tuple(t.shape) == X.shape and np.array_equal(_bits(t.cpu().numpy()), _bits(X))
    before = _bits(owner.cpu().numpy()).copy()
    meta = (t.data_ptr(), t.stride(), tuple(t.shape), t.dtype, t.device)
    got = call(t)
    assert (t.data_ptr(), t.stride(), tuple(t.shape), t.dtype, t.device) == meta
    assert np.array_equal(_bits(owner.cpu().numpy()), before)
    return got


class _Case:
    """A sampler, its rows, its consumers and -- computed once, on first use -- their results on the host matrix."""

    def __init__(self, s, X, full_interactions=True):
        self.s, self.X, self.p = s, X, X.shape[1]
        self.calls = _calls(s, self.p, full_interactions)
        self._want = {}

    def want(self, name):
        if name not in self._want:
            self._want[name] = self.calls[name](self.X)
            for a in self._want[name]:
                a.setflags(write=False)
                assert not np.isnan(a).any() and np.count_nonzero(a) > 0
        return self._want[name]


@pytest.fixture(scope="module")
def cases(hip):
    rng = np.random.default_rng(1907)
    X = _data(rng, 257, 5)                                            # four full waves and one lane; both walks
    main = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 24, 5, linear=[3]), 7, 6, hip)
    kvec = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 24, 5, K=3, linear=[3]), 7, 6, hip)
    big = np.concatenate([X, X[:200]])                                # 457 rows: eight blocks of 64, the last of 9
    wide = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 21, LDS_MAXP + 1, depth=5, linear=[0, LDS_MAXP]), 7, 4, hip)
    one = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 9, 1), 3, 4, hip)
    return {"K1": _Case(main, X), "K3": _Case(kvec, X),
            "blocks-K1": _Case(main, big), "blocks-K3": _Case(kvec, big),
            "blocks-p127": _Case(wide, _data(rng, 457, LDS_MAXP + 1), full_interactions=False),
            "p1": _Case(one, _data(rng, 65, 1))}


# ------------------------------------------------------------------ a. every consumer x every form
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("consumer", CONSUMERS)
@pytest.mark.parametrize("which", ["K1", "K3"])
def test_every_consumer_takes_every_form_of_the_same_rows(cases, hip, which, consumer, form):
    case = cases[which]
    want = case.want(consumer)
    t, owner = _form(form, hip, case.s, case.X)
    assert t.is_contiguous() == (form in ("handle", "torch"))
    _same(_call_and_leave_alone(case.calls[consumer], t, owner, case.X), want)


def test_a_contiguous_handle_is_read_where_it_lies(cases, hip):
    """No copy on the path the public sweeps take: the tensor the consumers read is the handle itself."""
    case = cases["K1"]
    t = case.s.resident_rows(case.X)
    got = hip.mem.device_rows(t)
    assert got is t and got.data_ptr() == t.data_ptr() and hip.mem.is_resident(t)
    view, _ = _form("column-slice", hip, case.s, case.X)
    copy = hip.mem.device_rows(view)
    assert copy.is_contiguous() and copy.data_ptr() != view.data_ptr() and not hip.mem.is_resident(view)
    assert np.array_equal(_bits(copy.cpu().numpy()), _bits(case.X))


# ------------------------------------------------------------------ b. row blocks over a handle
@pytest.mark.parametrize("form", ["handle", "column-slice"])
@pytest.mark.parametrize("which", ["blocks-K1", "blocks-K3", "blocks-p127"])
def test_row_blocks_over_a_pointer_the_caller_owns(cases, hip, monkeypatch, which, form):
    """``ptr + 8 r0 p`` for blocks of 64 rows, against the unblocked sweep of the host matrix."""
    case = cases[which]
    names = [c for c in ("shap", "shap_interactions", "shap_interactions_cols", "pdp_sweep") if c in case.calls]
    monkeypatch.delenv("PGB_SHAP_BLOCK_BYTES", raising=False)
    monkeypatch.delenv("PGB_PDP_BLOCK_BYTES", raising=False)
    want = {c: case.want(c) for c in names}                           # the default: one block
    monkeypatch.setenv("PGB_SHAP_BLOCK_BYTES", "4096")
    monkeypatch.setenv("PGB_PDP_BLOCK_BYTES", "4096")
    K, p = case.s.n_outputs, case.p
    eight = [(r0, min(457, r0 + 64)) for r0 in range(0, 457, 64)]
    assert len(eight) == 8 and shap.blocks(4 * K * p, 457) == eight  # 4 picks: attributions, then interactions
    assert all(shap.blocks(4 * K * q * q, 457) == eight for q in ((2, 5) if p == 5 else (3,)))
    assert pdp.blocks(3, 8, K, 457) == [(c, c + 1, r0, r1) for c in range(3) for r0, r1 in eight]
    for c in names:
        t, owner = _form(form, hip, case.s, case.X)
        _same(_call_and_leave_alone(case.calls[c], t, owner, case.X), want[c])


# ------------------------------------------------------------------ c. a vector
@pytest.mark.parametrize("consumer", CONSUMERS)
def test_a_vector_on_the_device_is_its_column(cases, hip, consumer):
    case = cases["p1"]
    assert case.X.shape == (65, 1)
    want = case.want(consumer)
    t = torch.from_numpy(np.ascontiguousarray(case.X[:, 0])).to(hip.mem.device)
    assert tuple(t.shape) == (65,)
    got = case.calls[consumer](t)
    assert tuple(t.shape) == (65,) and np.array_equal(_bits(t.cpu().numpy()), _bits(case.X[:, 0]))
    _same(got, want)


# ------------------------------------------------------------------ d. two chains, the handle of the first
def test_two_chains_share_the_handle_of_the_first(hip):
    rng = np.random.default_rng(21)
    a = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 14, 4), 7, 5, hip)
    b = ice_host.pool_sampler(rng, ice_host.random_pool(rng, 18, 4, depth=6, linear=[2]), 7, 3, hip)
    s = _MultiChainSampler([a, b])
    X = _data(rng, 100, 4)
    picks = [0, 6, 4, 7, 5]                                           # chain a, b, a, b, b
    ppicks = np.array([[0, 6, 4, 7], [5, 1, 7, 2]])
    for rows in (a.resident_rows(X), _resident_rows(s, X), _resident_rows([s, s], X)):
        assert hip.mem.is_resident(rows)
        for excl in (None, [1, 3]):
            _same((s.sample_posterior(rows, picks, excl),), (s.sample_posterior(X, picks, excl),))
        _same(s.shap(rows, picks), s.shap(X, picks))
        _same((s.pdp_sweep(rows, [3, 0], ppicks),), (s.pdp_sweep(X, [3, 0], ppicks),))
        assert np.array_equal(_bits(rows.cpu().numpy()), _bits(X))


# ------------------------------------------------------------------ e. the public sweeps
@pytest.fixture(scope="module")
def fits(hip):
    rng = np.random.default_rng(31)
    X = rng.uniform(-1, 1, size=(300, 4))
    Y = 2.0 * X[:, 0] - X[:, 1] ** 2 + rng.normal(0, 0.1, 300)
    Y2 = np.where(X[:, 2] > 0, X[:, 3], -1.0) + rng.normal(0, 0.1, 300)
    ops, stats = [], []
    for y, seed in ((Y, 6), (Y2, 7)):
        ops.append(BARTOp(X, y, m=10))
        stats.append(sample_chain(ops[-1], tune=20, draws=10, num_particles=10, random_seed=seed, sigma=0.2, backend=hip))
    return X, ops, stats


def _with_and_without_the_handle(hip, monkeypatch, module, run):
    """``run()`` with the module's ``_resident_rows`` as it is (recorded: it hands out a device handle) and with one
    that hands the matrix back."""
    handed = []
    real = getattr(module, "_resident_rows")
    monkeypatch.setattr(module, "_resident_rows", lambda sampler, X: (handed.append(real(sampler, X)), handed[-1])[1])
    resident = run()
    assert len(handed) == 1 and hip.mem.is_resident(handed[0])
    monkeypatch.setattr(module, "_resident_rows", lambda sampler, X: X)
    return resident, run()


def test_variable_importance_is_the_same_from_a_handle_and_from_the_matrix(fits, hip, monkeypatch):
    X, ops, stats = fits

    def run():
        return importance.compute_variable_importance(stats[0]["variable_inclusion"], ops[0], X, method="VI", samples=8,
                                                      random_seed=1, backend=hip)

    resident, plain = _with_and_without_the_handle(hip, monkeypatch, importance, run)
    assert resident["preds"].shape == (4, 8, 300) and resident["preds_all"].shape == (8, 300)
    assert np.array_equal(resident["indices"], plain["indices"]) and resident["labels"].tolist() == plain["labels"].tolist()
    _same([resident[k] for k in ("preds", "preds_all", "r2_mean", "r2_hdi")],
          [plain[k] for k in ("preds", "preds_all", "r2_mean", "r2_hdi")])


def test_partial_dependence_of_two_bart_variables_is_the_same_from_a_handle_and_from_the_matrix(fits, hip, monkeypatch):
    X, ops, _ = fits

    def run():
        return partial.partial_dependence(ops, X, xs_interval="insample", samples=8, random_seed=2, backend=hip)

    resident, plain = _with_and_without_the_handle(hip, monkeypatch, partial, run)
    assert list(resident["pd"]) == list(plain["pd"]) == [0, 1, 2, 3] and resident["pd"][0].shape == (8, 300, 2)
    _same([resident["pd"][j] for j in range(4)] + [resident["x"][j] for j in range(4)] + [resident["reference"]],
          [plain["pd"][j] for j in range(4)] + [plain["x"][j] for j in range(4)] + [plain["reference"]])


# ------------------------------------------------------------------ f. the producer on the same stream
def test_rows_made_on_the_current_stream_are_read_behind_their_producer(cases, hip):
    """The library enqueues on the stream torch calls current at the time of the call: rows an asynchronous device op
    is still writing are read after it, with no synchronise in between."""
    case = cases["K1"]
    dev = hip.mem.device
    base_d = torch.from_numpy(case.X).to(dev)
    want_shap, want_pred = case.want("shap"), case.want("sample_posterior")
    torch.cuda.synchronize(dev)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        assert hip.mem.stream_ptr == int(st.cuda_stream) != 0
        stale = torch.full((257, 5), POISON, dtype=torch.float64, device=dev)
        del stale                                                     # (the block the next allocation of this size gets)
        busy = torch.full((4096, 4096), 1.0 / 4096, device=dev)
        for _ in range(4):
            busy = busy @ busy                                        # the stream is busy when the rows are asked for
        Xd = base_d * 1.0
        got_shap = case.calls["shap"](Xd)
        busy = busy @ busy
        Xd2 = base_d * 1.0
        got_pred = case.calls["sample_posterior"](Xd2)
    _same(got_shap, want_shap)
    _same(got_pred, want_pred)
    torch.cuda.synchronize(dev)


# ------------------------------------------------------------------ g. refusals
@pytest.mark.parametrize("consumer", CONSUMERS)
@pytest.mark.parametrize("kind", ["float32", "3-D"])
def test_what_is_no_device_matrix_is_refused_before_anything_is_launched(cases, hip, kind, consumer):
    case = cases["K1"]
    dev = hip.mem.device
    if kind == "float32":
        bad = torch.from_numpy(np.nan_to_num(case.X).astype(np.float32)).to(dev)
        match = r"torch\.float32"
    else:
        bad = torch.zeros((257, 5, 1), dtype=torch.float64, device=dev)
        match = r"X must be a matrix \(n_rows, p\), got shape \(257, 5, 1\)"
    guard = torch.full(np.asarray(case.want(consumer)[0]).shape, -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    before = hip.lib.lib.pgb_last_error()
    with pytest.raises(ValueError, match=match):
        case.calls[consumer](bad)
    torch.cuda.synchronize(dev)
    assert hip.lib.lib.pgb_last_error() == before
    assert bool((guard == -7.0).all())
