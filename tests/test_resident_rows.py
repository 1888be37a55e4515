"""What a stored-draw consumer takes for a device matrix (``TorchHipMemory.device_rows``), rule by rule, with no GPU:
the helper looks at a tensor's type, device, dtype, shape, strides and ``requires_grad`` only, so a memory holder built
without ``__init__`` whose device is the CPU runs every rule on CPU tensors.  Then the oracle backend, whose memory has
no device tensors: ``resident_rows`` hands the matrix back and every consumer takes it as the plain call does."""
import re

import numpy as np
import pytest
import torch

import _ice_host as ice_host
from pymc_bart_amd._device import TorchHipMemory, device_rows


def _mem(device) -> TorchHipMemory:
    mem = TorchHipMemory.__new__(TorchHipMemory)
    mem.device = torch.device(device)
    return mem


@pytest.fixture(scope="module")
def mem():
    return _mem("cpu")


def _arange(n, p):
    return torch.arange(n * p, dtype=torch.float64).reshape(n, p)


def test_the_memory_holder_keeps_what_the_consumers_call():
    for name in ("stream_ptr", "from_host", "device_rows", "is_resident", "empty", "host_result", "ptr", "to_host",
                 "synchronize", "sampler_stream", "output_stream"):
        assert hasattr(TorchHipMemory, name), name


# ------------------------------------------------------------------ 1. the host path
@pytest.mark.parametrize("obj", [np.zeros((3, 2)), [[1.0, 2.0]], ((1.0,), (2.0,)), None, 3.5, "rows"],
                         ids=["ndarray", "list", "tuple", "None", "float", "str"])
def test_what_is_no_tensor_takes_the_host_path(mem, obj):
    assert mem.device_rows(obj) is None and mem.is_resident(obj) is False
    got, resident = device_rows(mem, obj)
    assert got is obj and resident is False


def test_a_tensor_on_the_cpu_takes_the_host_path():
    gpu = _mem("cuda:0")                                           # (a device object: no GPU is touched)
    for t in (_arange(3, 2), _arange(3, 2).float(), _arange(6, 1)[:, 0], _arange(3, 4)[:, 1:3]):
        assert gpu.device_rows(t) is None and gpu.is_resident(t) is False
        got, resident = device_rows(gpu, t)
        assert got is t and resident is False


def test_a_memory_without_device_tensors_takes_the_host_path(oracle):
    X = np.zeros((3, 2))
    t = _arange(3, 2)
    assert not hasattr(oracle.mem, "device_rows") and not hasattr(oracle.mem, "is_resident")
    for obj in (X, t):
        got, resident = device_rows(oracle.mem, obj)
        assert got is obj and resident is False


# ------------------------------------------------------------------ 2. refusals
def test_another_device_is_refused_and_both_are_named(mem):
    t = torch.empty((3, 2), dtype=torch.float64, device="meta")
    with pytest.raises(ValueError, match=r"meta.*cpu"):
        mem.device_rows(t)
    assert mem.is_resident(t) is False
    with pytest.raises(ValueError, match=r"meta.*cuda:1"):
        _mem("cuda:1").device_rows(t)
    with pytest.raises(ValueError, match=r"meta.*cuda:0"):          # (before the dtype is looked at)
        _mem("cuda:0").device_rows(torch.empty((3, 2), dtype=torch.float32, device="meta"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.int64, torch.int32, torch.bool,
                                   torch.complex128], ids=str)
def test_another_dtype_is_refused_and_named(mem, dtype):
    t = torch.zeros((3, 2), dtype=dtype)
    with pytest.raises(ValueError, match=str(dtype).replace(".", r"\.")):
        mem.device_rows(t)
    with pytest.raises(ValueError, match=str(dtype).replace(".", r"\.")):   # (1-D and 3-D too: the dtype comes first)
        mem.device_rows(torch.zeros((2, 2, 2), dtype=dtype))
    assert mem.is_resident(t) is False


@pytest.mark.parametrize("shape", [(), (2, 3, 4), (1, 1, 1, 1), (0,), (0, 3), (3, 0), (0, 0)], ids=str)
def test_what_is_no_matrix_is_refused_with_its_shape(mem, shape):
    t = torch.zeros(shape, dtype=torch.float64)
    shown = (shape + (1,)) if len(shape) == 1 else shape           # (a vector is looked at as its (n, 1) view)
    with pytest.raises(ValueError, match=re.escape(f"X must be a matrix (n_rows, p), got shape {shown}")):
        mem.device_rows(t)
    assert mem.is_resident(t) is False


# ------------------------------------------------------------------ 3. passed through, viewed, detached, copied
@pytest.mark.parametrize("shape", [(257, 5), (1, 5), (257, 1), (1, 1)], ids=str)
def test_a_row_major_matrix_is_the_same_tensor(mem, shape):
    t = _arange(*shape)
    got = mem.device_rows(t)
    assert got is t and got.data_ptr() == t.data_ptr() and mem.is_resident(t) is True
    back, resident = device_rows(mem, t)
    assert back is t and resident is True


def test_a_vector_is_its_column_view(mem):
    t = torch.arange(65, dtype=torch.float64)
    got = mem.device_rows(t)
    assert tuple(got.shape) == (65, 1) and got.data_ptr() == t.data_ptr() and got.is_contiguous()
    assert torch.equal(got[:, 0], t) and tuple(t.shape) == (65,)
    assert mem.is_resident(t) is False and mem.is_resident(got) is True   # (the vector itself is no (n, p) matrix)
    step = torch.arange(130, dtype=torch.float64)[::2]              # a strided vector: its column, copied
    got = mem.device_rows(step)
    assert tuple(got.shape) == (65, 1) and got.is_contiguous() and torch.equal(got[:, 0], step)
    assert got.data_ptr() != step.data_ptr() and step.stride() == (2,)


def test_requires_grad_is_detached(mem):
    t = _arange(7, 3).requires_grad_(True)
    got = mem.device_rows(t)
    assert not got.requires_grad and got.data_ptr() == t.data_ptr() and torch.equal(got, t.detach())
    assert t.requires_grad and mem.is_resident(t) is False and mem.is_resident(got) is True
    view = (_arange(7, 6).requires_grad_(True) * 1.0)[:, 1:4]       # a non-leaf view: detached and copied
    got = mem.device_rows(view)
    assert not got.requires_grad and got.is_contiguous() and torch.equal(got, view.detach())


def _views():
    W, W2, T = _arange(257, 8), _arange(514, 5), _arange(5, 257)
    return {"column-slice": (W, W[:, 2:7]), "row-step": (W2, W2[::2]), "transpose": (T, T.T)}


@pytest.mark.parametrize("name", ["column-slice", "row-step", "transpose"])
def test_any_other_view_is_one_contiguous_copy(mem, name):
    parent, view = _views()[name]
    before, strides = parent.clone(), view.stride()
    assert tuple(view.shape) == (257, 5) and not view.is_contiguous()
    got = mem.device_rows(view)
    assert got is not view and got.is_contiguous() and got.stride() == (5, 1) and tuple(got.shape) == (257, 5)
    assert got.dtype == torch.float64 and got.device == view.device
    want = view.numpy().copy()                                      # numpy's own strided read of the same storage
    assert np.array_equal(got.numpy(), want) and np.array_equal(got.numpy().ravel(), want.ravel())
    lo, hi = parent.data_ptr(), parent.data_ptr() + 8 * parent.numel()
    assert not lo <= got.data_ptr() < hi                            # a copy, not another view of the parent
    assert mem.is_resident(view) is False and mem.is_resident(got) is True and mem.device_rows(got) is got
    assert view.stride() == strides and torch.equal(parent, before)  # the caller's tensor is as it was
    flat = torch.as_strided(view, (257 * 5,), (1,)).numpy().reshape(257, 5)
    assert not np.array_equal(flat, want)                           # (what a flat read from data_ptr() would have seen)


def test_a_single_row_or_column_of_a_wider_matrix(mem):
    W = _arange(9, 8)
    col = W[:, 3:4]                                                 # (9, 1) with rows 8 apart: a copy
    got = mem.device_rows(col)
    assert got.is_contiguous() and got.data_ptr() != col.data_ptr() and torch.equal(got, col)
    row = W[4:5, :]                                                 # (1, 8): dense where it lies
    assert mem.device_rows(row) is row


# ------------------------------------------------------------------ 4. the oracle backend: the matrix comes back
@pytest.fixture(scope="module")
def samplers(oracle):
    rng = np.random.default_rng(5)
    pool = ice_host.random_pool(rng, 24, 5, linear=[3])
    s = ice_host.pool_sampler(rng, pool, 7, 6, oracle)
    pool3 = ice_host.random_pool(rng, 12, 5, K=3, linear=[0])
    s3 = ice_host.pool_sampler(rng, pool3, 4, 5, oracle)
    X = rng.normal(size=(67, 5))
    X[rng.random(X.shape) < 0.08] = np.nan
    return s, s3, X


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("which", [0, 1], ids=["K1", "K3"])
def test_on_the_oracle_the_handle_is_the_matrix_and_every_consumer_takes_it(samplers, which):
    s, X = samplers[which], samplers[2]
    rows = s.resident_rows(X)
    assert isinstance(rows, np.ndarray) and rows.flags.c_contiguous and _same(rows, X)
    one = s.resident_rows(X[:, 0])                                  # a vector: the (n, 1) matrix
    assert one.shape == (67, 1) and _same(one[:, 0], X[:, 0])
    D = s.n_draws
    picks = [0, D - 1, 0, 2]
    assert _same(s.sample_posterior(rows, picks, None), s.sample_posterior(X, picks, None))
    assert _same(s.sample_posterior(rows, picks, [1, 3]), s.sample_posterior(X, picks, [1, 3]))
    cols = [3, 0]
    ipicks = np.random.default_rng(1).integers(0, D, size=(2, 2, 3))
    assert _same(s.ice_mean(rows, X[[4, 9]], cols, ipicks), s.ice_mean(X, X[[4, 9]], cols, ipicks))
    ppicks = np.random.default_rng(2).integers(0, D, size=(2, 4))
    assert _same(s.pdp_sweep(rows, cols, ppicks), s.pdp_sweep(X, cols, ppicks))
    assert _same(rows, X)                                           # nothing wrote into the handle
    for call in (lambda: s.shap(rows, picks), lambda: s.shap(X, picks)):
        with pytest.raises(NotImplementedError, match="pgb_predict_shap"):
            call()
    for call in (lambda: s.shap_interactions(rows, picks), lambda: s.shap_interactions(rows, picks, cols=[4, 1]),
                 lambda: s.shap_interactions(X, picks)):
        with pytest.raises(NotImplementedError, match="pgb_predict_shap_interactions"):
            call()


def test_on_the_oracle_the_sweep_helper_hands_the_matrix_back(samplers):
    from pymc_bart_amd.utils import _MultiChainSampler, _resident_rows, _sample_posterior

    s, _, X = samplers
    multi = _MultiChainSampler([s, s])
    rows = _resident_rows(multi, X)
    assert isinstance(rows, np.ndarray) and _same(rows, X)
    assert _same(_resident_rows([multi, multi], X), X)
    got = _sample_posterior(multi, rows, np.random.default_rng(3), size=5, excluded=[2])
    assert _same(got, _sample_posterior(multi, X, np.random.default_rng(3), size=5, excluded=[2]))
