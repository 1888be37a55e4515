"""Per-draw averages over rows on the MI355X: ``k_rowreduce`` and ``k_rowreduce_finish`` through ``pgb_row_reduce`` and
``pgb_row_reduce_finish`` against the host build of the same header (``tests/_rowreduce_host.py``) -- bit for bit, on
synthetic device matrices at every tile regime, group layout and argument variant, in one block and in successive
64-row blocks -- the refusals of the entry points, and the public calls of ``pymc_bart_amd.average`` on short real
chains.

"Bit for bit" is the 64-bit pattern of every output that is a number; a NaN on both sides counts as equal (the sign
and payload of a NaN an operation GENERATES are the hardware's, not the contract's)."""
import ctypes as C

import numpy as np
import pytest

import _rowreduce_host as host
from pymc_bart_amd import (BARTOp, CategoricalLikelihood, _abi, _stored, average_contrast, average_prediction, bayes_r2,
                           summarize_matrix)
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _get_posterior_sampler

pytestmark = pytest.mark.gpu

PAD = 7.0e77        # what the columns beyond nb hold: no result may show it
GUARD = -7.0        # what lies behind every output buffer


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)


def same(got, want) -> bool:
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


def groups(layout: str, n: int, G: int, rng) -> np.ndarray:
    if layout == "random":
        return rng.integers(0, G, n).astype(np.int32)
    if layout == "contiguous":                                  # boundaries inside the tiles, not at multiples of 64
        cuts = np.sort(rng.integers(0, n + 1, G - 1))
        return np.searchsorted(cuts, np.arange(n), side="right").astype(np.int32)
    if layout == "interleaved":                                 # the group changes at every row of every lane
        return (np.arange(n) % G).astype(np.int32)
    assert layout == "one lane class"                           # group G - 1 lives in rows 5, 69, 133, ... alone
    g = rng.integers(0, max(G - 1, 1), n).astype(np.int32)
    g[5::64] = G - 1
    return g


def inputs(n, D, K, G, layout, seed):
    rng = np.random.default_rng(seed)
    return {"a": rng.normal(0.0, 2.0, (D, K, n)), "b": rng.normal(0.0, 2.0, (D, K, n)), "w": rng.uniform(0.0, 3.0, n),
            "g": groups(layout, n, G, rng), "y": rng.normal(0.0, 2.0, n), "off_a": rng.normal(0.0, 1.0, (K, n)),
            "off_b": rng.normal(0.0, 1.0, (K, n)), "centre": rng.normal(0.0, 1.0, (K, G))}


def device(hip, a, w, g, G, b=None, y=None, off_a=None, off_b=None, centre=None, transform="identity", pad=0, chunk=None,
           v_mode="none"):
    """``pgb_row_reduce`` per block of ``chunk`` rows (``None``: one block) and ``pgb_row_reduce_finish`` on device
    copies of the arguments; the matrices get ``pad`` columns beyond the block's (``ld = nb + pad``).  ``v_mode``:
    "none", "separate" or "alias" (``v_out`` is ``a``).  -> what ``host.reduce`` returns (``v``: ``None`` without)."""
    mem, lib = hip.mem, hip.lib
    reduce_, finish, query = lib.rowreduce_entry_points()
    D, K, n = a.shape
    has_y = y is not None
    words = host.ws_doubles(D, K, G, has_y)
    assert query(D, K, G, int(has_y)) == 8 * words
    wsd = mem.from_host(np.full(words + 8, GUARD))
    ptr = lambda t: None if t is None else mem.ptr(t)  # noqa: E731
    up = lambda x: None if x is None else mem.from_host(np.ascontiguousarray(x))  # noqa: E731
    cd = up(centre)
    code = transform if isinstance(transform, int) else host.TRANSFORMS[transform]
    v = None if v_mode == "none" else np.empty((D, K, n))
    step = n if chunk is None else chunk
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        nb, ld = r1 - r0, r1 - r0 + pad

        def padded(m):
            full = np.full((D, K, ld), PAD)
            full[:, :, :nb] = m[:, :, r0:r1]
            return full

        ad, bd = mem.from_host(padded(a)), None if b is None else mem.from_host(padded(b))
        vd = {"none": None, "alias": ad, "separate": mem.from_host(np.full((D, K, ld), GUARD))}[v_mode]
        cut = lambda x: None if x is None else up(x[..., r0:r1])  # noqa: E731
        wd, gd, yd, oad, obd = cut(w), cut(g), cut(y), cut(off_a), cut(off_b)
        rc = reduce_(ptr(ad), ptr(bd), D, K, nb, ld, ptr(wd), ptr(gd), ptr(yd), ptr(oad), ptr(obd), ptr(cd), G, code, r0,
                     int(r0 == 0), ptr(wsd), ptr(vd), mem.stream_ptr)
        lib.check(rc, "pgb_row_reduce")
        if vd is not None:
            got = mem.to_host(vd)
            assert np.all(got[:, :, nb:] == (PAD if v_mode == "alias" else GUARD))   # nothing written beyond the block
            v[:, :, r0:r1] = got[:, :, :nb]
        if bd is not None:
            assert np.array_equal(mem.to_host(bd), padded(b))                          # (b is read only)
    n_out = 6 if has_y else 2
    od, wod = mem.from_host(np.full(n_out * D * K * G + 8, GUARD)), mem.from_host(np.full(G + 8, GUARD))
    counts = (C.c_int64 * 2)(-1, -1)
    rc = finish(ptr(wsd), D, K, G, int(has_y), ptr(cd), ptr(od), ptr(wod), counts, mem.stream_ptr)
    out, W, ws = mem.to_host(od), mem.to_host(wod), mem.to_host(wsd)
    assert np.all(out[-8:] == GUARD) and np.all(W[-8:] == GUARD) and np.all(ws[-8:] == GUARD)
    return {"rc": rc, "out": out[:-8].reshape(n_out, D, K, G), "W": W[:-8], "n_nonfinite": int(counts[0]),
            "n_bad_group": int(counts[1]), "v": v, "ws": ws[:-8]}


def check(hip, kw: dict, G: int, what, **dev_kw):
    want = host.reduce(kw["a"], kw["w"], kw["g"], G, **{k: kw.get(k) for k in ("b", "y", "off_a", "off_b", "centre")},
                       transform=kw.get("transform", "identity"))
    got = device(hip, kw["a"], kw["w"], kw["g"], G, **{k: kw.get(k) for k in ("b", "y", "off_a", "off_b", "centre")},
                 transform=kw.get("transform", "identity"), **dev_kw)
    assert got["rc"] == 0, what
    bad = [j for j in range(want["out"].shape[0]) if not same(got["out"][j], want["out"][j])]
    assert not bad, (what, "outputs that differ", bad)
    assert same(got["W"], want["W"]), what
    assert got["n_nonfinite"] == want["n_nonfinite"] and got["n_bad_group"] == want["n_bad_group"] == 0, what
    n_part = got["ws"].size - 2
    assert same(got["ws"][:n_part], want["ws"][:n_part]), (what, "partials")
    if got["v"] is not None:
        assert same(got["v"], want["v"]), (what, "v")
    return got


def pick(kw: dict, i: int, K: int) -> dict:
    """Argument variant ``i`` of the inputs: which optional arguments are given, and the transform."""
    out = {k: kw[k] for k in ("a", "w", "g")}
    out["transform"] = list(host.TRANSFORMS)[(i // 5) % 4]
    if i & 1:
        out["b"] = kw["b"]
        if i & 2:
            out["off_b"] = kw["off_b"]
    if i & 4:
        out["off_a"] = kw["off_a"]
    if i & 8:
        out["centre"] = kw["centre"]
    if K == 1 and (i // 3) & 1:
        out["y"] = kw["y"]
    return out


# ------------------------------------------------------------------ 1. every shape, every layout of the groups
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 200])
def test_device_equals_the_host_header_at_every_shape(n, hip):
    i = 0
    for D in (1, 2, 65):
        for K in (1, 2):
            for G in (1, 3, 70):
                for layout in ("random", "contiguous", "interleaved", "one lane class"):
                    kw = inputs(n, D, K, G, layout, seed=1000 * n + 10 * D + K + G)
                    i += 1
                    check(hip, pick(kw, i, K), G, (n, D, K, G, layout, i), pad=(0, 5)[i % 2],
                          v_mode=("none", "separate", "alias")[i % 3])


# ------------------------------------------------------------------ 2. every argument variant
@pytest.mark.parametrize("transform", list(host.TRANSFORMS))
def test_device_equals_the_host_header_for_every_argument_variant(transform, hip):
    n, D, G = 200, 2, 3
    for K in (1, 2):
        kw = inputs(n, D, K, G, "contiguous", seed=7 + K)
        for has_b in (False, True):
            for has_y in ((False, True) if K == 1 else (False,)):
                for has_off in (False, True):
                    for has_c in (False, True):
                        for v_mode in ("none", "separate", "alias"):
                            args = {k: kw[k] for k in ("a", "w", "g")}
                            args["transform"] = transform
                            if has_b:
                                args["b"] = kw["b"]
                            if has_y:
                                args["y"] = kw["y"]
                            if has_off:
                                args["off_a"] = kw["off_a"]
                                if has_b:
                                    args["off_b"] = kw["off_b"]
                            if has_c:
                                args["centre"] = kw["centre"]
                            check(hip, args, G, (transform, K, has_b, has_y, has_off, has_c, v_mode), pad=3 * has_c,
                                  v_mode=v_mode)


# ------------------------------------------------------------------ 3. one block, or successive blocks
@pytest.mark.parametrize("layout", ["random", "contiguous", "interleaved", "one lane class"])
def test_successive_blocks_give_the_bits_of_one_block(layout, hip):
    for n, D, K, G in ((200, 2, 1, 3), (129, 65, 2, 70), (333, 3, 1, 70)):
        kw = inputs(n, D, K, G, layout, seed=n + G)
        args = pick(kw, 15, K)                                    # b, both offsets, centres (K = 1: and y), probit
        one = check(hip, args, G, (layout, n, "one block"), v_mode="separate")
        for chunk in (64, 128):
            many = check(hip, args, G, (layout, n, chunk), chunk=chunk, v_mode="alias", pad=1)
            for key in ("out", "W", "ws", "v"):
                assert same(many[key], one[key]), (layout, n, chunk, key)
            assert many["n_nonfinite"] == one["n_nonfinite"]


def test_non_finite_terms_are_counted_on_the_device(hip):
    rng = np.random.default_rng(5)
    a = rng.normal(0, 1, (3, 2, 200))
    a[rng.random(a.shape) < 0.1] = 800.0                                # exp overflows
    kw = {"a": a, "b": a[:, :, ::-1].copy(), "w": rng.uniform(0, 2, 200), "g": groups("random", 200, 3, rng),
          "transform": "exp"}
    got = check(hip, kw, 3, "exp overflow", chunk=64)
    assert got["n_nonfinite"] == int(((a == 800.0) | (a[:, :, ::-1] == 800.0)).sum()) > 0


# ------------------------------------------------------------------ 4. refusals
def test_refusals_before_any_launch(hip):
    mem, lib = hip.mem, hip.lib
    reduce_, finish, query = lib.rowreduce_entry_points()
    D, K, nb, G = 4, 1, 128, 3
    words = host.ws_doubles(D, 2, G, True)
    ad, bd = mem.from_host(np.zeros((D, 2, nb))), mem.from_host(np.zeros((D, 2, nb)))
    wd, gd, yd = mem.from_host(np.ones(nb)), mem.from_host(np.zeros(nb, np.int32)), mem.from_host(np.zeros(nb))
    offd = mem.from_host(np.zeros((2, nb)))
    wsd, vd = mem.from_host(np.full(words, GUARD)), mem.from_host(np.full((D, 2, nb), GUARD))
    p = mem.ptr
    good = dict(a=p(ad), b=p(bd), D=D, K=K, nb=nb, ld=nb, w=p(wd), g=p(gd), y=p(yd), oa=None, ob=None, c=None, G=G, t=0, r0=64,
                init=1, ws=p(wsd), v=p(vd))
    cases = (({"D": 0}, "D and K must be >= 1"), ({"K": 0}, "D and K must be >= 1"), ({"nb": 0}, "nb must be >= 1"),
             ({"ld": nb - 1}, "ld >= nb"), ({"r0": 1}, "multiple of 64, got 1"), ({"r0": 65}, "multiple of 64"),
             ({"r0": -64}, "multiple of 64"), ({"G": 0}, r"groups must be in \[1, 4096\], got 0"),
             ({"G": host.max_groups() + 1}, "groups must be in"), ({"t": 4}, "unknown transform 4"),
             ({"t": -1}, "unknown transform"), ({"K": 2}, r"y takes one output \(K == 1\)"),
             ({"b": None, "ob": p(offd)}, "an offset of b without b"), ({"a": None}, "null argument"),
             ({"w": None}, "null argument"), ({"g": None}, "null argument"), ({"ws": None}, "null argument"))
    for change, msg in cases:
        k = dict(good, **change)
        rc = reduce_(k["a"], k["b"], k["D"], k["K"], k["nb"], k["ld"], k["w"], k["g"], k["y"], k["oa"], k["ob"], k["c"], k["G"],
                     k["t"], k["r0"], k["init"], k["ws"], k["v"], mem.stream_ptr)
        assert rc == -1, change                                          # PGB_E_INVALID
        with pytest.raises(_abi.PGBError, match=msg):
            lib.check(rc, "pgb_row_reduce")
        assert np.all(mem.to_host(wsd) == GUARD) and np.all(mem.to_host(vd) == GUARD), change   # nothing ran
    od, wod = mem.from_host(np.full(6 * D * 2 * G, GUARD)), mem.from_host(np.full(G, GUARD))
    counts = (C.c_int64 * 2)(-1, -1)
    for (fD, fK, fG, fy), msg in (((0, 1, G, 0), "D and K must be >= 1"), ((D, 0, G, 0), "D and K must be >= 1"),
                                  ((D, 1, 0, 0), "groups must be in"), ((D, 1, host.max_groups() + 1, 0), "groups must be in"),
                                  ((D, 2, G, 1), "y takes one output")):
        rc = finish(p(wsd), fD, fK, fG, fy, None, p(od), p(wod), counts, mem.stream_ptr)
        assert rc == -1, (fD, fK, fG, fy)
        with pytest.raises(_abi.PGBError, match=msg):
            lib.check(rc, "pgb_row_reduce_finish")
        assert np.all(mem.to_host(od) == GUARD) and np.all(mem.to_host(wod) == GUARD) and list(counts) == [-1, -1]
    assert query(0, 1, 1, 0) == 0 and query(1, 0, 1, 0) == 0 and query(1, 1, 0, 0) == 0
    assert query(1, 1, host.max_groups() + 1, 0) == 0 and query(1, 1, host.max_groups(), 1) == 8 * host.ws_doubles(1, 1, host.max_groups(), True)


def test_rows_without_a_group_add_nothing_and_the_finish_refuses_them(hip):
    rng = np.random.default_rng(8)
    a, w = rng.normal(0, 1, (2, 1, 130)), rng.uniform(0, 2, 130)
    g = groups("random", 130, 3, rng)
    g[[7, 99]] = (-1, 3)
    want = host.reduce(a, w, g, 3)
    got = device(hip, a, w, g, 3)
    assert got["rc"] == -1 and got["n_bad_group"] == want["n_bad_group"] == 2
    with pytest.raises(_abi.PGBError, match=r"2 rows have a group outside \[0, 3\)"):
        hip.lib.check(got["rc"], "pgb_row_reduce_finish")
    assert same(got["out"], want["out"]) and same(got["W"], want["W"])


# ------------------------------------------------------------------ 5. the public calls on short chains
N, P, M_TREES = 600, 4, 10
FLOOR = 1 << 16     # the floor of PGB_PW_BLOCK_BYTES: at N rows every call below takes several blocks there


@pytest.fixture
def several_blocks(monkeypatch):
    """Sets the knob to its floor and hands out the list of row-block lists the calls made from then on: the test
    asserts that every one of them has more than one block."""
    seen = []
    plain = _stored.row_blocks

    def recording(n, bytes_per_row, limit):
        seen.append(plain(n, bytes_per_row, limit))
        return seen[-1]

    def start():
        monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(FLOOR))
        monkeypatch.setattr(_stored, "row_blocks", recording)
        return seen

    yield start
    monkeypatch.undo()


def _data(seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, P))
    X[:, 3] = rng.integers(0, 2, N)                                   # the treatment column
    f = 2.0 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 1.5 * (X[:, 2] - 0.5) + X[:, 3]
    return rng, X, f


@pytest.fixture(scope="module")
def normal_fit(hip):
    """Two chains behind one sampler: 2 x 12 pooled draws."""
    rng, X, f = _data(41)
    y = f + rng.normal(0, 0.5, N)
    op = BARTOp(X, y, m=M_TREES)
    attach_history(op, [sample_chain(op, 8, 12, random_seed=2, chain=c, backend=hip, keep_draws=False) for c in (0, 1)])
    return X, y, _get_posterior_sampler(op, backend=hip)


@pytest.fixture(scope="module")
def two_output_fit(hip):
    """K = 2: a two-class softmax fit."""
    rng, X, f = _data(42)
    y = (f + rng.normal(0, 0.5, N) > 1.5).astype(np.float64)
    op = BARTOp(X, y, m=M_TREES)
    res = sample_chain(op, 8, 20, num_particles=10, random_seed=3, chain=0, backend=hip, keep_draws=False,
                       likelihood=CategoricalLikelihood(2))
    base, batches = res["history"]
    return X, PosteriorSampler.from_history(batches, base, M_TREES, 2, backend=hip)


KEYS = ("mean", "weight", "n_rows", "group_labels")


def _equal(got: dict, want: dict, keys=KEYS):
    for key in keys:
        assert np.shape(got[key]) == np.shape(want[key]), key
        if np.asarray(want[key]).dtype == np.float64:
            assert same(got[key], want[key]), key
        else:
            assert np.array_equal(got[key], want[key]), key
    assert got["n_draws"] == want["n_draws"] and got["n_nonfinite"] == want["n_nonfinite"]


@pytest.mark.parametrize("fit", ["normal_fit", "two_output_fit"])
def test_average_prediction_and_contrast_equal_the_header_on_the_posterior_matrix(fit, request, several_blocks):
    fx = request.getfixturevalue(fit)
    X, sampler = fx[0], fx[-1]
    K, D = sampler.n_outputs, sampler.n_draws
    everything = list(range(D))
    rng = np.random.default_rng(12)
    w = rng.uniform(0.0, 2.0, N)
    labels = np.array(["young", "mid", "old"])[np.minimum((X[:, 0] * 3).astype(int), 2)]
    off = rng.normal(0, 1, (K, N))
    pred = sampler.sample_posterior(X, everything, None)
    assert pred.shape == (D, K, N)
    X1, X0 = X.copy(), X.copy()
    X1[:, 3], X0[:, 3] = 1.0, 0.0
    p1, p0 = sampler.sample_posterior(X1, everything, None), sampler.sample_posterior(X0, everything, None)

    def both(draws=None):
        return (average_prediction(sampler, X, draws=draws),
                average_prediction(sampler, X, w, labels, draws=draws, transform="logistic", offset=off),
                average_contrast(sampler, X1, X0, w, labels, draws=draws),
                average_contrast(sampler, X1, X0, draws=draws, rows=True, transform="probit", offset_b=off,
                                 quantiles=[0.1, 0.9], hdi_prob=0.8))

    plain, full, ate, rows = both()
    assert plain["mean"].shape == (D, 1, K) and full["mean"].shape == (D, 3, K)
    assert list(full["group_labels"]) == ["mid", "old", "young"] and plain["weight"][0] == float(N)
    _equal(plain, host.public(pred))
    _equal(full, host.public(pred, w, labels, offset=off, transform="logistic"))
    _equal(ate, host.public(p1, w, labels, pred_b=p0))
    want = host.public(p1, pred_b=p0, offset_b=off, transform="probit")
    _equal(rows, want)
    # rows: summarize_matrix of the header's v
    sm = summarize_matrix(want["v"].reshape(D, K * N), quantiles=[0.1, 0.9], hdi_prob=0.8)
    for key in ("mean", "var", "sd", "quantiles", "hdi"):
        assert same(rows["rows"][key], np.moveaxis(sm[key].reshape(sm[key].shape[:-1] + (K, N)), -2, -1)), key
    assert rows["rows"]["n_draws"] == D and rows["rows"]["hdi_prob"] == 0.8
    assert np.all(average_contrast(sampler, X1, X1, w, labels)["mean"] == 0.0)
    # a subset of the draws and excluded covariates
    idx = [3, 3] + list(range(5, D, 2))
    sub = average_prediction(sampler, X, w, labels, draws=idx, excluded=[1])
    _equal(sub, host.public(sampler.sample_posterior(X, idx, [1]), w, labels))
    # several blocks: no bit changes.  (At the floor of the knob the partial sums of the three groups fit for ten
    # draws: 10 K 3 KiB; those of all draws are refused, as the refusals say.)
    ten = list(range(1, 20, 2))
    whole = both(ten)
    seen = several_blocks()
    _equal(average_prediction(sampler, X), plain)
    with pytest.raises(ValueError, match="partial sums of"):
        average_prediction(sampler, X, w, labels)
    blocked = both(ten)
    for one, many in zip(whole, blocked):
        _equal(many, one)
    for key in ("mean", "var", "quantiles", "hdi"):
        assert same(blocked[3]["rows"][key], whole[3]["rows"][key]), key
    assert len(seen) == 5 and all(len(blocks) > 1 and blocks[-1][1] == N for blocks in seen), seen


def test_bayes_r2_equals_the_header_and_the_numpy_formula(normal_fit, several_blocks):
    X, y, sampler = normal_fit
    D = sampler.n_draws
    rng = np.random.default_rng(13)
    w = rng.uniform(0.0, 2.0, N)
    labels = (X[:, 3] > 0).astype(int)
    pred = sampler.sample_posterior(X, list(range(D)), None)
    keys = ("r2", "mse", "rmse", "bias", "var_fit", "var_res", "weight", "n_rows", "group_labels")
    for kw in ({}, {"weights": w, "groups": labels}):
        got = bayes_r2(sampler, X, y, **kw)
        _equal(got, host.public(pred, kw.get("weights"), kw.get("groups"), y=y), keys)
        ww, gg = kw.get("weights", np.ones(N)), kw.get("groups", np.zeros(N, int))
        for gi in range(got["group_labels"].size):
            m = gg == gi
            v, W = pred[:, 0, m], ww[m].sum()
            E = lambda t: (ww[m] * t).sum(axis=-1) / W  # noqa: E731
            res = y[m] - v
            var_fit, var_res = E((v - E(v)[:, None]) ** 2), E((res - E(res)[:, None]) ** 2)
            # (the bias is a sum with cancellation: it is held to 1e-12 of the size of its terms, E|y - v|)
            for key, ref, scale in (("mse", E(res * res), None), ("rmse", np.sqrt(E(res * res)), None),
                                    ("bias", E(res), E(np.abs(res))), ("r2", var_fit / (var_fit + var_res), None)):
                rel = np.max(np.abs(got[key][:, gi] - ref) / np.abs(ref if scale is None else scale))
                print(f"{key} group {gi}: largest relative difference from NumPy {rel:.3e}")
                assert rel <= 1e-12, (key, gi, rel)
        assert np.all((got["r2"] > 0.0) & (got["r2"] < 1.0))
    ten = list(range(1, 20, 2))                                      # (their partial sums fit the knob's floor)
    whole = [bayes_r2(sampler, X, y, draws=ten, **kw) for kw in ({}, {"weights": w, "groups": labels})]
    seen = several_blocks()
    for one, kw in zip(whole, ({}, {"weights": w, "groups": labels})):
        _equal(bayes_r2(sampler, X, y, draws=ten, **kw), one, keys)
    assert len(seen) == 2 and all(len(blocks) > 1 and blocks[-1][1] == N for blocks in seen), seen
