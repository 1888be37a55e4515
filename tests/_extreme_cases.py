"""Sampler cases at the ends of the double range (tests/test_extremes.py, tests/test_extremes_gpu.py).

Every case is n = 1025 rows (two chunks of 1024, a single row in the second), p = 4, m = 8 trees, 8 particles, 12 steps.
A case is a BASE design matrix at benign magnitudes and TWINS of it that the sampler must not be able to tell from the
base: order-preserving (continuous rule) or injective (one-hot rule) recodings of the covariates onto ladders of extreme
doubles, power-of-two rescalings of a regressed column, power-of-two rescalings of the response.
"""
import numpy as np

from pymc_bart_amd.sampler import PyBartSettings, PySampler

N, P_COLS, M, PARTICLES, STEPS = 1025, 4, 8, 8, 12
DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)      # smallest normal double
DENORM_MIN = 5e-324
LADDERS = ("adjacent", "f32_overflow", "f32_underflow", "full")
SIX_LEVELS = np.array([-np.inf, -DBL_MAX, -DENORM_MIN, DENORM_MIN, DBL_MAX, np.inf])
# an injective, NOT monotone recoding of the codes 0..5 of a one-hot column (only equality may matter)
ONEHOT_RECODE = np.array([np.inf, -np.inf, -0.0, DENORM_MIN, 1.0 + 2.0 ** -52, 1.0])


def _positive_rungs(h):
    """h increasing positive doubles that reach both ends of the range: the specials first, decades in between."""
    special = [np.inf, DENORM_MIN, DBL_MAX, DBL_MIN, 1e-310][:h]
    middle = np.logspace(-300.0, 300.0, h - len(special)).tolist() if h > len(special) else []
    return np.array(sorted(special + middle), np.float64)


def ladder(kind, k):
    """k strictly increasing doubles.
    "adjacent": 1 + i 2^-52 -- neighbouring doubles, ONE float32;
    "f32_overflow": all beyond +-1e39, both signs -- +-inf as float32;
    "f32_underflow": all within +-1e-50, both signs -- +-0 as float32;
    "full": -inf, -DBL_MAX, ..., -DBL_MIN, -1e-310, -5e-324, 5e-324, ..., DBL_MAX, +inf."""
    k = int(k)
    hn, hp = k // 2, k - k // 2
    if kind == "adjacent":
        out = 1.0 + np.arange(k, dtype=np.float64) * 2.0 ** -52
    elif kind == "f32_overflow":
        out = np.concatenate([-np.logspace(39.5, 300.0, hn)[::-1], np.logspace(39.5, 300.0, hp)])
    elif kind == "f32_underflow":
        out = np.concatenate([-np.logspace(-300.0, -50.5, hn)[::-1], np.logspace(-300.0, -50.5, hp)])
    elif kind == "full":
        out = np.concatenate([-_positive_rungs(hn)[::-1], _positive_rungs(hp)])
    else:
        raise ValueError(kind)
    out = np.asarray(out, np.float64)
    assert out.shape == (k,) and np.all(np.diff(out) > 0), (kind, k)   # (inf - DBL_MAX = inf > 0; no inf - inf: one per end)
    return out


def remap(X, kinds):
    """Per column j with kinds[j] not None: the i-th smallest distinct non-NaN value becomes the i-th rung of
    ladder(kinds[j], number of distinct values) -- or of kinds[j] itself when it is an array (any injective table).
    NaN stays NaN.  Returns (the new matrix, {j: (distinct values, rungs)}); `map_values` maps split values."""
    Xt = np.array(X, np.float64, copy=True)
    maps = {}
    for j, kind in enumerate(kinds):
        if kind is None:
            continue
        col = Xt[:, j]
        ok = ~np.isnan(col)
        vals = np.unique(col[ok])
        rungs = ladder(kind, len(vals)) if isinstance(kind, str) else np.asarray(kind, np.float64)
        assert rungs.shape == vals.shape, (j, rungs.shape, vals.shape)
        new = rungs[np.searchsorted(vals, col[ok])]
        assert len(np.unique(new)) == len(vals), j          # no two values merged
        col[ok] = new
        maps[j] = (vals, rungs)
    return Xt, maps


def map_values(maps, var, split):
    """The split values `split` (on the columns `var`) of a base chain, mapped like the data were."""
    var, out = np.asarray(var), np.array(split, np.float64, copy=True)
    for j, (vals, rungs) in maps.items():
        at = var == j
        idx = np.searchsorted(vals, out[at])
        assert np.array_equal(vals[idx], out[at]), j        # a split value is a value of its column
        out[at] = rungs[idx]
    return out


def _base(seed, code_col):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, P_COLS))
    X[rng.random(N) < 0.1, 2] = np.nan
    code = rng.integers(0, 6, N)
    if code_col:
        X[:, 3] = code
    return rng, X, code


def _case(name, X, Y, **kw):
    c = dict(name=name, X=X, Y=Y, family="normal", K=1, response="constant", rules=np.zeros(P_COLS, np.int32), seed=77,
             sigma=0.3, range_exp=None)
    c.update(kw)
    return c


def ladder_case():
    """Four continuous columns: two of 1025 distinct normals, one with 10 % NaN, one rounded (about nine levels with
    hundreds of ties each -- a ladder of nine rungs)."""
    rng, X, _ = _base(4, False)
    X[:, 3] = np.round(X[:, 3])
    Y = np.sin(X[:, 0]) + 0.5 * X[:, 1] + 0.4 * np.nan_to_num(X[:, 2]) + 0.3 * X[:, 3] + rng.normal(0, 0.3, N)
    return _case("ladder", X, Y)


def six_level_case():
    """Column 3: a code 0..5 under the continuous rule, with steps of the response at codes 1, 3 and 5; its twin holds
    the six levels {-inf, -DBL_MAX, -5e-324, 5e-324, DBL_MAX, +inf}: the steps are splits at -inf, -5e-324, DBL_MAX."""
    rng, X, code = _base(6, True)
    Y = np.sin(X[:, 0]) + 1.5 * (code >= 1) - 1.0 * (code >= 3) + 0.8 * (code >= 5) + rng.normal(0, 0.3, N)
    return _case("six_level", X, Y)


def six_level_twin(c):
    return remap(c["X"], [None, None, None, SIX_LEVELS])


def onehot_case():
    """Column 3: the same code under the one-hot rule, an effect per category."""
    rng, X, code = _base(8, True)
    Y = np.sin(X[:, 0]) + np.array([-1.5, 0.0, 1.0, -0.5, 2.0, 0.5])[code] + rng.normal(0, 0.3, N)
    return _case("onehot", X, Y, rules=np.array([0, 0, 0, 1], np.int32))


def onehot_twin(c):
    return remap(c["X"], [None, None, None, ONEHOT_RECODE])


def signed_zero_twin(c, j=3):
    """Every second member of column j's zero group becomes -0.0 (equal to 0.0 in every comparison)."""
    Xt = c["X"].copy()
    zeros = np.flatnonzero(Xt[:, j] == 0.0)
    assert len(zeros) >= 100
    Xt[zeros[1::2], j] = -0.0
    assert np.signbit(Xt[:, j]).sum() > np.signbit(c["X"][:, j]).sum()
    return Xt


def with_family(c, family):
    """The case under another likelihood: "bernoulli_probit" (the response cut at its mean) or "categorical" (K = 3:
    the response cut at its terciles)."""
    c = dict(c)
    if family == "bernoulli_probit":
        c.update(family=family, Y=(c["Y"] > c["Y"].mean()).astype(float))
    elif family == "categorical":
        c.update(family=family, K=3, Y=np.digitize(c["Y"], np.quantile(c["Y"], [1 / 3, 2 / 3])).astype(float))
    else:
        assert family == "normal", family
    return c


def linear_case(response="linear", family="normal"):
    """Column 0 carries a broken line: leaves that regress on it have slopes that matter."""
    rng = np.random.default_rng(10)
    X = rng.normal(size=(N, P_COLS))
    X[rng.random(N) < 0.1, 2] = np.nan
    Y = np.where(X[:, 0] < 0, 2 * X[:, 0] + 1, -1.5 * X[:, 0] + 1) + 0.5 * X[:, 1] + rng.normal(0, 0.2, N)
    return with_family(_case(f"{response}-{family}", X, Y, response=response, sigma=0.2), family)


def scale_column(X, j, k):
    """Column j times 2^k (exact while no value leaves the normal range)."""
    Xt = X.copy()
    Xt[:, j] = np.ldexp(X[:, j], k)
    assert np.array_equal(np.ldexp(Xt[:, j], -k), X[:, j], equal_nan=True)
    return Xt


def scale_response(c, k, range_exp=None):
    """The Normal case with Y 2^k, sigma 2^k and range_exp + k (or the range_exp given, the data scaled to it)."""
    base = settings(c).range_exp
    if range_exp is not None:
        k = int(range_exp) - base
    c = dict(c)
    c.update(Y=np.ldexp(c["Y"], k), sigma=float(np.ldexp(c["sigma"], k)), range_exp=base + k, k=k)
    return c


def settings(c, X=None):
    X = c["X"] if X is None else X
    return PyBartSettings.from_data(X, c["Y"], m=M, num_particles=c.get("P", PARTICLES), seed=c["seed"], batch=(0.5, 0.5),
                                    family=c["family"], n_outputs=c["K"], response=c["response"], range_exp=c["range_exp"])


def run_chain(c, backend, X=None, stepper=None):
    """The case's 12 steps (6 of them tuning) on `backend`, on the design matrix X (default: the base).  Per step:
    sum_trees, the accepted trees and the counters.  `stepper(s, tune) -> sum_trees`: another stepping entry point."""
    X = c["X"] if X is None else X
    st = settings(c, X)
    s = PySampler(st, X, c["Y"], c["rules"], np.ones(P_COLS), backend=backend)
    s.set_likelihood([c["sigma"]] if c["family"] == "normal" else [])
    sums, steps, ctrs = [], [], []
    for it in range(STEPS):
        sums.append(np.array(s.step(it < STEPS // 2)[0] if stepper is None else stepper(s, it < STEPS // 2)))
        steps.append(s.export_trees(0).decoded())
        ctr = s.counters.as_dict()
        ctr.pop("slots")                       # (backend-specific)
        ctrs.append(ctr)
    trees = steps + [s.export_trees(1).decoded()]
    cat = {f: np.concatenate([np.asarray(getattr(t, f)).ravel() for t in trees]) for f in ("var", "split", "count", "value")}
    if c["response"] != "constant":
        K = c["K"]
        cat["svar"] = np.concatenate([np.asarray(t.svar) for t in trees])
        cat["xbar"] = np.concatenate([np.asarray(t.xbar) for t in trees])
        cat["slope"] = np.concatenate([np.asarray(t.slope).reshape(-1, K) for t in trees])
    return dict(sum_trees=np.array(sums), counters=ctrs, state=s.state(), settings=st, sampler=s, **cat)


def inner_splits(res):
    """(column, split value) of every inner node the run accepted."""
    at = res["var"] >= 0
    return res["var"][at], res["split"][at]


def assert_alive(res):
    """The chain has moved: the sampler had something to get wrong."""
    last = res["sum_trees"][-1]
    assert np.std(last if last.ndim == 1 else last[0]) > 0.2


def assert_same_chain(base, twin, maps, what, equal_splits=False):
    """The twin chain IS the base chain: sum_trees of every step bit for bit, the same trees, the same row counts, the
    same leaf values, the split values mapped like the data (`equal_splits`: comparing equal, signs of zero aside)."""
    assert np.array_equal(base["sum_trees"], twin["sum_trees"]), what
    assert np.array_equal(base["var"], twin["var"]) and np.array_equal(base["count"], twin["count"]), what
    assert np.array_equal(base["value"], twin["value"]), what
    var, split = inner_splits(base)
    tsplit = inner_splits(twin)[1]
    if equal_splits:
        assert np.all(split == tsplit), what
    else:
        want = map_values(maps, var, split)
        assert np.array_equal(want, tsplit) and np.array_equal(np.signbit(want), np.signbit(tsplit)), what
    assert base["counters"] == twin["counters"], what


def assert_splits_on(res, cols, what):
    var, _ = inner_splits(res)
    for j in cols:
        assert np.any(var == j), f"{what}: no accepted split on column {j}"


def assert_same_run(a, b, what):
    """Two backends on the same data: per step sum_trees and counters, every exported array bit for bit."""
    assert np.array_equal(a["sum_trees"], b["sum_trees"], equal_nan=True), what
    assert a["counters"] == b["counters"], what
    for f in ("var", "split", "count", "value", "svar", "xbar", "slope"):
        if f in a:
            x, y = np.asarray(a[f]), np.asarray(b[f])
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, f)
    assert np.array_equal(a["state"]["leaf_sd"], b["state"]["leaf_sd"]), what


def slopes_on(res, j):
    """Slopes (all outputs) and xbar of the leaves that regress on column j."""
    at = res["svar"] == j
    return res["slope"][at], res["xbar"][at]
