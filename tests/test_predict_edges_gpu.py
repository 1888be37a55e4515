"""The prediction walk (``pred_walk_forest`` in ``k_predict``, ``k_pointwise`` and ``k_ice``) at its edges, against an
exact reference.

Every case of ``pgb_predict`` makes three assertions (``check``):

1. the device against ``tests/_predict_exact.py`` -- a ``fractions.Fraction`` walk written from the contract: with
   tolerance 0 on pools of the exact class (no operation of any implementation can round; the reference asserts that),
   within the derived bound ``gamma_N S`` otherwise (the largest ``error / bound`` is printed);
2. the device against the oracle backend's ``pgb_predict`` on the same pool: bit for bit;
3. where no variable is excluded and every rule is continuous: the same rows with a NaN in a column that no tree
   splits or regresses on -- which sends their whole wave from the fixed-length walk to the general one -- give the
   same bits (the general walk adds ``1.0 * v``).

The launches go through the C entry points directly, so that the leading dimensions are the test's to choose; the
padding holds a value no result may show.  Shapes are the smallest that reach the path: the ``Fraction`` walk is the
slow side."""
import ctypes as C

import numpy as np
import pytest

import _pointwise_host as pw_host
import _predict_exact as E
from _ice_host import random_pool
from pymc_bart_amd import _abi
from pymc_bart_amd.trees import TreeArrays

pytestmark = pytest.mark.gpu

POISON = 7.0e77      # in the padding of a strided matrix
GUARD = -7.0         # behind every output
MAX_DEPTH = 64       # PGB_MAX_DEPTH (include/pgbart_spec.h)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.delenv("PGB_PRED_WGS", raising=False)
    monkeypatch.delenv("PGB_PW_WGS", raising=False)


# ------------------------------------------------------------------ launches
def strided(X, ld):
    X = np.ascontiguousarray(X, np.float64)
    if ld is None or ld == X.shape[1]:
        return X
    a = np.full((X.shape[0], ld), POISON)
    a[:, :X.shape[1]] = X
    return a


def predict(be, pool, fidx, X, excluded=(), ldx=None):
    """``pgb_predict`` of backend ``be`` (the product or the oracle) -> (D, K, n); ``ldx``: the leading dimension."""
    X = np.ascontiguousarray(X, np.float64)
    n, p = X.shape
    fidx = np.ascontiguousarray(fidx, np.int32)
    D, m = fidx.shape
    K = int(pool.n_outputs)
    a = strided(X, ldx)
    excl = np.ascontiguousarray(list(excluded), np.int32)
    xd = be.mem.from_host(a)
    od = be.mem.from_host(np.full(D * K * n + 8, GUARD))
    carr = pool.as_c()
    rc = be.lib.lib.pgb_predict(C.byref(carr), fidx.ctypes.data, D, m, be.mem.ptr(xd), n, p, a.shape[1],
                                excl.ctypes.data if excl.size else None, int(excl.size), be.mem.ptr(od),
                                be.mem.stream_ptr)
    be.lib.check(rc, "pgb_predict")
    out = be.mem.to_host(od)
    assert np.all(out[D * K * n:] == GUARD)                   # nothing written beyond [D][K][n]
    return out[:D * K * n].reshape(D, K, n)


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def continuous(pool) -> bool:
    return bool(np.all(np.asarray(pool.rule)[np.asarray(pool.var) >= 0] == E.CONT))


def check(hip, oracle, pool, fidx, X, excluded=(), exact=True, ldx=None, spare=None, ref=None, what=None):
    """The three assertions of one ``pgb_predict`` case -> (the device's result, the reference).  ``spare``: a column
    no tree uses; ``ref``: the reference when an earlier call made it (same pool, forests, rows and exclusions)."""
    ref = E.walk(pool, fidx, X, excluded) if ref is None else ref
    got = predict(hip, pool, fidx, X, excluded, ldx)
    if exact:
        want = ref.exact_class()
        assert same_bits(got, want), (what, "device != exact reference", np.argwhere(got != want)[:5])
    else:
        ratio = ref.bound_ratio(got)
        print(f"{what}: max error / bound = {ratio:.3g}")
        assert ratio <= 1.0, (what, ratio)
    assert same_bits(got, predict(oracle, pool, fidx, X, excluded, ldx)), (what, "device != oracle")
    if spare is not None and not len(excluded) and continuous(pool) and not np.any(np.isnan(X[:, spare])):
        used = set(np.asarray(pool.var)[np.asarray(pool.var) >= 0].tolist()) | \
            set(np.asarray(pool.svar)[np.asarray(pool.svar) >= 0].tolist())
        assert spare not in used
        Xn = np.array(X, np.float64)
        Xn[::37, spare] = np.nan                             # (37 < 64: every wave holds one)
        assert same_bits(predict(hip, pool, fidx, Xn, excluded, ldx), got), (what, "general walk != fixed-length walk")
    return got, ref


# ------------------------------------------------------------------ data
def split_q(rng, j):
    """Split values that are multiples of 1/4 within +-2: rows drawn by ``rows_q`` hit them exactly now and then."""
    return E.dyadic(rng, 2, 2.0)


def rows_q(rng, n, p):
    """Rows of multiples of 2^-4 within +-2.5."""
    return E.dyadic(rng, 4, 2.5, (n, p))


def forests(rng, n_trees, D, m):
    return np.stack([rng.choice(n_trees, size=m, replace=m > n_trees) for _ in range(D)]).astype(np.int32)


def mixed_pool(rng, K, cols, linear, n_trees=20, counts="dyadic"):
    """Trees of depth 0 .. 6: a group of four walks rarely holds four of one depth."""
    roots = [E.dyadic_tree(rng, K, int(rng.integers(0, 7)), cols, split_q, 0.8, linear, counts) for _ in range(n_trees)]
    return E.build_pool(roots, K)


# ------------------------------------------------------------------ rows and launch geometry
_GEOMETRY = {}


def _geometry_case(n):
    """One pool, forest table, rows and reference per row count, shared by the launch geometries."""
    if n not in _GEOMETRY:
        rng = np.random.default_rng(100 + n)
        pool = mixed_pool(rng, 2, cols=[0, 1, 2], linear=[3])
        fidx = forests(rng, pool.n_trees, 7, 12)
        X = rows_q(rng, n, 5)                                # column 4: spare
        if n > 64:
            X[64 + (n - 65) // 2, 1] = np.nan                # the second wave marginalises, the first stays clean
        _GEOMETRY[n] = (pool, fidx, X, E.walk(pool, fidx, X))
    return _GEOMETRY[n]


@pytest.mark.parametrize("wgs", [None, "one", "three"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_every_row_count_under_every_forest_stride(n, wgs, hip, oracle, monkeypatch):
    """7 forests: a grid row per forest (the default at this size), ONE workgroup row that walks all 7 on the rows
    it staged once, and 3 workgroup rows (forests 0 3 6 / 1 4 / 2 5)."""
    pool, fidx, X, ref = _geometry_case(n)
    gx = -(-n // 64)
    if wgs is not None:                                       # gy = min(ceil(PGB_PRED_WGS / gx), 7)
        monkeypatch.setenv("PGB_PRED_WGS", str(1 if wgs == "one" else 3 * gx))
    check(hip, oracle, pool, fidx, X, spare=4, ref=ref, what=(n, wgs))


# ------------------------------------------------------------------ layout
def wide_pool(rng, p, K=1):
    """Splits on the columns 0, 125 and p - 1, leaves that regress on 125 and p - 1 (column 1 stays unused)."""
    cols = sorted({0, min(125, p - 1), p - 1})
    roots = [E.dyadic_tree(rng, K, int(rng.integers(1, 5)), cols, split_q, 0.8, cols[1:] if p > 1 else [0])
             for _ in range(10)]
    return E.build_pool(roots, K)


def wide_case(p, n=70, D=3, m=5, K=1):
    rng = np.random.default_rng(200 + p)
    pool = wide_pool(rng, p, K)
    used = set(np.asarray(pool.var).tolist())
    assert used >= {0, p - 1} and (p < 126 or 125 in used)
    fidx = forests(rng, pool.n_trees, D, m)
    X = rows_q(rng, n, p)
    return pool, fidx, X


@pytest.mark.parametrize("p", [1, 5, 126, 127])
def test_every_width_contiguous_and_strided(p, hip, oracle):
    """p = 126 is the last width staged in LDS, 127 the first read from global memory; ldx = p + 3 takes the strided
    staging branch (p <= 126) and the strided global reads."""
    pool, fidx, X = wide_case(p)
    spare = 1 if p > 2 else None
    got, ref = check(hip, oracle, pool, fidx, X, spare=spare, what=(p, "contiguous"))
    got3, _ = check(hip, oracle, pool, fidx, X, ldx=p + 3, spare=spare, ref=ref, what=(p, "ldx = p + 3"))
    assert same_bits(got, got3)
    Xn = X.copy()                                             # ... and through the general walk of both stagings
    Xn[5, 0] = Xn[66, p - 1] = np.nan
    refn = E.walk(pool, fidx, Xn)
    check(hip, oracle, pool, fidx, Xn, ref=refn, what=(p, "NaN, contiguous"))
    check(hip, oracle, pool, fidx, Xn, ldx=p + 3, ref=refn, what=(p, "NaN, ldx = p + 3"))


# ------------------------------------------------------------------ the group walk
def sized_tree(rng, K, kind, cols, linear=(), counts="dyadic"):
    """The trees at the limits of the walks: ``complete7`` (255 nodes: the largest the fixed-length walk takes, child
    index 254 in a byte), ``over`` (257 nodes: the general walk), ``left64`` / ``right64`` (chains of PGB_MAX_DEPTH)."""
    if kind == "complete7":
        return E.complete_tree(rng, K, 7, cols, split_q, linear, counts)
    if kind == "over":
        root = E.complete_tree(rng, K, 7, cols, split_q, linear, counts)
        nd = root
        while isinstance(nd.right, E.Split):
            nd = nd.right
        nd.right = E.Split(int(cols[0]), float(split_q(rng, 0)), E.dyadic_leaf(rng, K, linear, counts == "free"),
                           E.dyadic_leaf(rng, K, linear, counts == "free"), count=nd.right.count)
        nd.right.left.count, nd.right.right.count = E.pair_counts(rng, counts)
        return root
    assert kind in ("left64", "right64"), kind
    return E.chain_tree(rng, K, MAX_DEPTH, cols, split_q, kind[:-2], linear, counts)


def test_the_sized_trees_are_what_they_claim():
    rng = np.random.default_rng(1)
    pool = E.build_pool([sized_tree(rng, 1, k, [0, 1]) for k in ("complete7", "over", "left64", "right64")], 1)
    assert np.diff(pool.node_off).tolist() == [255, 257, 129, 129]
    assert [E.tree_depth(pool, t) for t in range(4)] == [7, 8, MAX_DEPTH, MAX_DEPTH]
    assert pool.right[:255].max() == 254                      # the last child index a byte must hold


_GROUP = {}


def _group_pool():
    """Trees 0 .. 3 have the depths 0, 1, 7 and 64; then the other chain, the 257-node tree, a tree stored children
    first (valid, but only the general walk takes it) and ten of depth 0 .. 6."""
    if not _GROUP:
        rng = np.random.default_rng(300)
        K, cols, lin = 1, [0, 1, 2], [3]
        roots = [E.dyadic_leaf(rng, K), E.dyadic_tree(rng, K, 1, cols, split_q, 1.0, lin),
                 sized_tree(rng, K, "complete7", cols, lin), sized_tree(rng, K, "left64", cols, lin),
                 sized_tree(rng, K, "right64", cols, lin), sized_tree(rng, K, "over", cols, lin)]
        roots += [E.dyadic_tree(rng, K, int(rng.integers(0, 7)), cols, split_q, 0.8, lin) for _ in range(10)]
        pool = E.build_pool(roots, K)
        rev = E.build_pool([E.dyadic_tree(rng, K, 4, cols, split_q, 0.9, lin)], K, order="reversed")
        _GROUP["pool"] = TreeArrays.concat([pool, rev])
        _GROUP["X"] = rows_q(rng, 70, 5)
    return _GROUP["pool"], _GROUP["X"]


@pytest.mark.parametrize("m", [1, 3, 4, 5, 8, 9, 12])
def test_the_group_walk_at_every_forest_size(m, hip, oracle):
    """m < 4 never forms a group; 5 and 9 leave a tail of one; a group of the depths {0, 1, 7, 64} walks 64 steps with
    three walks idling on their leaves; the 257-node tree and the children-first tree break a group up."""
    pool, X = _group_pool()
    rng = np.random.default_rng(310 + m)
    n_trees = pool.n_trees
    table = [list(range(n_trees))[:m],                       # depths 0, 1, 7, 64 first
             [3, 2, 1, 0, 4, 6, 7, 8, 5, 9, 10, 16][:m],     # (5: 257 nodes; 16: children first)
             [16, 5, 0, 1, 2, 3, 4, 6, 7, 8, 9, 10][:m]]
    table += forests(rng, n_trees, 4, m).tolist()
    check(hip, oracle, pool, np.asarray(table, np.int32), X, spare=4, what=m)


def test_a_marginalising_tree_at_every_position_of_a_forest_of_twelve(hip, oracle):
    """Forest k holds the one tree that splits on the excluded column at position k: a general walk inside groups
    whose roots were requested ahead, before, between and after full groups."""
    rng = np.random.default_rng(320)
    K, m = 2, 12
    plain = [E.dyadic_tree(rng, K, int(rng.integers(1, 5)), [0, 1, 2], split_q, 0.8, [4]) for _ in range(m - 1)]
    odd = E.dyadic_tree(rng, K, 3, [0, 1, 2], split_q, 1.0, [4])
    odd.var = odd.left.var = 3                                # two marginalised levels
    pool = E.build_pool(plain + [odd], K)
    fidx = np.empty((m, m), np.int32)
    for k in range(m):
        row = list(range(m - 1))
        row.insert(k, m - 1)
        fidx[k] = row
    X = rows_q(rng, 65, 6)                                    # no NaN: the waves are clean
    got, _ = check(hip, oracle, pool, fidx, X, excluded=[3], what="excluded column 3")
    assert not same_bits(got, predict(hip, pool, fidx, X))    # (the exclusion is not a no-op)
    for k in range(1, m):                                     # exact sums: the position changes no bit
        assert same_bits(got[k], got[0])


# ------------------------------------------------------------------ tree sizes
@pytest.mark.parametrize("mode", ["clean", "nan", "all excluded"])
@pytest.mark.parametrize("kind", ["complete7", "over", "left64", "right64"])
def test_the_largest_and_deepest_trees(kind, mode, hip, oracle):
    """Forests of five trees of one kind (a group of four and one more).  Clean rows: the exact class.  A NaN in
    column 0 marginalises every fourth level; every variable excluded marginalises all of them -- 64 entries of the
    walk's stack for the chains, whose weights no double holds exactly: those cases are held to the bound."""
    rng = np.random.default_rng(400 + ["complete7", "over", "left64", "right64"].index(kind))
    K, p = 1, 6
    chain = kind.endswith("64")
    exact = mode == "clean" or not chain
    counts = "dyadic" if exact else "free"
    cols = [0, 1, 2, 3]
    roots = [sized_tree(rng, K, kind, cols, [4], counts) for _ in range(6)]
    if mode == "all excluded" and not chain:                  # 7 or 8 levels of eighths and 2^-10 leaves: halves
        for root in roots:
            todo = [root]
            while todo:
                nd = todo.pop()
                if isinstance(nd, E.Split):
                    nd.left.count = nd.right.count = 16
                    todo += [nd.left, nd.right]
    pool = E.build_pool(roots, K)
    fidx = forests(rng, 6, 3, 5)
    n = 65 if mode != "all excluded" else 3                   # (every row of an all-excluded walk reaches every leaf)
    X = rows_q(rng, n, p)
    if mode == "nan":
        X[::3, 0] = np.nan
    excluded = list(range(p)) if mode == "all excluded" else []
    _, ref = check(hip, oracle, pool, fidx, X, excluded=excluded, exact=exact, spare=5, what=(kind, mode))
    if mode == "all excluded":
        assert int(ref.L.max()) == E.tree_depth(pool, 0) and (not chain or int(ref.L.max()) == MAX_DEPTH)


# ------------------------------------------------------------------ values
def value_pool(rng, K=1):
    """Splits at +0.0, -0.0, 1.5, -2.25 and +-inf on the columns 0 .. 2, leaves that regress on column 3."""
    values = [0.0, -0.0, 1.5, -2.25, np.inf, -np.inf]

    def split_of(rng, j):
        return values[int(rng.integers(0, len(values)))]

    roots = [E.dyadic_tree(rng, K, int(rng.integers(1, 6)), [0, 1, 2], split_of, 0.85, [3]) for _ in range(16)]
    pool = E.build_pool(roots, K)
    assert {float(v) for v in pool.split[pool.var >= 0]} >= {0.0, 1.5, -2.25, np.inf, -np.inf}
    assert np.any(np.signbit(pool.split[pool.var >= 0]) & (pool.split[pool.var >= 0] == 0.0))
    return pool


def value_rows(rng, n):
    """The split columns hold every split value, its two neighbours, both zeros and both infinities."""
    edge = []
    for v in (0.0, -0.0, 1.5, -2.25):
        edge += [v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)]
    edge += [np.inf, -np.inf]
    X = rows_q(rng, n, 5)
    X[:, :3] = rng.choice(edge, size=(n, 3))
    return X


@pytest.mark.parametrize("nan_rows", ["none", "lane 0", "lane 63", "last wave", "every lane"])
def test_values_at_and_next_to_the_splits_and_where_the_missing_values_sit(nan_rows, hip, oracle):
    rng = np.random.default_rng(500)
    pool = value_pool(rng)
    fidx = forests(rng, pool.n_trees, 4, 8)
    n = 130                                                   # two full waves and a wave of two rows
    X = value_rows(rng, n)
    where = {"none": [], "lane 0": [0, 64], "lane 63": [63, 127], "last wave": [129], "every lane": list(range(n))}
    for i in where[nan_rows]:
        X[i, i % 3] = np.nan
    check(hip, oracle, pool, fidx, X, spare=4, what=nan_rows)


# ------------------------------------------------------------------ rules
@pytest.mark.parametrize("p", [4, 130])
def test_one_hot_and_subset_rules(p, hip, oracle):
    """One-hot splits at v met by v, v + 0.5 and -v; subset masks with bit 0, bit 51 and all 52 bits met by codes
    below, at and beyond both ends; NaN on the rule columns.  (p = 130: the instance without the LDS tile.)"""
    rng = np.random.default_rng(600)
    K = 2
    masks = [1.0, float(2 ** 51), float(2 ** 52 - 1), float(2 ** 51 + 1), float(0b101010), float(2 ** 50)]
    rules = {0: E.ONEHOT, 1: E.SUBSET}

    def split_of(rng, j):
        if j == 0:
            return float(rng.choice([2.0, 3.0, 0.0]))
        if j == 1:
            return masks[int(rng.integers(0, len(masks)))]
        return split_q(rng, j)

    roots = [E.dyadic_tree(rng, K, int(rng.integers(1, 5)), [0, 1, 2], split_of, 0.85, [3], rules=rules)
             for _ in range(16)]
    roots[0].var, roots[0].rule, roots[0].split = 0, E.ONEHOT, 2.0       # (every rule at a root at least once)
    roots[1].var, roots[1].rule, roots[1].split = 1, E.SUBSET, masks[1]
    roots[2].var, roots[2].rule, roots[2].split = 1, E.SUBSET, masks[2]
    pool = E.build_pool(roots, K)
    fidx = forests(rng, pool.n_trees, 3, 9)
    onehot = [2.0, 2.5, -2.0, 3.0, 3.5, -3.0, 0.0, -0.0, 0.5, np.nan]
    subset = [-3.0, 0.0, 0.5, 50.9, 51.0, 52.0, 1e9, 1.0, 3.0, 5.0, 50.0, np.inf, -np.inf, np.nan]
    n = len(onehot) * len(subset)                            # 140 rows: every pair
    X = np.zeros((n, p))
    X[:, :4] = rows_q(rng, n, 4)
    X[:, 0] = np.repeat(onehot, len(subset))
    X[:, 1] = np.tile(subset, len(onehot))
    check(hip, oracle, pool, fidx, X, what=("rules", p))
    check(hip, oracle, pool, fidx, X, excluded=[1], what=("rules, subset column excluded", p))


# ------------------------------------------------------------------ excluded variables
@pytest.mark.parametrize("excluded", [[], [1], [0, 1, 2, 3, 4], [3], [7], [5, 9, -1], [1, 1, 2, 1]],
                         ids=["none", "one split variable", "all", "the regressor", "beyond p", "beyond p and negative",
                              "duplicates"])
def test_excluded_variables(excluded, hip, oracle):
    rng = np.random.default_rng(700)
    pool = mixed_pool(rng, 2, cols=[0, 1, 2], linear=[3])
    fidx = forests(rng, pool.n_trees, 3, 9)
    X = rows_q(rng, 65, 5)
    X[7, 2] = X[64, 3] = np.nan
    got, _ = check(hip, oracle, pool, fidx, X, excluded=excluded, what=excluded)
    plain = predict(hip, pool, fidx, X)
    effective = {e for e in excluded if 0 <= e < 5}
    assert same_bits(got, plain) == (not effective)
    if excluded == [1, 1, 2, 1]:
        assert same_bits(got, predict(hip, pool, fidx, X, [2, 1]))


# ------------------------------------------------------------------ leaves
@pytest.mark.parametrize("K", [1, 3, 16])
def test_leaves_of_every_width_linear_leaves_and_empty_children(K, hip, oracle):
    """Linear leaves with a finite, a NaN and an excluded regressor; under marginalisation a pair of children that
    both hold no training row (nothing is added) and pairs with one empty side (weights 0 and 1)."""
    rng = np.random.default_rng(800 + K)
    roots = [E.dyadic_tree(rng, K, int(rng.integers(1, 5)), [0, 1, 2], split_q, 0.85, [3]) for _ in range(12)]
    for root, (cl, cr) in zip(roots, [(0, 0), (0, 8), (8, 0), (0, 0)]):
        root.var = 0
        root.left.count, root.right.count = cl, cr
    lin = E.Leaf(E.dyadic(rng, 10, 8.0, K), svar=3, slope=E.dyadic(rng, 4, 2.0, K), xbar=0.25)
    roots.append(lin)                                         # a stump that is a linear leaf
    pool = E.build_pool(roots, K)
    assert np.any(np.asarray(pool.svar) >= 0)
    fidx = np.vstack([np.array([[0, 1, 2, 3, 12, 4, 5, 6, 7]], np.int32), forests(rng, 13, 2, 9)])
    X = rows_q(rng, 65, 5)
    X[::5, 0] = np.nan                                        # the roots with empty children marginalise
    X[::7, 3] = np.nan                                        # a missing regressor
    got, _ = check(hip, oracle, pool, fidx, X, what=("leaves", K))
    got_x, _ = check(hip, oracle, pool, fidx, X, excluded=[3], what=("leaves, regressor excluded", K))
    assert not same_bits(got, got_x)
    Xc = rows_q(rng, 65, 5)                                   # clean rows: linear leaves at the end of fixed-length walks
    check(hip, oracle, pool, fidx, Xc, spare=4, what=("leaves, clean", K))


# ------------------------------------------------------------------ the bounded class
@pytest.mark.parametrize("case", ["deep chains", "bushy", "rules"])
def test_arbitrary_pools_stay_within_the_derived_bound(case, hip, oracle):
    """Normal deviates for values, slopes and rows, arbitrary counts, depth up to 12, NaNs and an excluded column."""
    rng = np.random.default_rng(900)
    p = 6
    if case == "rules":
        rules = [0, 1, 2, 0, 0, 0]
        pool = random_pool(rng, 24, p, K=2, depth=6, rules=rules, linear=[4])
    else:
        rules = None
        pool = random_pool(rng, 24, p, K=2, depth=12, linear=[4], split_cols=[0, 1, 2, 3], chain=case == "deep chains")
    fidx = forests(rng, 24, 5, 12)
    n = 40
    X = rng.normal(size=(n, p))
    if rules is not None:
        X[:, 1] = rng.integers(0, 4, n)
        X[:, 2] = rng.integers(0, 8, n)
    X[rng.random(n) < 0.2, 0] = np.nan
    X[rng.random(n) < 0.1, 4] = np.nan
    for excluded in ([], [1], [0, 1, 2, 3]):
        check(hip, oracle, pool, fidx, X, excluded=excluded, exact=False, spare=5, what=(case, excluded))


# ------------------------------------------------------------------ the other kernels of the walk at the same edges
def pointwise(hip, pool, fidx, X, y, sigma, ldx=None, family="normal", clamped=None):
    """``pgb_pointwise_loglik`` (matrix output) -> (D, n).  ``sigma``: the Normal family's parameter per draw -- for
    another built-in ``family`` its parameters ``(D, n_params)``.  ``clamped``: a list that takes the count of clamped
    entries in place of the assertion that there is none."""
    X = np.ascontiguousarray(X, np.float64)
    n, p = X.shape
    fidx = np.ascontiguousarray(fidx, np.int32)
    D, m = fidx.shape
    a = strided(X, ldx)
    mem, lib = hip.mem, hip.lib
    xd, yd = mem.from_host(a), mem.from_host(np.ascontiguousarray(y, np.float64))
    od = mem.from_host(np.full(D * n + 8, GUARD))
    sigma = np.ascontiguousarray(sigma, np.float64)
    lik = _abi.PointwiseLik()
    lik.family, lik.n_params, lik.y_dev = _abi.FAMILIES[family], sigma.size // D, mem.ptr(yd)
    lik.params_host = sigma.ctypes.data if sigma.size else None
    carr = pool.as_c()
    nc = C.c_int64(0)
    rc = lib.pointwise_entry_point()(C.byref(carr), fidx.ctypes.data, D, m, mem.ptr(xd), n, p, a.shape[1], C.byref(lik),
                                     mem.ptr(od), None, C.byref(nc), mem.stream_ptr)
    lib.check(rc, "pgb_pointwise_loglik")
    out = mem.to_host(od)
    assert np.all(out[D * n:] == GUARD)
    if clamped is None:
        assert nc.value == 0
    else:
        clamped.append(int(nc.value))
    return out[:D * n].reshape(D, n)


def check_pointwise(hip, pool, fidx, X, what):
    rng = np.random.default_rng(7)
    n = X.shape[0]
    D = fidx.shape[0]
    y = rng.normal(size=n)
    sigma = rng.uniform(0.5, 2.0, D)
    mu = predict(hip, pool, fidx, X)                         # k_predict, held to the exact reference above
    assert pool.n_outputs == 1
    want = np.stack([pw_host.logpdf("normal", y, mu[d], [sigma[d]]) for d in range(D)])
    p = X.shape[1]
    got = pointwise(hip, pool, fidx, X, y, sigma)
    assert same_bits(got, want), (what, "contiguous")
    assert same_bits(pointwise(hip, pool, fidx, X, y, sigma, ldx=p + 3), got), (what, "ldx = p + 3")


@pytest.mark.parametrize("p", [126, 127])
def test_pointwise_at_the_lds_boundary_contiguous_and_strided(p, hip):
    pool, fidx, X = wide_case(p)
    check_pointwise(hip, pool, fidx, X, (p, "clean"))
    X[5, 0] = X[66, p - 1] = np.nan
    check_pointwise(hip, pool, fidx, X, (p, "NaN"))


@pytest.mark.parametrize("nan_rows", ["lane 0", "lane 63", "last wave", "every lane"])
def test_pointwise_where_the_missing_values_sit(nan_rows, hip):
    rng = np.random.default_rng(500)
    pool = value_pool(rng)
    fidx = forests(rng, pool.n_trees, 4, 8)
    n = 130
    X = value_rows(rng, n)
    where = {"lane 0": [0, 64], "lane 63": [63, 127], "last wave": [129], "every lane": list(range(n))}
    for i in where[nan_rows]:
        X[i, i % 3] = np.nan
    check_pointwise(hip, pool, fidx, X, nan_rows)


def ice(hip, pool, fidx, X, inst, cols, picks, ldx=None, ldi=None):
    """``pgb_predict_ice`` -> (n_cols, n_inst, K, n)."""
    X = np.ascontiguousarray(X, np.float64)
    n, p = X.shape
    fidx = np.ascontiguousarray(fidx, np.int32)
    D, m = fidx.shape
    K = int(pool.n_outputs)
    a, b = strided(X, ldx), strided(inst, ldi)
    cols = np.ascontiguousarray(cols, np.int32)
    picks = np.ascontiguousarray(picks, np.int32)
    n_cols, n_inst, n_picks = picks.shape
    mem, lib = hip.mem, hip.lib
    xd, idev = mem.from_host(a), mem.from_host(b)
    size = n_cols * n_inst * K * n
    od = mem.from_host(np.full(size + 8, GUARD))
    carr = pool.as_c()
    rc = lib.ice_entry_point()(C.byref(carr), fidx.ctypes.data, D, m, mem.ptr(xd), n, p, a.shape[1], mem.ptr(idev),
                               n_inst, b.shape[1], cols.ctypes.data, n_cols, picks.ctypes.data, n_picks, mem.ptr(od),
                               mem.stream_ptr)
    lib.check(rc, "pgb_predict_ice")
    out = mem.to_host(od)
    assert np.all(out[size:] == GUARD)
    return out[:size].reshape(n_cols, n_inst, K, n)


def test_ice_with_strided_rows_and_strided_instances(hip):
    """ldx = p + 3 and ldi = p + 2 in one call: the bits of the contiguous call, which are those of k_predict on the
    probe rows (exact sums: the mean over the picks of an exact-class pool is a sum of doubles divided once)."""
    rng = np.random.default_rng(1000)
    p, K = 5, 2
    pool = mixed_pool(rng, K, cols=[0, 1, 2], linear=[3])
    fidx = forests(rng, pool.n_trees, 6, 9)
    X = rows_q(rng, 70, p)
    X[3, 1] = np.nan
    inst = rows_q(rng, 3, p)
    inst[1, 2] = np.nan
    cols = [1, 3, 0]
    picks = rng.integers(0, 6, (3, 3, 4))
    got = ice(hip, pool, fidx, X, inst, cols, picks)
    assert same_bits(ice(hip, pool, fidx, X, inst, cols, picks, ldx=p + 3, ldi=p + 2), got)
    for c, j in enumerate(cols):                             # ... and the contiguous call against k_predict
        for r in range(3):
            probe = np.tile(inst[r], (70, 1))
            probe[:, j] = X[:, j]
            mu = predict(hip, pool, fidx[picks[c, r]], probe)
            total = mu[0].copy()
            for s in range(1, 4):
                total = total + mu[s]
            assert same_bits(got[c, r], total / 4.0), (c, r)
