"""An exact reference of the prediction walk, written from its contract alone (``test_predict_edges_gpu.py``).

``walk`` runs every row through every tree of a ``TreeArrays`` pool in ``fractions.Fraction`` -- no rounding anywhere --
and shares no code with ``trees.predict_numpy``, the oracle or the product.  The contract:

* a split on an excluded variable, or on a value that is NaN, takes BOTH subtrees, weighted ``cl / (cl + cr)`` and
  ``cr / (cl + cr)`` by the training counts of the two children; when ``cl + cr == 0`` nothing is added;
* continuous rule: left when ``x <= v``; one-hot rule: left when ``x == v``; subset rule: left when bit ``code(x)`` of
  the mask ``v`` is set, ``code`` being 0 for ``x <= 0``, ``trunc(x)`` below 51 and 51 from 51 on;
* a leaf adds ``value + slope * (x[svar] - xbar)``; an excluded or NaN regressor (or ``svar < 0``) gives ``value``.

Per (forest, output, row) the result holds the exact sum ``R``, the magnitude ``S = sum |w| (|value| + |slope| |x -
xbar|)`` over the leaves reached, the number ``T`` of those leaves and the most marginalised levels ``L`` on one path.

Two ways to hold a device result against it:

* ``exact_class``: asserts -- in ``Fraction`` arithmetic alone -- that every quantity the walk can form (the count
  ratios, every product of them along a path, ``x - xbar``, ``slope * (x - xbar)``, the leaf value, the weighted leaf
  value) is a multiple of one power of two ``g`` and that ``S`` and all of them lie below ``2^53 g``.  Every partial sum
  of the terms, in any order, is then a multiple of ``g`` below ``2^53 g``, i.e. a double: no operation of any
  implementation rounds, and the device must return ``float(R)`` with tolerance 0.
* ``bound_ratio``: arbitrary data.  The walk of ``pgb_pred_walk.h`` computes a term as ``w * (value + slope * (x -
  xbar))`` with ``w`` a product of ``L`` quotients ``c / (cl + cr)`` (the sum of two counts is exact below 2^53, which
  ``walk`` asserts): 2 roundings per level, 4 for the leaf and its weighting, and at most ``T`` additions on the way
  into the accumulator -- ``N = 2 L + 4 + T`` factors ``(1 + d)``, ``|d| <= u = 2^-53``, on every term, hence
  ``|device - R| <= gamma_N S`` with ``gamma_N = N u / (1 - N u)`` (Higham, Accuracy and Stability of Numerical
  Algorithms, lemma 3.1).  Nothing in it is measured.  (The data stay far from overflow and underflow.)

The builders (``Leaf``, ``Split``, ``build_pool``, ``dyadic_tree``, ``complete_tree``, ``chain_tree``) make hand-built
pools: nodes in breadth-first order, children after their parent, as both samplers store them.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from pymc_bart_amd import _abi
from pymc_bart_amd.trees import TreeArrays

U = Fraction(1, 2 ** 53)
CONT, ONEHOT, SUBSET = _abi.RULE_CONTINUOUS, _abi.RULE_ONEHOT, _abi.RULE_SUBSET


# ------------------------------------------------------------------ the walk
def _goes_left(rule: int, x: float, v: float) -> bool:
    """``x`` is not NaN.  An infinity has no Fraction: it is ordered as the extended reals order it."""
    if rule == CONT:
        if math.isinf(x) or math.isinf(v):
            return x == v or x == -math.inf or v == math.inf
        return Fraction(x) <= Fraction(v)
    if rule == ONEHOT:
        if math.isinf(x) or math.isinf(v):
            return x == v
        return Fraction(x) == Fraction(v)
    assert rule == SUBSET, rule
    if x <= 0.0:
        code = 0
    elif x >= 51.0:
        code = 51
    else:
        code = int(Fraction(x))  # truncation towards zero of a positive value
    mask = int(Fraction(v))
    return bool((mask >> code) & 1)


@dataclass
class _Reach:
    """What one row reaches in one tree."""
    leaves: list = field(default_factory=list)   # (weight, node, regressor difference or None)
    levels: int = 0                              # most marginalised levels on one path
    parts: list = field(default_factory=list)    # every intermediate quantity of the weights (ratios, prefix products)


def _reach(pool: TreeArrays, t: int, x: np.ndarray, excl: set) -> _Reach:
    base = int(pool.node_off[t])
    out = _Reach()
    todo = [(0, Fraction(1), 0)]  # (tree-local node, weight, marginalised levels so far), left first
    steps = 0
    while todo:
        k, w, lv = todo.pop()
        while True:
            steps += 1
            assert steps <= 1 << 20, "the walk does not end: the pool is not made of trees"
            g = base + k
            j = int(pool.var[g])
            if j < 0:
                break
            xv = float(x[j])
            if j in excl or math.isnan(xv):
                l, r = int(pool.left[g]), int(pool.right[g])
                cl, cr = int(pool.count[base + l]), int(pool.count[base + r])
                assert 0 <= cl and 0 <= cr and cl + cr < 2 ** 53, "counts whose sum a double does not hold"
                if cl + cr == 0:
                    k = -1
                    break
                fl, fr = Fraction(cl, cl + cr), Fraction(cr, cl + cr)
                out.parts += [fl, fr, w * fl, w * fr]
                todo.append((r, w * fr, lv + 1))
                k, w, lv = l, w * fl, lv + 1
                continue
            k = int(pool.left[g]) if _goes_left(int(pool.rule[g]), xv, float(pool.split[g])) else int(pool.right[g])
        if k < 0:
            continue
        g = base + k
        js = int(pool.svar[g])
        diff = None
        if js >= 0 and js not in excl and js < x.shape[0] and not math.isnan(float(x[js])):
            assert math.isfinite(float(x[js])), "a regressor must be finite"
            diff = Fraction(float(x[js])) - Fraction(float(pool.xbar[g]))
        out.leaves.append((w, g, diff))
        out.levels = max(out.levels, lv)
    return out


class Exact:
    """The result of :func:`walk`: object arrays of ``Fraction`` (``R``, ``S``: (D, K, n)), ``T`` and ``L`` (D, n)."""

    def __init__(self, R, S, T, L, parts):
        self.R, self.S, self.T, self.L = R, S, T, L
        self._parts = parts  # per (D, n): every intermediate quantity of that entry's terms

    def exact_class(self) -> np.ndarray:
        """``float(R)`` (D, K, n) after asserting that no operation of any implementation can round."""
        D, K, n = self.R.shape
        out = np.empty((D, K, n))
        most_bits = 0
        for d in range(D):
            for i in range(n):
                parts = [q for q in self._parts[d][i] if q != 0]
                g = Fraction(1)
                for q in parts:
                    den = q.denominator
                    assert den & (den - 1) == 0, f"not dyadic: {q} (forest {d}, row {i})"
                    g = min(g, Fraction(1, den))
                top = max([abs(q) for q in parts] + [self.S[d, o, i] for o in range(K)] + [Fraction(0)])
                assert top < 2 ** 53 * g, f"{top} needs more than 53 bits at granularity {g} (forest {d}, row {i})"
                if top:
                    most_bits = max(most_bits, (top / g).numerator.bit_length())
                for o in range(K):
                    out[d, o, i] = float(self.R[d, o, i])
                    assert Fraction(out[d, o, i]) == self.R[d, o, i]
        self.most_bits = most_bits
        return out

    def bound_ratio(self, got: np.ndarray) -> float:
        """max over the entries of ``|got - R| / (gamma_N S)`` (0 / 0 counts as 0; anything / 0 as infinity)."""
        D, K, n = self.R.shape
        got = np.asarray(got, np.float64).reshape(D, K, n)
        assert np.all(np.isfinite(got))
        worst = Fraction(0)
        for d in range(D):
            for i in range(n):
                N = 2 * int(self.L[d, i]) + 4 + int(self.T[d, i])
                gamma = N * U / (1 - N * U)
                for o in range(K):
                    err = abs(Fraction(float(got[d, o, i])) - self.R[d, o, i])
                    bound = gamma * self.S[d, o, i]
                    if err == 0:
                        continue
                    if bound == 0:
                        return math.inf
                    worst = max(worst, err / bound)
        return float(worst)


def walk(pool: TreeArrays, forest_idx, X, excluded=()) -> Exact:
    X = np.asarray(X, np.float64)
    n, p = X.shape
    fidx = np.asarray(forest_idx)
    D, m = fidx.shape
    K = int(pool.n_outputs)
    excl = {int(e) for e in excluded if 0 <= int(e) < p}
    value = np.asarray(pool.value, np.float64).reshape(-1, K)
    slope = np.asarray(pool.slope, np.float64).reshape(-1, K)
    cache = {}

    def tree_row(t, i):
        key = (t, i)
        if key not in cache:
            rc = _reach(pool, t, X[i], excl)
            R = [Fraction(0)] * K
            S = [Fraction(0)] * K
            parts = list(rc.parts)
            for w, g, diff in rc.leaves:
                if diff is not None:
                    parts.append(diff)
                for o in range(K):
                    v = Fraction(float(value[g, o]))
                    a = abs(v)
                    if diff is not None:
                        sl = Fraction(float(slope[g, o])) * diff
                        parts.append(sl)
                        v, a = v + sl, a + abs(sl)
                    parts += [v, w * v]
                    R[o] += w * v
                    S[o] += w * a
            cache[key] = (R, S, len(rc.leaves), rc.levels, parts)
        return cache[key]

    R = np.empty((D, K, n), object)
    S = np.empty((D, K, n), object)
    T = np.zeros((D, n), np.int64)
    L = np.zeros((D, n), np.int64)
    parts = [[None] * n for _ in range(D)]
    for d in range(D):
        for i in range(n):
            r, s, pt = [Fraction(0)] * K, [Fraction(0)] * K, []
            for t in fidx[d]:
                tr, ts, nt, lv, tp = tree_row(int(t), i)
                r = [a + b for a, b in zip(r, tr)]
                s = [a + b for a, b in zip(s, ts)]
                T[d, i] += nt
                L[d, i] = max(L[d, i], lv)
                pt = pt + tp
            for o in range(K):
                R[d, o, i], S[d, o, i] = r[o], s[o]
            parts[d][i] = pt
    return Exact(R, S, T, L, parts)


# ------------------------------------------------------------------ builders
@dataclass
class Leaf:
    value: object                 # K numbers
    count: int = 8
    svar: int = -1
    slope: object = None          # K numbers
    xbar: float = 0.0


@dataclass
class Split:
    var: int
    split: float
    left: object
    right: object
    rule: int = CONT
    count: int = 8


def build_pool(roots: list, K: int, order: str = "bfs") -> TreeArrays:
    """The trees in breadth-first order (``order="reversed"``: the same trees with every non-root node stored in
    reverse, children BEFORE their parents -- a valid tree that only the general walk takes)."""
    flat = []
    for root in roots:
        nodes, links = [root], []
        k = 0
        while k < len(nodes):
            nd = nodes[k]
            if isinstance(nd, Split):
                links.append((k, len(nodes), len(nodes) + 1))
                nodes += [nd.left, nd.right]
            k += 1
        nn = len(nodes)
        pos = list(range(nn)) if order == "bfs" else [0] + list(range(nn - 1, 0, -1))
        flat.append((nodes, {k: (pos[l], pos[r]) for k, l, r in links}, pos))
    total = sum(len(nodes) for nodes, _, _ in flat)
    pool = TreeArrays.empty(len(flat), total, K)
    base = 0
    for t, (nodes, links, pos) in enumerate(flat):
        pool.tree_id[t] = t
        pool.node_off[t] = base
        for k, nd in enumerate(nodes):
            g = base + pos[k]
            pool.count[g] = nd.count
            if isinstance(nd, Split):
                pool.var[g], pool.split[g], pool.rule[g] = nd.var, nd.split, nd.rule
                pool.left[g], pool.right[g] = links[k]
            else:
                pool.var[g] = -1
                pool.value[g] = np.broadcast_to(np.asarray(nd.value, np.float64), (K,))
                if nd.svar >= 0:
                    pool.svar[g], pool.xbar[g] = nd.svar, nd.xbar
                    pool.slope[g] = np.broadcast_to(np.asarray(nd.slope, np.float64), (K,))
        base += len(nodes)
    pool.node_off[len(flat)] = base
    return pool


def dyadic(rng, bits: int, bound: float, size=None):
    """Multiples of 2^-bits in [-bound, bound]."""
    q = 2 ** bits
    return rng.integers(-int(bound * q), int(bound * q) + 1, size=size) / q


def pair_counts(rng, kind: str = "dyadic"):
    """The training counts of two siblings.  ``dyadic``: ratios to their sum that are multiples of 1/8;
    ``free``: anything."""
    if kind == "dyadic":
        a, c = int(rng.integers(1, 8)), int(rng.integers(1, 40))
        return a * c, (8 - a) * c
    assert kind == "free", kind
    return int(rng.integers(1, 1000)), int(rng.integers(1, 1000))


def dyadic_leaf(rng, K: int, linear=(), free: bool = False) -> Leaf:
    """Leaf values that are multiples of 2^-10 within +-8; two thirds of the leaves regress on one of ``linear`` with
    slopes and xbar that are multiples of 2^-4 within +-2 (``free``: normal deviates)."""
    lf = Leaf(rng.normal(size=K) if free else dyadic(rng, 10, 8.0, K))
    if len(linear) and rng.random() < 2 / 3:
        lf.svar = int(rng.choice(linear))
        lf.slope = rng.normal(size=K) if free else dyadic(rng, 4, 2.0, K)
        lf.xbar = float(rng.normal()) if free else float(dyadic(rng, 4, 2.0))
    return lf


def dyadic_tree(rng, K: int, depth: int, cols, split_of, grow: float = 0.75, linear=(), counts: str = "dyadic",
                rules=None, level: int = 0):
    """A random tree of at most ``depth`` levels that splits on ``cols``; ``split_of(rng, column)`` gives a split
    value; ``rules`` maps a column to its rule (default continuous)."""
    if level >= depth or (level > 0 and rng.random() > grow):
        return dyadic_leaf(rng, K, linear, free=counts == "free")
    j = int(rng.choice(cols))
    nd = Split(j, float(split_of(rng, j)), None, None, rule=(rules or {}).get(j, CONT))
    nd.left = dyadic_tree(rng, K, depth, cols, split_of, grow, linear, counts, rules, level + 1)
    nd.right = dyadic_tree(rng, K, depth, cols, split_of, grow, linear, counts, rules, level + 1)
    nd.left.count, nd.right.count = pair_counts(rng, counts)
    return nd


def complete_tree(rng, K: int, depth: int, cols, split_of, linear=(), counts: str = "dyadic", level: int = 0):
    """Every leaf at ``depth``; level ``l`` splits on ``cols[l % len(cols)]``."""
    if level == depth:
        return dyadic_leaf(rng, K, linear, free=counts == "free")
    j = int(cols[level % len(cols)])
    nd = Split(j, float(split_of(rng, j)), complete_tree(rng, K, depth, cols, split_of, linear, counts, level + 1),
               complete_tree(rng, K, depth, cols, split_of, linear, counts, level + 1))
    nd.left.count, nd.right.count = pair_counts(rng, counts)
    return nd


def chain_tree(rng, K: int, depth: int, cols, split_of, side: str, linear=(), counts: str = "dyadic"):
    """``depth`` splits in a row, each with one leaf child: ``side="left"`` continues on the left."""
    nd = dyadic_leaf(rng, K, linear, free=counts == "free")
    for level in range(depth - 1, -1, -1):
        j = int(cols[level % len(cols)])
        other = dyadic_leaf(rng, K, linear, free=counts == "free")
        a, b = pair_counts(rng, counts)
        nd.count, other.count = a, b
        nd = Split(j, float(split_of(rng, j)), nd, other) if side == "left" else Split(j, float(split_of(rng, j)), other, nd)
    return nd


def tree_depth(pool: TreeArrays, t: int) -> int:
    base = int(pool.node_off[t])
    best, todo = 0, [(0, 0)]
    while todo:
        k, d = todo.pop()
        best = max(best, d)
        if pool.var[base + k] >= 0:
            todo += [(int(pool.left[base + k]), d + 1), (int(pool.right[base + k]), d + 1)]
    return best
