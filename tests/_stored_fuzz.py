"""Seeded fuzz of the stored-draw entry points: one generator that draws every dimension of a call at once, and one
runner per entry point that lays the device call out as that entry point's GPU module does and holds it to that entry
point's host reference, bit for bit (``tests/test_stored_fuzz.py``, ``tests/test_stored_fuzz_gpu.py``,
``tools/fuzz_hunt.py --stored``).

``random_walk_case(seed)`` is deterministic in ``seed``.  Up to ``COVER`` it picks the index of every dimension from the
seed by a covering rule, beyond it at random:

* the four dimensions whose pairs the suite must cover -- ``p`` at or below / above ``PRED_LDS_MAXP``, all-continuous /
  mixed rules, rows without / with a NaN, ``K = 1`` / ``K > 1`` -- take the cell ``seed % 16`` and, inside their half,
  the value ``rank % len``, ``rank`` counting the earlier seeds of the same half;
* every other dimension takes ``(seed * prime + seed // stride + shift) % len`` with a prime of its own that does not
  divide ``len`` and one of ten strides, so that dimensions of one length do not move together.

A case holds what was drawn (``case["dims"]``, the names of the issue's lists) and what it means (the pool, the forest
table, the picks, the rows ...).  Where two draws cannot both hold -- a column no tree uses at ``p = 1``, sixteen arm
columns at ``p = 5`` -- the case records what it took instead under ``case["took"]``; the coverage test counts ``took``.

Every history is passed through the oracle's ``pgb_validate_forest`` (a one-row ``pgb_predict``) when it is generated.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

import _predict_exact as E
from pymc_bart_amd import _abi
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(path: str, name: str) -> int:
    text = open(os.path.join(ROOT, path)).read()
    return int(re.search(rf"#define {name} \(?(\d+)", text).group(1))


LDS_MAXP = _define("pymc_bart_amd/csrc/pgb_pred_walk.h", "PRED_LDS_MAXP")
MAX_DEPTH = _abi.MAX_DEPTH
SHAPX_MAX_U = _define("include/pgbart_shap_interaction.h", "PGB_SHAPX_MAX_U")
SHAP_MAX_U = MAX_DEPTH + 1            # PGB_SHAP_MAX_U, and PGB_HSTAT_MAX_U with it
ALE_MAX_BINS = _define("include/pgbart_ale.h", "PGB_ALE_MAX_BINS")
ARMS_MAX = _define("include/pgbart_arms.h", "PGB_ARMS_MAX")
ARMS_MAX_COLS = _define("include/pgbart_arms.h", "PGB_ARMS_MAX_COLS")
SURV_MAX_LEVELS = _define("include/pgbart_surv.h", "PGB_SURV_MAX_LEVELS")
ONEHOT, SUBSET = _abi.RULE_ONEHOT, _abi.RULE_SUBSET
POISON = 7.0e77                       # the padding of a leading dimension: no result may show it
FAMILIES = ("normal", "bernoulli_probit", "bernoulli_logit", "poisson_log", "negbin_log", "asymmetric_laplace",
            "student_t", "gamma_log", "categorical", "normal_meanscale")

P_BELOW = (1, 2, 5, 64, 65, LDS_MAXP - 1, LDS_MAXP)
P_ABOVE = (LDS_MAXP + 1, LDS_MAXP + 4)
K_MANY = (2, 3, 4, 5, 16)
DATA_CLEAN = ("clean", "split-neighbours", "signed-zero", "inf", "unseen-codes")
DATA_NAN = ("nan-0.05", "nan-lane-0", "nan-lane-63", "nan-last-tile", "nan-column")
# the issue's lists, by name; "p", "K", "data" and "rules" are the four of the cells
DIMS = {
    "p": P_BELOW + P_ABOVE, "K": (1,) + K_MANY, "data": DATA_CLEAN + DATA_NAN, "rules": ("continuous", "mixed"),
    "nb": (1, 2, 63, 64, 65, 127, 128, 129, 200), "first_row": (0, 64, 192), "tail": (0, 1, 70), "pad": (0, 1, 3),
    "m": (1, 3, 4, 5, 8, 9, 12), "D": (1, 2, 3, 7), "extra": ("0", "2", "m"), "picks": ("identity", "subset", "repeat"),
    "leaves": ("constant", "linear-used", "linear-unused", "linear-excluded"), "excluded": ("none", "one-used", "all"),
    "cols": ("one", "all", "unused"), "R": (1, 3), "bins": (1, 2, 40), "arms": (1, 2, 5), "arm_cols": (1, 2, ARMS_MAX_COLS),
    "J": (1, 2, 50), "levels": (0, 1, SURV_MAX_LEVELS), "pairs": ("none", "one", "all"),
    "route": ("direct", "profile", "auto"), "ice": ("strided", "contiguous"), "family": FAMILIES,
}
TOOK_DIMS = dict(DIMS, cols_few=DIMS["cols"])   # (what a case took in place of a draw, by the draw's list)
SHAPES = ("stump", "depth-1", "bushy", "complete-255", "left-64", "right-64", "children-first")
_FREE = [k for k in DIMS if k not in ("p", "K", "data", "rules")]
_PRIMES = dict(zip(_FREE, (11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97)))
assert len(_PRIMES) == len(_FREE) and all(_PRIMES[k] % len(DIMS[k]) for k in _FREE)
_STRIDES = (16, 3, 9, 5, 7, 2, 11, 4, 13, 6)
COVER = 64                            # seeds below it follow the covering rule
SUITE_SEEDS = tuple(range(32))        # what the suite runs (tests/test_stored_fuzz.py holds them to the coverage)
ONCE_MAX_BINS, ONCE_MAX_ARMS = 5, 11  # seed % 32: PGB_ALE_MAX_BINS / PGB_ARMS_MAX in place of the drawn count


def _cell(seed: int):
    """The four bits of a covering seed and its rank inside each half."""
    c = seed % 16
    bits = {"p": c & 1, "rules": (c >> 1) & 1, "data": (c >> 2) & 1, "K": (c >> 3) & 1}
    shift = {"p": 0, "rules": 1, "data": 2, "K": 3}
    rank = {}
    for k, s in shift.items():
        within = sum(1 for e in range(c) if ((e >> s) & 1) == bits[k])
        rank[k] = (seed // 16) * 8 + within
    return bits, rank


def _draw_dims(seed: int, rng) -> dict:
    d = {}
    if seed < COVER:
        bits, rank = _cell(seed)
        d["p"] = (P_ABOVE if bits["p"] else P_BELOW)[(rank["p"] + seed // 16) % (2 if bits["p"] else len(P_BELOW))]
        d["rules"] = DIMS["rules"][bits["rules"]]
        d["data"] = (DATA_NAN if bits["data"] else DATA_CLEAN)[(rank["data"] + seed // 32) % 5]
        d["K"] = 1 if not bits["K"] else K_MANY[rank["K"] % len(K_MANY)]
        for i, k in enumerate(_FREE):                                   # (the strides: lists of one length do not move together)
            d[k] = DIMS[k][(seed * _PRIMES[k] + seed // _STRIDES[i % len(_STRIDES)] + i) % len(DIMS[k])]
    else:
        for k, v in DIMS.items():
            d[k] = v[int(rng.integers(0, len(v)))]
    return d


# ------------------------------------------------------------------ the pool
def _split_of(rules: dict):
    def f(rng, j):
        r = rules.get(j, E.CONT)
        if r == ONEHOT:
            return float(rng.integers(0, 4))
        if r == SUBSET:
            return float(int(rng.integers(1, 255)))                     # a bit mask over the codes 0 .. 7
        return 0.0 if rng.random() < 0.15 else float(E.dyadic(rng, 2, 2.0))  # (a split at 0.0 now and then)
    return f


def _retarget(nd, rules, split_of, rng):
    """The rule and split value of every split of a builder that knows no rules (``complete_tree``, ``chain_tree``)."""
    todo = [nd]
    while todo:
        nd = todo.pop()
        if isinstance(nd, E.Split):
            nd.rule = rules.get(nd.var, E.CONT)
            nd.split = float(split_of(rng, nd.var))
            todo += [nd.left, nd.right]


def _tree(rng, shape, K, cols, chain_cols, rules, linear, chain_depth):
    split_of = _split_of(rules)
    if shape == "stump":
        return E.dyadic_leaf(rng, K, linear, free=True)
    if shape == "depth-1":
        return E.dyadic_tree(rng, K, 1, cols, split_of, 1.0, linear, "free", rules)
    if shape in ("bushy", "children-first"):
        return E.dyadic_tree(rng, K, int(rng.integers(2, 7)), cols, split_of, 0.8, linear, "free", rules)
    if shape == "complete-255":
        nd = E.complete_tree(rng, K, 7, cols, split_of, linear, "free")
    else:
        nd = E.chain_tree(rng, K, chain_depth, chain_cols, split_of, shape.split("-")[0], linear, "free")
    _retarget(nd, rules, split_of, rng)
    return nd


def _pool(rng, seed, n_trees, K, cols, chain_cols, rules, linear, chain_depth):
    """``n_trees`` trees of mixed shapes: the first four walk through ``SHAPES`` with the seed, the others are small with
    a large one now and then; the trees stored children first are one pool of their own, spliced in at their places."""
    shapes = []
    for t in range(n_trees):
        if t < 4:
            shapes.append(SHAPES[(seed * 3 + t) % len(SHAPES)])
        else:
            shapes.append(str(rng.choice(SHAPES[:3])) if rng.random() < 0.85 else str(rng.choice(SHAPES)))
    roots = [_tree(rng, s, K, cols, chain_cols, rules, linear, chain_depth) for s in shapes]
    parts = [E.build_pool([r], K, order="reversed" if s == "children-first" else "bfs") for r, s in zip(roots, shapes)]
    pool = TreeArrays.concat(parts) if len(parts) > 1 else parts[0]
    pool.tree_id[:] = np.arange(n_trees)
    return pool, shapes


def validate(oracle, pool, table, p: int) -> None:
    """The oracle's ``pgb_validate_forest``: a one-row ``pgb_predict`` of every forest refuses an unwalkable tree."""
    table = np.ascontiguousarray(table, np.int32)
    x, out = np.zeros((1, p)), np.zeros(table.shape[0] * int(pool.n_outputs))
    carr = pool.as_c()
    rc = oracle.lib.lib.pgb_predict(C.byref(carr), table.ctypes.data, table.shape[0], table.shape[1], x.ctypes.data, 1, p, p,
                                    None, 0, out.ctypes.data, None)
    oracle.lib.check(rc, "pgb_validate_forest")


# ------------------------------------------------------------------ the rows
def _rows(rng, d, n_total, first_row, nb, p, rules, used, pool, no_inf):
    X = rng.normal(size=(n_total, p))
    for j, r in rules.items():
        X[:, j] = rng.integers(0, 4 if r == ONEHOT else 8, n_total)
    cont = [j for j in used if j not in rules]
    block = slice(first_row, first_row + nb)
    mode = d["data"]
    hit = int(used[int(rng.integers(0, len(used)))])
    if mode == "nan-0.05":
        X[rng.random((n_total, p)) < 0.05] = np.nan
    elif mode in ("nan-lane-0", "nan-lane-63"):
        lane = 0 if mode == "nan-lane-0" else min(63, nb - 1)
        X[first_row + lane:first_row + nb:64, hit] = np.nan
    elif mode == "nan-last-tile":
        X[first_row + nb - 1, hit] = np.nan
    elif mode == "nan-column":
        X[:, hit] = np.nan
    elif mode == "split-neighbours" and cont:
        for j in cont:
            v = np.asarray(pool.split)[(np.asarray(pool.var) == j)]
            if v.size:
                edge = np.concatenate([v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)])
                X[:, j] = rng.choice(edge, size=n_total)
    elif mode == "signed-zero" and cont:
        for j in cont:
            X[:, j] = np.where(rng.random(n_total) < 0.5, rng.choice([0.0, -0.0], size=n_total), X[:, j])
    elif mode == "inf":
        for j in [j for j in cont if j not in no_inf]:
            z = rng.random(n_total)
            X[z < 0.15, j] = np.inf
            X[z > 0.85, j] = -np.inf
    elif mode == "unseen-codes":
        for j, r in rules.items():
            X[:, j] = np.where(rng.random(n_total) < 0.3, rng.choice([9.0, 60.0, -3.0, 2.5], size=n_total), X[:, j])
    return X, X[block]


# ------------------------------------------------------------------ the case
def random_walk_case(seed: int, oracle=None) -> dict:
    """One call of every stored-draw entry point, drawn from ``seed`` alone (``oracle``: the backend that validates the
    history; default the suite's)."""
    rng = np.random.default_rng([0x57, seed])
    d = _draw_dims(seed, rng)
    took = dict(d)
    p, K, m, D, nb = d["p"], d["K"], d["m"], d["D"], d["nb"]
    n_trees = m + {"0": 0, "2": 2, "m": m}[d["extra"]]
    # the columns: `used` are split on; `reg` is regressed on by linear leaves; `spare` is used by no tree
    pick = [int(j) for j in rng.permutation(np.arange(1, max(p - 1, 1)))[:4]] if p > 3 else []
    used = sorted({0, p - 1} | set(pick)) if p > 2 else [0]
    free = [j for j in range(p) if j not in used]
    spare = free[0] if free else None
    reg = None
    if d["leaves"] in ("linear-unused", "linear-excluded") and len(free) > 1:
        reg = free[1]
    elif d["leaves"] != "constant":
        reg = used[-1]
        if d["leaves"] == "linear-unused":
            took["leaves"] = "linear-used"
    rules = {}
    if d["rules"] == "mixed":
        rules[used[0]] = ONEHOT
        if len(used) > 2:
            rules[used[1]] = SUBSET
    if reg in rules:                                                    # (a regressor is a number, not a code)
        del rules[reg]
        if not rules:
            rules[used[0]] = ONEHOT
            reg = used[-1] if used[-1] != used[0] else None
            if reg is None:
                took["leaves"] = "constant"
    linear = () if reg is None else (reg,)
    # chains: depth 64 over the used columns, and where p allows it over 64 (SHAPX: 32) distinct columns, so that a
    # path holds exactly the most slots an entry point takes, the regressor's included
    wide = p >= MAX_DEPTH + 1 and seed % 2 == 0
    case = {"seed": seed, "dims": d, "took": took, "p": p, "K": K, "m": m, "D": D, "nb": nb, "used": used, "spare": spare,
            "reg": reg, "rules": rules, "wide_chains": wide}
    pools = {}
    for name, limit in (("full", SHAP_MAX_U), ("u32", SHAPX_MAX_U)):
        r = np.random.default_rng([0x57, seed, 1])                      # the same draws for both: they differ in the chains
        if wide:                                                        # (the regressor's slot is one of the `limit`)
            chain_depth = min(MAX_DEPTH, limit - (reg is not None))
            chain_cols = [j for j in range(p) if j != spare and j != reg and j not in rules][:chain_depth]
        else:
            chain_cols, chain_depth = used, MAX_DEPTH
        pools[name], shapes = _pool(r, seed, n_trees, K, used, chain_cols, rules, linear, chain_depth)
        case["chain_depth_" + name] = chain_depth
    case["pool"], case["pool_u32"], case["shapes"] = pools["full"], pools["u32"], shapes
    case["table"] = np.stack([rng.permutation(n_trees)[:m] for _ in range(D)]).astype(np.int32)
    if d["picks"] == "identity" or D == 1 and d["picks"] == "subset":
        picks = list(range(D))
        took["picks"] = "identity"
    elif d["picks"] == "subset":
        picks = sorted(int(v) for v in rng.permutation(D)[:max(1, D // 2)])
    else:
        picks = [int(v) for v in rng.permutation(D)] + [int(rng.integers(0, D))]
    case["picks"] = picks
    first_row, n_total = d["first_row"], d["first_row"] + nb + d["tail"]
    case["first_row"], case["n_total"], case["pad"] = first_row, n_total, d["pad"]
    every = sorted(set(np.asarray(pools["full"].var)[np.asarray(pools["full"].var) >= 0].tolist())
                   | set(np.asarray(pools["u32"].var)[np.asarray(pools["u32"].var) >= 0].tolist()))
    case["every_used"] = every
    no_inf = set(linear)
    case["X"], case["block"] = _rows(rng, d, n_total, first_row, nb, p, rules, every if wide and every else used,
                                     pools["full"], no_inf)
    if d["data"] == "unseen-codes" and not rules:
        took["data"] = "clean"
    excl = {"none": [], "one-used": [used[-1]], "all": list(range(p))}[d["excluded"]]
    if d["leaves"] == "linear-excluded" and reg is not None and reg not in excl:
        excl = sorted(excl + [reg])
        took["excluded"] = d["excluded"] + "+regressor"
    case["excluded"] = excl
    # ---- the entry points' own arguments
    if d["cols"] == "unused" and spare is None:
        took["cols"] = "one"
    case["cols"] = {"one": [used[-1]], "all": list(range(p)), "unused": [used[0], spare]}[took["cols"]]
    few = sorted(set(used + ([spare] if spare is not None else []) + ([reg] if reg is not None else [])))
    case["cols_few"] = case["cols"] if len(case["cols"]) <= 12 else few   # where the output grows with q * q
    took["cols_few"] = took["cols"] if len(case["cols"]) <= 12 else "used+spare"
    took["all_columns_paired"] = len(case["cols_few"]) == p             # (ident_shapx runs)
    took["constant_leaves"] = reg is None                                # (ident_arms runs)
    case["R"], case["perm_seed"] = d["R"], int(rng.integers(1, 2 ** 31))
    bins = ALE_MAX_BINS if seed % 32 == ONCE_MAX_BINS else d["bins"]
    took["bins"] = bins
    case["edges"] = [np.sort(rng.uniform(-2.5, 2.5, bins + 1)) if c not in rules else np.arange(bins + 1.0) - 0.5
                     for c in case["cols"]]
    A = ARMS_MAX if seed % 32 == ONCE_MAX_ARMS else d["arms"]
    s = min(d["arm_cols"], p)
    took["arms"], took["arm_cols"] = A, s
    arm_cols = (used + [j for j in range(p) if j not in used])[:s]
    case["arm_cols"] = arm_cols
    arms = rng.normal(size=(A, s))
    for c, j in enumerate(arm_cols):
        if j in rules:
            arms[:, c] = rng.integers(0, 4 if rules[j] == ONEHOT else 8, A)
    if A > 1:
        arms[1, 0] = np.nan                                             # an arm that marginalises
    case["arm_values"] = arms
    case["J"], case["levels"] = d["J"], d["levels"]
    q = len(case["cols_few"])
    all_pairs = [(a, b) for a in range(q) for b in range(a + 1, q)]
    if d["pairs"] != "none" and not all_pairs:
        took["pairs"] = "none"
    case["pairs"] = {"none": [], "one": all_pairs[-1:], "all": all_pairs}[took["pairs"]]
    case["weights"] = rng.uniform(0.5, 2.0, n_total)
    case["route"], case["ice_pad"] = {"direct": 1, "profile": 2, "auto": 0}[d["route"]], 2 if d["ice"] == "strided" else 0
    scalar = [f for f in FAMILIES if f not in ("categorical", "normal_meanscale")]
    fam = d["family"]
    if seed < COVER:                                                    # the family fixes the outputs it takes: it walks
        rank = _cell(seed)[1]["K"]                                      # through the families of the case's K
        fam = scalar[rank % len(scalar)] if K == 1 else ("categorical", "normal_meanscale")[rank // len(K_MANY) % 2]
    if K == 1 and fam not in scalar:
        fam = scalar[seed % len(scalar)]
    elif K == 2 and fam in scalar:
        fam = ("categorical", "normal_meanscale")[seed % 2]
    elif K > 2:
        fam = "categorical"
    case["family"] = took["family"] = fam
    n_par = {"normal": 1, "negbin_log": 1, "gamma_log": 1, "asymmetric_laplace": 2, "student_t": 2}.get(fam, 0)
    prm = rng.uniform(0.5, 2.0, (len(picks), n_par))
    if fam == "asymmetric_laplace":
        prm[:, 1] = rng.uniform(0.1, 0.9, len(picks))                   # (b, q): 0 < q < 1
    elif fam == "student_t":
        prm[:, 1] = rng.uniform(2.5, 8.0, len(picks))                   # (sigma, nu)
    case["params"] = prm
    if fam.startswith("bernoulli"):
        y = rng.integers(0, 2, nb)
    elif fam in ("poisson_log", "negbin_log"):
        y = rng.poisson(2.0, nb)
    elif fam == "gamma_log":
        y = rng.gamma(3.0, 0.5, nb)
    elif fam == "categorical":
        y = rng.integers(0, K, nb)
    else:
        y = rng.normal(size=nb)
    case["y"] = np.asarray(y, np.float64)
    inst_rows = rng.integers(0, n_total, 3)
    case["instances"] = case["X"][inst_rows].copy()
    case["ice_picks"] = rng.integers(0, D, (len(case["cols"]), 3, int(rng.integers(1, 5))))
    case["pdp_picks"] = rng.integers(0, D, (len(case["cols"]), len(picks)))
    case["levels_u"] = [1.0, 0.7, 0.4, 0.05][:d["levels"]]
    case["link"] = ("logistic", "probit")[seed // 8 % 2]
    case["offset"] = rng.normal(0, 0.3, nb) if seed % 3 == 0 else None
    if oracle is None:
        from _oracle import oracle_backend

        oracle = oracle_backend()
    for pool in (case["pool"], case["pool_u32"]):
        validate(oracle, pool, case["table"], p)
    return case


def describe(case) -> str:
    return f"seed {case['seed']}: " + ", ".join(f"{k}={v}" for k, v in case["took"].items()) + \
        f", shapes={case['shapes'][:4]}, wide_chains={case['wide_chains']}"


# ------------------------------------------------------------------ the comparison
def compare(got: dict, want: dict, guard: list) -> list:
    """-> the list of what differs (empty: equal).  Doubles compare by their 64-bit patterns, a NaN on both sides at the
    same position counting as equal (``tests/test_rowsummary_gpu.py``); integers compare exactly; the cells of ``guard``
    -- ``(name, cells, value)`` -- are what they were; ``POISON`` shows in no result."""
    bad = []
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name in sorted(want):
        a, b = np.asarray(got[name]), np.asarray(want[name])
        if a.shape != b.shape:
            bad.append(f"{name}: shape {a.shape} != {b.shape}")
        elif b.dtype.kind == "f":
            a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
            both = np.isnan(a) & np.isnan(b)
            diff = (a.view(np.uint64) != b.view(np.uint64)) & ~both
            if diff.any():
                at = tuple(int(v) for v in np.argwhere(diff)[0])
                bad.append(f"{name}: {int(diff.sum())} of {diff.size} differ, first at {at}: {a[at]!r} != {b[at]!r}")
            if np.any(a == POISON):
                bad.append(f"{name}: the padding's value shows in the result")
        elif not np.array_equal(a, b):
            bad.append(f"{name}: {int(np.sum(a != b))} of {a.size} integers differ")
    for name, cells, value in guard:
        if not np.all(np.asarray(cells) == value):
            bad.append(f"{name}: the guard cells were written")
    return bad


def _sample_rows(case, most: int = 6) -> list:
    """The rows an identity in ``Fraction`` arithmetic looks at: both ends of the block, both sides of the first tile
    edge and every row with a NaN, ``most`` at the most."""
    nb, block = case["nb"], case["block"]
    rows = [0, nb - 1, 63, 64] + np.flatnonzero(np.isnan(block).any(axis=1)).tolist()
    out = []
    for r in rows:
        if 0 <= r < nb and r not in out:
            out.append(int(r))
    return out[:most]


def _sampler(case, backend, pool=None):
    pool = case["pool"] if pool is None else pool
    return PosteriorSampler(pool, case["table"], case["m"], case["K"], backend=backend)


# ------------------------------------------------------------------ the runners
# Per entry point three functions:
#   device(case, be, oracle) -> (got, guard)  the call, laid out by the entry point's GPU module (its helper imported);
#                                             `guard`: the cells behind the outputs, where the helper does not assert
#                                             them itself
#   reference(case, oracle)  -> want          the host reference of the entry point's tests/_*_host.py
#   identities(case, res, be)                 what the entry point's module states without going through its header,
#                                             asserted on a result -- the device's, and in the CPU module the reference's
# RUNNERS[entry](case, backend, oracle) -> (got, want, guard) puts them together.
GUARD = -7.75e300


def _fidx(case):
    return case["table"][case["picks"]]


def _wide_block(case):
    wide = np.full((case["nb"], case["p"] + case["pad"]), POISON)
    wide[:, :case["p"]] = case["block"]
    return wide


def _fractions(a):
    from fractions import Fraction

    return np.vectorize(lambda x: Fraction(float(x)), otypes=[object])(a)


# ---- pgb_predict
def dev_predict(case, be, oracle):
    import test_predict_edges_gpu as T

    got = T.predict(be, case["pool"], _fidx(case), case["block"], case["excluded"], case["p"] + case["pad"])
    return {"out": got}, []                                             # (predict asserts the guard behind [D][K][n])


def ref_predict(case, oracle):
    return dev_predict(case, oracle, oracle)[0]


def ident_predict(case, res, be):
    """Against ``_predict_exact.walk`` within its derived bound, at the sampled rows."""
    rows = _sample_rows(case)
    ratio = E.walk(case["pool"], _fidx(case), case["block"][rows], case["excluded"]).bound_ratio(res["out"][:, :, rows])
    assert ratio <= 1.0, f"pgb_predict against the exact walk: error / bound = {ratio}"


# ---- pgb_pointwise_loglik
def dev_pointwise(case, be, oracle):
    import test_predict_edges_gpu as T

    clamped = []
    got = T.pointwise(be, case["pool"], _fidx(case), case["block"], case["y"], case["params"], case["p"] + case["pad"],
                      case["family"], clamped)                          # (asserts the guard)
    return {"ll": got, "clamped": np.asarray(clamped)}, []


def ref_pointwise(case, oracle):
    import _pointwise_host as pw

    mu = ref_predict(dict(case, excluded=[]), oracle)["out"]
    want, nc = pw.matrix(case["family"], case["y"], mu, case["params"] if case["params"].size else None, return_clamped=True)
    return {"ll": want, "clamped": np.asarray([nc])}


# ---- pgb_predict_ice
def dev_ice(case, be, oracle):
    import test_predict_edges_gpu as T

    p = case["p"]
    got = T.ice(be, case["pool"], case["table"], case["block"], case["instances"], case["cols"], case["ice_picks"],
                ldx=p + case["pad"], ldi=p + case["ice_pad"])           # (asserts the guard)
    return {"out": got}, []


def ref_ice(case, oracle):
    import _ice_host as ice_host

    return {"out": ice_host.yardstick(_sampler(case, oracle), case["block"], case["instances"], case["cols"],
                                      case["ice_picks"])}


# ---- pgb_predict_pdp
def dev_pdp(case, be, oracle):
    """The drawn route; the direct and the profile route as well, which must agree bit for bit."""
    import test_pdp_gpu as T

    out = {}
    for route in (case["route"], 1, 2):
        if route not in out:
            out[route] = T._raw(be, _sampler(case, be), _wide_block(case), case["p"], case["cols"], case["pdp_picks"], route,
                                GUARD)
    assert np.array_equal(out[1][0].view(np.uint64), out[2][0].view(np.uint64)), "the direct and the profile route differ"
    return {"out": out[case["route"]][0]}, [("out", np.concatenate([o[2] for o in out.values()]), GUARD)]


def ref_pdp(case, oracle):
    import _pdp_host as pdp_host

    return {"out": pdp_host.yardstick(_sampler(case, oracle), case["block"], case["cols"], case["pdp_picks"])}


# ---- pgb_predict_shap, pgb_predict_shap_interactions
def _shap_tolerance(pool, case, name, rows):
    """``8 * accuracy * M`` of the SHAP modules (``profiles/<name>.json``, ``_shap_host.magnitude``) at ``rows``, as
    ``Fraction``: (D, K, n)."""
    import json

    import _shap_host as host

    accuracy = json.load(open(os.path.join(ROOT, "profiles", name + ".json")))["max"]
    M, _ = host.magnitude(pool, _fidx(case), case["block"][rows])
    return _fractions(8.0 * accuracy * M)


def dev_shap(case, be, oracle):
    import test_shap_gpu as T

    got, base, cells = T._raw(be, case["pool"], case["table"], _wide_block(case), case["p"], case["picks"], GUARD)
    return {"values": got, "base": base}, [("values", cells, GUARD)]


def ref_shap(case, oracle):
    import _shap_host as host

    want, wb = host.rows(case["pool"], case["table"], case["block"], picks=case["picks"])
    return {"values": want, "base": wb}


def ident_shap(case, res, be):
    """Efficiency (``test_shap_gpu.test_efficiency_on_the_device``): ``base + values.sum()`` is the prediction within
    ``(p + 1) tol`` -- one ``tol`` per attribution and the base -- and the walk's ``gamma_N S``."""
    import test_shap_gpu as T

    rows = _sample_rows(case, 3)
    tol = _shap_tolerance(case["pool"], case, "shap_accuracy", rows)
    slack = T._gamma_S(E.walk(case["pool"], _fidx(case), case["block"][rows]))
    pred = _fractions(ref_predict(dict(case, excluded=[]), be)["out"][:, :, rows])
    total = _fractions(res["base"])[:, :, None] + _fractions(res["values"][:, :, :, rows]).sum(axis=2)
    bad = np.abs(total - pred) > (case["p"] + 1) * tol + slack
    assert not bad.any(), f"base + values.sum() against the prediction at {np.argwhere(bad)[0].tolist()} (pick, output, row)"


def dev_shapx(case, be, oracle):
    import test_shap_interaction_gpu as T

    rc, got, base, cells = T._raw(be, case["pool_u32"], case["table"], _wide_block(case), case["p"], case["cols_few"],
                                  case["picks"], guard=GUARD)
    be.lib.check(rc, "pgb_predict_shap_interactions")
    return {"values": got, "base": base}, [("values", cells, GUARD)]


def ref_shapx(case, oracle):
    import _shap_interaction_host as hx

    want, wb = hx.rows(case["pool_u32"], case["table"], case["block"], cols=case["cols_few"], picks=case["picks"])
    return {"values": want, "base": wb}


def ident_shapx(case, res, be):
    """With every column in the call, a row of interactions sums to the SHAP value within ``(p + 1) tol``
    (``test_shap_interaction_gpu.test_row_sums_and_the_total_on_the_device``)."""
    import _shap_host as shap_host

    p = case["p"]
    if len(case["cols_few"]) != p:
        return
    rows = _sample_rows(case, 2)
    tol = _shap_tolerance(case["pool_u32"], case, "shap_interaction_accuracy", rows)
    shap, _ = shap_host.rows(case["pool_u32"], case["table"], case["block"][rows], picks=case["picks"])
    sums = _fractions(res["values"][..., rows]).sum(axis=3)             # (n_picks, K, q, n)
    bad = np.abs(sums - _fractions(shap)) > (p + 1) * tol[:, :, None, :]
    assert not bad.any(), f"interaction row sums against the SHAP value at {np.argwhere(bad)[0].tolist()}"


# ---- pgb_predict_permuted
def _permuted_args(case):
    return (case["pool"], case["table"], case["X"], case["first_row"], case["nb"], case["cols"], case["R"], case["perm_seed"],
            case["picks"])


def dev_permuted(case, be, oracle):
    import _permimp_host as host
    import test_permimp_gpu as T

    got, guard = {}, []
    for mode, name in ((host.PRED, "pred"), (host.DELTA, "delta")):
        rc, out, cells, f = T._call(be, *_permuted_args(case), mode, case["pad"])
        be.lib.check(rc, "pgb_predict_permuted")
        got[name] = out
        guard.append((name, cells, T.GUARD))
        if mode == host.PRED:
            got["f"] = f
    return got, guard


def ref_permuted(case, oracle):
    import _permimp_host as host

    want = {name: host.reference(oracle, *_permuted_args(case), mode) for mode, name in ((host.PRED, "pred"), (host.DELTA, "delta"))}
    want["f"] = host.predict(oracle, case["pool"], _fidx(case), case["block"])
    return want


def ident_permuted(case, res, be):
    if case["spare"] in case["cols"]:                                    # a column no tree uses: +0.0 in DELTA mode
        delta = np.ascontiguousarray(res["delta"][:, case["cols"].index(case["spare"])])
        assert np.all(delta.view(np.int64) == 0), "the delta of a column no tree uses is not +0.0"


# ---- pgb_predict_ale
def _ale_args(case):
    return (case["pool"], case["table"], case["block"], case["cols"], case["edges"], case["picks"])


def dev_ale(case, be, oracle):
    import test_ale_gpu as T

    rc, out, bins, (g_out, g_bins) = T._call(be, *_ale_args(case), case["pad"])
    be.lib.check(rc, "pgb_predict_ale")
    return {"out": out, "bins": bins}, [("out", g_out, T.GUARD), ("bins", g_bins, T.BIN_GUARD)]


def ref_ale(case, oracle):
    import _ale_host as host

    want, wb = host.reference_block(oracle, *_ale_args(case))
    return {"out": want, "bins": wb}


def ident_ale(case, res, be):
    if case["spare"] in case["cols"]:
        out = np.ascontiguousarray(res["out"][case["cols"].index(case["spare"])])
        assert np.all(out.view(np.int64) == 0), "the effect of a column no tree uses is not +0.0"


# ---- pgb_hstat_background / _rows / _finish
def _hstat_blocks(case):
    """The background is the head of the whole matrix, the evaluation rows are the block; both are cut at 64 rows when the
    seed is odd (a block continues the one before it)."""
    Xb, v = case["X"][:130], case["weights"][:130]
    Xe, w = case["block"], case["weights"][case["first_row"]:case["first_row"] + case["nb"]]
    cut = 64 if case["seed"] % 2 else None
    for which, X, wt in (("background", Xb, v), ("rows", Xe, w)):
        edges = [0, X.shape[0]] if cut is None or cut >= X.shape[0] else [0, cut, X.shape[0]]
        for r0, r1 in zip(edges[:-1], edges[1:]):
            yield which, X[r0:r1], wt[r0:r1], r0, r0 == 0


def _hstat_jobs(case):
    import _hstat_host as host

    return host.Jobs(case["pool"], case["table"], case["p"], case["cols_few"], case["pairs"], case["picks"])


def _hstat_result(words, n_common, ws, J, T_, I, out):  # noqa: E741
    res = {"words": np.asarray(words), "n_common": n_common, "ws": ws, "J": J, "T": T_, "I": I,
           "n_nonfinite": np.asarray(out["n_nonfinite"])}
    res.update({key: out[key] for key in ("main_var", "total_var", "h2_total", "inter_var", "h2")})
    return res


def dev_hstat(case, be, oracle):
    import test_hstat_gpu as T

    jobs = _hstat_jobs(case)
    dev = T.Device(be, jobs, case["pad"])
    for which, X, wt, r0, init in _hstat_blocks(case):
        be.lib.check(getattr(dev, which)(X, wt, r0, init), "pgb_hstat_" + which)  # (asserts the guards behind J, T and I)
    ws = dev.workspace()                                                # (asserts the guard behind the workspace)
    J, T_, I = (np.concatenate(getattr(dev, name), axis=-1) for name in ("J", "T", "I"))  # noqa: E741
    return _hstat_result(dev.words, dev.n_common, ws, J, T_, I, dev.finish(np.full((jobs.n_picks, jobs.K), 1.5))), []


def ref_hstat(case, oracle):
    import _hstat_host as host

    jobs = _hstat_jobs(case)
    ref = host.Reference(oracle, jobs)
    for which, X, wt, r0, init in _hstat_blocks(case):
        getattr(ref, which)(X, wt, r0, init)
    return _hstat_result(ref.sizes["words"], ref.n_common, ref.ws, ref.J, ref.T, ref.I,
                         ref.finish(np.full((jobs.n_picks, jobs.K), 1.5)))


# ---- pgb_predict_arms
def _arms_args(case):
    return (case["pool"], case["table"], case["block"], case["arm_cols"], case["arm_values"], case["picks"])


def dev_arms(case, be, oracle):
    import test_decision_gpu as T

    rc, out, lens, (g_out, g_lens) = T._arms_call(be, oracle, *_arms_args(case), case["pad"])
    be.lib.check(rc, "pgb_predict_arms")
    return {"out": out, "lens": lens}, [("out", g_out, T.GUARD), ("lens", g_lens, T.INT_GUARD)]


def ref_arms(case, oracle):
    import _arms_host as host

    want, wl = host.reference_block(oracle, *_arms_args(case))
    return {"out": want, "lens": wl}


def ident_arms(case, res, be):
    """Against ``pgb_predict`` on ``arm_copy`` within ``4 (m + 1) 2^-53 S``, ``S`` the largest sum over a forest's trees
    of the tree's largest ``|leaf|`` (``test_decision_gpu.test_arm_predictions_against_plain_predictions_of_copies``: its
    derivation takes constant leaves, so the identity is held where the case has no linear leaf)."""
    import _arms_host as host

    if case["reg"] is not None:
        return
    pool = case["pool"]
    top = np.abs(np.asarray(pool.value, np.float64).reshape(pool.total_nodes, -1)).max(axis=1) * (np.asarray(pool.var) < 0)
    per_tree = np.array([top[pool.node_off[t]:pool.node_off[t + 1]].max() for t in range(pool.n_trees)])
    bound = 4 * (case["m"] + 1) * 2.0 ** -53 * float(per_tree[case["table"]].sum(axis=1).max())
    for a in range(min(res["out"].shape[0], 3)):
        copy = host.arm_copy(case["block"], case["arm_cols"], case["arm_values"][a])
        plain = ref_predict(dict(case, block=copy, excluded=[], pad=0), be)["out"]
        err = float(np.abs(res["out"][a] - plain).max())
        assert err <= bound, f"pgb_predict_arms against pgb_predict on arm_copy: arm {a}, {err} > {bound}"


# ---- pgb_surv_curves (on the output of pgb_predict_arms)
SURV_CHUNK = 32  # the grid times of one pgb_predict_arms / pgb_surv_curves call here: J = 50 is cut once


def _surv_chunks(case):
    """Per chunk of ``SURV_CHUNK`` grid times: the arms call's arguments (the last used column set to the chunk's
    times) and the rest of the curves call's."""
    import _surv_host as host

    J = case["J"]
    t, dt, beyond = host.grid(J, origin=-0.25, rng=np.random.default_rng([0x57, case["seed"], 2]))
    for c0 in range(0, J, SURV_CHUNK):
        c1 = min(J, c0 + SURV_CHUNK)
        yield c0, (case["pool"], case["table"], case["block"], [case["used"][-1]], t[c0:c1, None], case["picks"]), \
            (t[c0:c1], dt[c0:c1], case["levels_u"], beyond, case["link"], case["offset"])


def dev_surv(case, be, oracle):
    import test_decision_gpu as A
    import test_survival_gpu as T

    got, guard, state, count = {}, [], None, 0
    for c0, arms_args, rest in _surv_chunks(case):
        rc, f, _, (g_out, g_lens) = A._arms_call(be, oracle, *arms_args, case["pad"])
        be.lib.check(rc, "pgb_predict_arms")
        rc, got[f"f{c0}"], state, count, ok = T._curves(be, f, case["K"] - 1, *rest, state=state, count=count, pad=case["pad"])
        be.lib.check(rc, "pgb_surv_curves")
        guard += [("arms", g_out, A.GUARD), ("lens", g_lens, A.INT_GUARD), ("curves", np.asarray([ok]), True)]
    got["state"], got["count"] = state, np.asarray(count)
    return got, guard


def ref_surv(case, oracle):
    import _arms_host as arms_host
    import test_survival_gpu as T

    want, state, count = {}, None, 0
    for c0, arms_args, rest in _surv_chunks(case):
        f, _ = arms_host.reference_block(oracle, *arms_args)
        want[f"f{c0}"], state, count = T._reference(f, case["K"] - 1, *rest, state=state, count=count)
    want["state"], want["count"] = state, np.asarray(count)
    return want


# ---- pgb_predict_leaf_codes
def dev_leaf_codes(case, be, oracle):
    import test_proximity_gpu as T

    got = T.dev_codes(be, case["pool"], _fidx(case), case["block"], case["excluded"], pad_x=case["pad"], pad_c=case["pad"])
    return {"codes": got}, []                                           # (dev_codes asserts its guards)


def ref_leaf_codes(case, oracle):
    import _proximity_host as host

    return {"codes": host.header_codes(case["pool"], _fidx(case), case["block"], case["excluded"])}


def ident_leaf_codes(case, res, be):
    import _proximity_host as host

    fidx = _fidx(case)
    stops = host.stop_nodes(case["pool"], fidx, case["block"], case["excluded"])
    assert np.array_equal(res["codes"], host.pack(stops.reshape(fidx.size, -1))), "the leaf codes are not the recount's stop nodes"


def _none(case, res, be):
    pass


ENTRIES = {
    "pgb_predict": (dev_predict, ref_predict, ident_predict),
    "pgb_pointwise_loglik": (dev_pointwise, ref_pointwise, _none),
    "pgb_predict_ice": (dev_ice, ref_ice, _none),
    "pgb_predict_pdp": (dev_pdp, ref_pdp, _none),
    "pgb_predict_shap": (dev_shap, ref_shap, ident_shap),
    "pgb_predict_shap_interactions": (dev_shapx, ref_shapx, ident_shapx),
    "pgb_predict_permuted": (dev_permuted, ref_permuted, ident_permuted),
    "pgb_predict_ale": (dev_ale, ref_ale, ident_ale),
    "pgb_hstat": (dev_hstat, ref_hstat, _none),
    "pgb_predict_arms": (dev_arms, ref_arms, ident_arms),
    "pgb_surv_curves": (dev_surv, ref_surv, _none),
    "pgb_predict_leaf_codes": (dev_leaf_codes, ref_leaf_codes, ident_leaf_codes),
}


def _runner(entry):
    device, reference, identities = ENTRIES[entry]

    def run(case, backend, oracle):
        got, guard = device(case, backend, oracle)
        identities(case, got, backend)
        return got, reference(case, oracle), guard

    run.__name__ = "run_" + entry
    return run


RUNNERS = {entry: _runner(entry) for entry in ENTRIES}
# the dimensions an entry point's call depends on (the coverage of tests/test_stored_fuzz.py is counted over them)
COMMON = ("p", "K", "data", "rules", "nb", "pad", "m", "D", "extra", "leaves")
CONSUMES = {
    "pgb_predict": COMMON + ("picks", "excluded"), "pgb_pointwise_loglik": COMMON + ("picks", "family"),
    "pgb_predict_ice": COMMON + ("cols", "ice"), "pgb_predict_pdp": COMMON + ("cols", "route"),
    "pgb_predict_shap": COMMON + ("picks",), "pgb_predict_shap_interactions": COMMON + ("picks", "cols_few"),
    "pgb_predict_permuted": COMMON + ("picks", "first_row", "tail", "cols", "R"),
    "pgb_predict_ale": COMMON + ("picks", "cols", "bins"), "pgb_hstat": COMMON + ("picks", "cols_few", "pairs"),
    "pgb_predict_arms": COMMON + ("picks", "arms", "arm_cols"), "pgb_surv_curves": COMMON + ("picks", "J", "levels"),
    "pgb_predict_leaf_codes": COMMON + ("picks", "excluded"),
}


def check(entry: str, case: dict, backend, oracle) -> list:
    """One case through one runner -> what differs (empty: nothing)."""
    try:
        return compare(*RUNNERS[entry](case, backend, oracle))
    except AssertionError as exc:
        return [f"assertion: {exc}"]
