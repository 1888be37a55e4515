"""Cases of the folded last round (k_ctrl: a slot whose proposed SMC round is empty and final ends the tree itself),
shared by tests/test_fold_last_round.py (CPU: what each case is there for) and tests/test_fold_last_round_gpu.py.

Small on purpose: 130 .. 2 100 rows (1 .. 3 chunks of 1024, the last one partial), 3 .. 6 columns, 1 .. 10 trees,
10 .. 30 steps.  STAR: data without missing values and continuous columns only, so an attempt always finds its row
and grows -- the last proposed round of a tree has no attempt, and every tree whose round 0 is not empty folds.
"""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np

from pymc_bart_amd.sampler import PyBartSettings


def _rng(name):
    return np.random.default_rng(int(hashlib.sha1(("fold/" + name).encode()).hexdigest()[:8], 16))


def _friedman(rng, n, p):
    X = rng.uniform(0, 1, (n, p))
    f = 10 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 20 * (X[:, 2] - 0.5) ** 2
    if p > 3:
        f = f + 10 * X[:, 3]
    return X, f


def fold_case(name):
    rng = _rng(name)
    c = dict(name="fold/" + name, m=6, P=10, steps=16, batch=(0.5, 0.5), rules=None, prior=None, seed=3415)
    if name == "normal_p40_tuned":      # 1: three chunks, 5 trees a step: 60 tuned tree updates > m, so `rebuild` runs
        X, f = _friedman(rng, 2100, 5)
        c.update(X=X, Y=f + rng.normal(0, 1, 2100), m=10, P=40, steps=24)
    elif name in ("p5", "p64"):         # 2: the smallest and the largest particle count of the 64-particle build
        X, f = _friedman(rng, 1025, 3)
        c.update(X=X, Y=f + rng.normal(0, 1, 1025), m=5, P=5 if name == "p5" else 64, steps=16)
    elif name == "p100":                # 3: two particles per lane; ancestors cross the block boundary of the scan
        X, f = _friedman(rng, 1300, 4)
        c.update(X=X, Y=f + rng.normal(0, 1, 1300), m=4, P=100, steps=10, batch=(1.0, 1.0))
    elif name == "deep":                # 4: trees of well over 8 rounds: the label ring (8 generations) wraps
        n = 2000
        X = rng.normal(size=(n, 3))
        Y = np.sin(5 * X[:, 0]) * 3 + np.cos(3 * X[:, 1]) * 2 + rng.normal(0, 0.05, n)
        c.update(X=X, Y=Y, m=4, P=10, steps=14, alpha=0.999, beta=0.1)
    elif name == "caps_n130":           # 5: the node table fills (n_nodes + 2 > 255) and leaves run out of rows (cnt < 2)
        n = 130
        X = rng.normal(size=(n, 3))
        f = np.sin(3 * X[:, 0]) + np.where(X[:, 1] < 0, X[:, 1], -0.5 * X[:, 1])
        c.update(X=X, Y=f + rng.normal(0, 0.3, n), m=2, P=10, steps=10, batch=(1.0, 1.0), alpha=0.9999, beta=0.0)
    elif name == "m1":                  # 6: tree_new == tree_old
        X, f = _friedman(rng, 700, 3)
        c.update(X=X, Y=f + rng.normal(0, 1, 700), m=1, P=10, steps=30)
    elif name == "one_tree_per_step":   # 7: every tree is the last of its step: the fold into the lone CMD_FINAL
        X, f = _friedman(rng, 1100, 4)
        c.update(X=X, Y=f + rng.normal(0, 1, 1100), m=4, P=12, steps=20, batch=(1, 1))
    elif name == "nan_onehot_subset":   # 8 (no star): attempts that fail at the selection, grows that fail with ok == -1
        n = 1500
        X = rng.normal(size=(n, 4))
        X[rng.random(n) < 0.9, 1] = np.nan          # mostly missing: the row draws run out of tries
        X[:, 2] = 2.0                               # one-hot column with one value: every grow on it fails
        X[rng.random(n) < 0.25, 2] = np.nan
        X[:, 3] = 3.0                               # subset column with one category: likewise
        Y = X[:, 0] + rng.normal(0, 0.3, n)
        c.update(X=X, Y=Y, m=6, P=10, steps=20, rules=np.array([0, 0, 1, 2], np.int32),
                 prior=np.array([1.0, 3.0, 3.0, 3.0]))
    elif name == "probit":              # 9: the slot has a likelihood pass; the weights come from ll_tot
        n = 1500
        X = rng.normal(size=(n, 4))
        from scipy.special import ndtr
        Y = (rng.random(n) < ndtr(1.5 * X[:, 0] - (X[:, 1] > 0))).astype(float)
        c.update(X=X, Y=Y, m=6, P=12, steps=14, family="bernoulli_probit")
    elif name == "compat3":             # 10: particles with n_nodes == 1 carry log-weight 0 into the folded final pick
        X, f = _friedman(rng, 1200, 4)
        c.update(X=X, Y=f + rng.normal(0, 1, 1200), m=6, P=10, steps=16, compat=3)
    elif name == "ties":                # 11: a constant response: every particle ties, thr meets W[q] at equality
        n = 600
        X = rng.normal(size=(n, 3))
        c.update(X=X, Y=np.full(n, 1.5), m=4, P=9, steps=12)
    elif name == "kvector":             # 12: K-vector leaves ...
        n, K = 1200, 3
        X = rng.normal(size=(n, 4))
        F = np.stack([X[:, 0], -X[:, 0], 1.5 * X[:, 1]])
        pr = np.exp(F) / np.exp(F).sum(0)
        Y = (rng.random(n)[None, :] > np.cumsum(pr, axis=0)).sum(0).clip(0, K - 1).astype(float)
        c.update(X=X, Y=Y, m=4, P=10, steps=12, family="categorical", K=K)
    elif name == "linear":              # ... and linear leaves
        n = 1200
        X = rng.uniform(-2, 2, size=(n, 3))
        f = np.where(X[:, 0] < 0, 2 * X[:, 0] + 1, -1.5 * X[:, 0] + 1)
        c.update(X=X, Y=f + rng.normal(0, 0.1, n), m=4, P=10, steps=12, response="linear")
    else:
        raise KeyError(name)
    return c


# fold rate: slots(unfolded) - slots(folded) == tree_updates
STAR = ["normal_p40_tuned", "p5", "p64", "p100", "deep", "m1", "one_tree_per_step", "probit", "compat3"]
NO_STAR = ["caps_n130", "ties"]        # equal outputs; the fold rate is not a condition there
NOT_ALWAYS = ["nan_onehot_subset"]     # the difference is strictly smaller than tree_updates
OTHER_INSTANCES = ["kvector", "linear"]  # k_ctrl<MK> / <LIN>: today's path, whatever PGB_FOLD_LAST says
ALL = STAR + NO_STAR + NOT_ALWAYS + OTHER_INSTANCES


def settings_of(c):
    return PyBartSettings.from_data(c["X"], c.get("bart_Y", c["Y"]), m=c["m"], num_particles=c["P"], seed=c["seed"],
                                    batch=c["batch"], alpha=c.get("alpha", 0.95), beta=c.get("beta", 2.0),
                                    family=c.get("family", "normal"), n_outputs=c.get("K", 1),
                                    response=c.get("response", "constant"), compat=c.get("compat", 0))


def trees_with_an_empty_round0(c, oracle, tree_updates):
    """Tree updates whose round 0 has no attempt: none of the particles 1 .. P - 1 draws a coin
    (iter, 0, i, PROPOSE).u0 above P(leaf | depth 0).  (Tree update k of a chain runs under iter = k; 0 and
    tree_updates + 1 are looked at too.)"""
    f = oracle.lib.lib.pgbo_draw2
    f.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    f.restype = None
    st = settings_of(c)
    pl0 = float(st.prior_leaf[0])
    out, empty = np.zeros(2), []
    for it in range(int(tree_updates) + 2):
        coins = []
        for i in range(1, c["P"]):
            f(int(st.seed), it, 0, i, 1, 0, out.ctypes.data)
            coins.append(float(out[0]))
        if not any(pl0 < u for u in coins):
            empty.append(it)
    return empty


_ORACLE_RUNS = {}


def oracle_run(name, oracle):
    """The oracle's run of a case: computed once, shared by every test that compares against it, never changed."""
    if name not in _ORACLE_RUNS:
        from _cases import run_case

        _ORACLE_RUNS[name] = run_case(fold_case(name), oracle)
    return _ORACLE_RUNS[name]
