"""Test helpers of the ICE tests (``test_ice.py``, ``test_ice_gpu.py``).

* :func:`ice_by_probe_matrices` -- ``individual_conditional_expectation`` as it was before ``pgb_predict_ice``: a
  host loop over columns x instances that builds each probe matrix, predicts it with ``_sample_posterior`` and takes
  ``np.mean`` over the draws.  Kept as the yardstick of the public function.
* :func:`yardstick` -- ``ice_mean`` restated with ``sample_posterior`` on the explicitly built probe matrix, summed
  in pick order in a Python loop and divided once.
* :func:`random_pool` -- hand-built tree pools (``TreeArrays``) that reach every path of the prediction walk.
"""

from __future__ import annotations

import numpy as np

from pymc_bart_amd import _abi
from pymc_bart_amd.partial import _as_matrix, _samplers
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays
from pymc_bart_amd.utils import _sample_posterior


def ice_by_probe_matrices(bart, X, var_idx=None, instances: int = 30, samples: int = 100, centered: bool = True,
                          func=None, random_seed=None, backend=None) -> dict:
    Xm, names = _as_matrix(X)
    n, p = Xm.shape
    cols = list(range(p)) if var_idx is None else [int(v) for v in var_idx]
    sampler = _samplers(bart, backend)
    rng = np.random.default_rng(random_seed)
    chosen = rng.choice(n, replace=False, size=min(int(instances), n))
    out = {"x": {}, "ice": {}, "labels": {}, "instances": chosen}
    for j in cols:
        others = [v for v in range(p) if v != j]
        curves = []
        for row in chosen:
            probe = Xm.copy()
            probe[:, others] = Xm[row, others]
            curves.append(_sample_posterior(sampler, X=probe, rng=rng, size=samples).mean(axis=0))
        ice_j = np.asarray(curves)
        if func is not None:
            ice_j = func(ice_j)
        if centered:
            ice_j = ice_j - ice_j[:, :1, :]
        out["x"][j] = Xm[:, j]
        out["ice"][j] = ice_j
        out["labels"][j] = names[j]
    return out


def yardstick(sampler, X, instances, cols, picks) -> np.ndarray:
    """``(n_cols, n_inst, K, n_rows)`` through ``sampler.sample_posterior`` on every probe matrix."""
    X = np.asarray(X, np.float64)
    inst = np.asarray(instances, np.float64)
    picks = np.asarray(picks)
    n, p = X.shape
    out = None
    for c, j in enumerate(cols):
        for r in range(inst.shape[0]):
            probe = np.tile(inst[r], (n, 1))
            probe[:, j] = X[:, j]
            pred = np.asarray(sampler.sample_posterior(probe, [int(v) for v in picks[c, r]], None))
            total = pred[0].copy()
            for s in range(1, pred.shape[0]):
                total = total + pred[s]
            if out is None:
                out = np.empty((len(cols), inst.shape[0]) + total.shape)
            out[c, r] = total / float(pred.shape[0])
    return out


def random_pool(rng, n_trees: int, p: int, K: int = 1, depth: int = 4, rules=None, linear=None, split_cols=None,
                chain: bool = False) -> TreeArrays:
    """``n_trees`` random trees of at most ``depth`` levels over ``p`` columns (children after their parent, counts
    that add up).  ``rules``: the split rule of every column (default continuous; one-hot columns hold the codes
    0 .. 3, subset columns 0 .. 7).  ``linear``: columns the leaves regress on (a third of the leaves stay constant).
    ``split_cols``: the columns splits may use (default all).  ``chain``: every split has one leaf child, so that
    the trees are as deep as ``depth`` allows."""
    rules = np.zeros(p, np.int32) if rules is None else np.asarray(rules, np.int32)
    split_cols = np.arange(p) if split_cols is None else np.asarray(split_cols)
    trees = []
    for _ in range(n_trees):
        nodes = [dict(depth=0, count=int(rng.integers(200, 400)))]
        k = 0
        while k < len(nodes):
            nd = nodes[k]
            grow = nd["depth"] < depth and len(nodes) + 2 <= 200 and (k == 0 or rng.random() < (0.95 if chain else 0.7))
            if chain and k > 0 and nodes[k].get("leaf_only"):
                grow = False
            if grow and nd["count"] >= 2:
                j = int(rng.choice(split_cols))
                nd["var"] = j
                nd["rule"] = int(rules[j])
                if rules[j] == _abi.RULE_ONEHOT:
                    nd["split"] = float(rng.integers(0, 4))
                elif rules[j] == _abi.RULE_SUBSET:
                    nd["split"] = float(int(rng.integers(1, 255)))  # a bit mask over the codes 0 .. 7
                else:
                    nd["split"] = float(rng.normal())
                cl = int(rng.integers(1, max(2, nd["count"] // 8) if chain else nd["count"]))
                nd["left"], nd["right"] = len(nodes), len(nodes) + 1
                nodes.append(dict(depth=nd["depth"] + 1, count=cl, leaf_only=chain))
                nodes.append(dict(depth=nd["depth"] + 1, count=nd["count"] - cl))
            else:
                nd["var"] = -1
            k += 1
        trees.append(nodes)
    total = sum(len(t) for t in trees)
    pool = TreeArrays.empty(n_trees, total, K)
    g = 0
    for t, nodes in enumerate(trees):
        pool.tree_id[t] = t
        pool.node_off[t] = g
        for nd in nodes:
            pool.var[g] = nd["var"]
            pool.count[g] = nd["count"]
            if nd["var"] >= 0:
                pool.split[g], pool.left[g], pool.right[g], pool.rule[g] = nd["split"], nd["left"], nd["right"], nd["rule"]
            else:
                pool.value[g] = rng.normal(size=K)
                if linear is not None and rng.random() < 2 / 3:
                    pool.svar[g] = int(rng.choice(linear))
                    pool.slope[g] = rng.normal(size=K)
                    pool.xbar[g] = rng.normal()
            g += 1
    pool.node_off[n_trees] = g
    return pool


def pool_sampler(rng, pool: TreeArrays, m: int, n_draws: int, backend) -> PosteriorSampler:
    """Draws that pick ``m`` of the pool's trees each (without replacement within a draw)."""
    table = np.stack([rng.choice(pool.n_trees, size=m, replace=False) for _ in range(n_draws)]).astype(np.int32)
    return PosteriorSampler(pool, table, m, pool.n_outputs, backend=backend)
