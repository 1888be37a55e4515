"""Partial dependence and individual conditional expectation *data* (SURVEY.md 8f f1/f4 neighbours).

The reference computes these inside its plotting functions (``plot_pdp`` ``utils.py:312-487``,
``plot_ice`` ``utils.py:168-310``) and draws them with matplotlib; drawing is out of scope here,
the numbers are not: they are sweeps of posterior predictions -- per covariate ``samples x m x grid``
tree traversals with every OTHER covariate marginalised out by the trees' own training counts
(``excluded``) for the PDP, and ``instances x samples x m x n`` traversals for ICE -- i.e. work for
the ``k_pdp_walk`` / ``k_pdp_lookup`` kernels behind ``PosteriorSampler.pdp_sweep`` (the PDP) and for ``k_ice`` behind
``PosteriorSampler.ice_mean`` (ICE) -- every curve of a sweep from one fused call each.

What the functions return is exactly what upstream hands to its axes: per covariate the grid
``x`` and the array of predictions; random draws follow the same call pattern (one
``rng.integers`` per prediction call, in the same order).
"""

from __future__ import annotations

import numpy as np

from .utils import _get_posterior_sampler, _resident_rows

DEFAULT_QUANTILES = (0.05, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.95)  # upstream's default grid


def _as_matrix(X):
    if hasattr(X, "columns") and hasattr(X, "to_numpy"):
        return np.asarray(X.to_numpy(), np.float64), [str(c) for c in X.columns]
    X = np.asarray(X, np.float64)
    return X, [f"X_{j}" for j in range(X.shape[1])]


def pdp_grid(X, xs_interval: str = "quantiles", xs_values=None) -> np.ndarray:
    """The rows at which the partial dependence is evaluated (one grid per column, side by side):
    ``"insample"`` -- the data themselves; ``"linear"`` -- ``xs_values`` (default 10) equally spaced
    points between each column's minimum and maximum; ``"quantiles"`` -- each column's quantiles
    ``xs_values`` (default 5 % ... 95 %)."""
    X = np.asarray(X, np.float64)
    if xs_interval == "insample":
        return X
    if xs_interval == "linear":
        k = 10 if xs_values is None else int(xs_values)
        return np.linspace(X.min(axis=0), X.max(axis=0), num=k, axis=0)
    if xs_interval == "quantiles":
        q = list(DEFAULT_QUANTILES if xs_values is None else xs_values)
        return np.quantile(X, q=q, axis=0)
    raise ValueError(f"{xs_interval} is not supported: use 'insample', 'linear' or 'quantiles'")


def _samplers(bart, backend):
    group = bart if isinstance(bart, list) else [bart]
    ops = [b.owner.op if getattr(b, "owner", None) is not None else b for b in group]
    got = [_get_posterior_sampler(op, backend=backend) for op in ops]
    return got if isinstance(bart, list) else got[0]


def _summarised(g, grid, cols, picks, spec, keep_pd: bool):
    """The sweep of one sampler with ``summary=``: ``(pred (n_cols, samples, K, grid) or None, [summary dict per
    column])``.  Every block of the sweep stays on the device: a column's ``[samples][K * rows]`` part of it is the
    matrix ``pgb_row_summary`` takes; only with ``keep_pd`` is the block also copied to the host."""
    from ._stored import hip_only, history
    from .pdp import checked, device_blocks
    from .summary import result, spec as summary_spec, summary_block

    parts, pool, table = history(g)
    be = hip_only(parts[0]._get_backend(), "posterior summaries run")
    lib, mem = be.lib, be.mem
    K, m = int(parts[0].n_outputs), int(parts[0].m)
    D = int(picks.shape[1])
    q, hdi_k, code = summary_spec(D, *spec)
    X, cols, picks = checked(grid, False, cols, picks, int(np.asarray(table).shape[0]), 0)
    n = int(X.shape[0])
    stats = np.empty((cols.size, 2 + q.size + 2, K, n))
    pred = np.empty((cols.size, D, K, n)) if keep_pd else None
    for c0, c1, r0, r1, od in device_blocks(be, pool, table, m, K, X, cols, picks):
        width = K * (r1 - r0)
        for c in range(c0, c1):
            md = od[(c - c0) * D * width:(c - c0 + 1) * D * width]  # [D][K][rows of the block]
            stats[c, :, :, r0:r1] = summary_block(lib, mem, md, D, width, width, None, code, q, hdi_k).reshape(-1, K, r1 - r0)
        if keep_pd:
            pred[c0:c1, :, :, r0:r1] = mem.to_host(od).reshape(c1 - c0, D, K, r1 - r0)
    return pred, [result(stats[c], n, K, q, spec[1], hdi_k, D) for c in range(cols.size)]


def partial_dependence(bart, X, var_idx=None, xs_interval: str = "quantiles", xs_values=None,
                       samples: int = 200, func=None, random_seed=None, backend=None, summary=None,
                       keep_pd: bool = True) -> dict:
    """Partial dependence of the BART function on each covariate of ``var_idx``.

    For covariate ``j`` the forest is evaluated on the grid with all other covariates excluded:
    at a split on an excluded covariate a tree answers with the count-weighted mean of both
    subtrees, which is BART's own marginalisation.  Returns ``{"x": {j: grid_j}, "pd": {j: array
    (samples, grid, outputs)}, "labels": {j: name}, "reference": mean of all partial dependences}``
    (the dashed reference line of the upstream plot).

    The draws of every covariate are chosen first -- one ``rng.integers(0, n_draws, samples)`` per covariate, in
    covariate order, as one ``_sample_posterior`` call per covariate chose them -- and all of them then come from ONE
    ``pdp_sweep`` call per sampler (``include/pgbart_pdp.h``: the trees are uploaded once, and a covariate that only
    ``x <= v`` splits test is evaluated once per interval between its split values, not once per row).

    ``summary={"quantiles": ..., "hdi_prob": ..., "transform": ...}`` (every key optional) adds ``out["summary"][j]``:
    the mean, sd, var, quantiles and HDI of ``pd[j]`` over its samples -- arrays ``(grid, outputs)`` -- computed on
    the device from the same draws by :func:`~pymc_bart_amd.posterior_summary`'s kernel, on the sweep where it lies.
    ``func`` is a host function and cannot be combined with it: name a ``transform``.  ``keep_pd=False`` (with
    ``summary=`` only) leaves ``pd[j]`` ``None``: nothing of size samples x grid reaches the host -- what makes
    ``xs_interval="insample"`` usable on large data -- and ``reference`` is the mean of the summaries' means."""
    spec = None
    if summary is not None:
        if func is not None:
            raise ValueError("func cannot be combined with summary=: the summary is computed on the device "
                             "(use summary={'transform': ...})")
        unknown = set(summary) - {"quantiles", "hdi_prob", "transform"}
        if unknown:
            raise ValueError(f"summary takes the keys quantiles, hdi_prob and transform, got {sorted(unknown)}")
        from . import summary as _summary

        spec = (summary.get("quantiles", _summary.DEFAULT_QUANTILES), summary.get("hdi_prob", _summary.DEFAULT_HDI_PROB),
                summary.get("transform", "identity"))
        _summary.spec(int(samples), *spec)  # (refused before a backend is touched)
    elif not keep_pd:
        raise ValueError("keep_pd=False leaves nothing to return without summary=: name the summaries to keep")
    Xm, names = _as_matrix(X)
    p = Xm.shape[1]
    cols = list(range(p)) if var_idx is None else [int(v) for v in var_idx]
    sampler = _samplers(bart, backend)
    group = sampler if isinstance(sampler, list) else [sampler]
    rng = np.random.default_rng(random_seed)
    grid = pdp_grid(Xm, xs_interval, xs_values)
    out = {"x": {}, "pd": {}, "labels": {}, "reference": None}
    if spec is not None:
        out["summary"] = {}
    if not cols:
        return out
    picks = np.stack([rng.integers(0, group[0].n_draws, size=int(samples)) for _ in cols])
    if spec is None:
        rows = _resident_rows(sampler, grid) if len(group) > 1 else grid  # (several samplers: one upload for all)
        preds = [g.pdp_sweep(rows, cols, picks) for g in group]  # (n_cols, samples, K_g, grid)
        summaries = None
    else:
        got = [_summarised(g, grid, cols, picks, spec, keep_pd) for g in group]
        preds = [pr for pr, _ in got] if keep_pd else None
        summaries = got[0][1]
        for c in range(len(cols) if len(got) > 1 else 0):  # a list of samplers contributes its outputs side by side
            for key in ("mean", "sd", "var", "quantiles", "hdi"):
                if summaries[c][key] is not None:
                    summaries[c][key] = np.concatenate([sm[c][key] for _, sm in got], axis=-1)
    stacked = None
    if preds is not None:
        stacked = preds[0] if len(preds) == 1 else np.concatenate(preds, axis=2)
    means = []
    for c, j in enumerate(cols):
        pd_j = None
        if stacked is not None:
            pd_j = np.ascontiguousarray(np.moveaxis(stacked[c], 1, 2))  # (samples, grid, K)
            if func is not None:
                pd_j = func(pd_j)
            means += [float(pd_j[:, :, k].mean()) for k in range(pd_j.shape[2])]
        else:
            mean_j = summaries[c]["mean"]
            means += [float(mean_j[:, k].mean()) for k in range(mean_j.shape[1])]
        if summaries is not None:
            out["summary"][j] = summaries[c]
        out["x"][j] = grid[:, j]
        out["pd"][j] = pd_j
        out["labels"][j] = names[j]
    out["reference"] = float(np.mean(means)) if means else None
    return out


def individual_conditional_expectation(bart, X, var_idx=None, instances: int = 30, samples: int = 100,
                                       centered: bool = True, func=None, random_seed=None,
                                       backend=None) -> dict:
    """ICE curves: for each of ``instances`` randomly chosen rows, the posterior-mean prediction
    along the observed values of covariate ``j`` with all other covariates held at that row's
    values.  Returns ``{"x": {j: X[:, j]}, "ice": {j: array (instances, n, outputs)}, "labels"}``;
    ``centered`` subtracts each curve's value at the first row, as the upstream plot does.

    The draws of every curve are chosen first -- one ``rng.integers(0, n_draws, samples)`` per (covariate,
    instance), in that order -- and all curves then come from ONE ``ice_mean`` call per sampler: no probe matrix is
    built (``include/pgbart_ice.h``).  A list of BART variables contributes its outputs side by side, from the
    same draws."""
    Xm, names = _as_matrix(X)
    n, p = Xm.shape
    cols = list(range(p)) if var_idx is None else [int(v) for v in var_idx]
    sampler = _samplers(bart, backend)
    group = sampler if isinstance(sampler, list) else [sampler]
    rng = np.random.default_rng(random_seed)
    chosen = rng.choice(n, replace=False, size=min(int(instances), n))
    out = {"x": {}, "ice": {}, "labels": {}, "instances": chosen}
    if not cols:
        return out
    picks = np.empty((len(cols), len(chosen), int(samples)), np.int64)
    for c in range(len(cols)):
        for r in range(len(chosen)):
            picks[c, r] = rng.integers(0, group[0].n_draws, size=int(samples))
    rows = _resident_rows(sampler, Xm) if len(group) > 1 else Xm  # (several samplers: one upload for all of them)
    blocks = [g.ice_mean(rows, Xm[chosen], cols, picks) for g in group]  # (n_cols, n_inst, K_g, n)
    stacked = blocks[0] if len(blocks) == 1 else np.concatenate(blocks, axis=2)
    for c, j in enumerate(cols):
        ice_j = np.ascontiguousarray(np.moveaxis(stacked[c], 1, 2))  # (n_inst, n, K)
        if func is not None:
            ice_j = func(ice_j)
        if centered:
            ice_j = ice_j - ice_j[:, :1, :]
        out["x"][j] = Xm[:, j]
        out["ice"][j] = ice_j
        out["labels"][j] = names[j]
    return out
