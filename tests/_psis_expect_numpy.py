"""PSIS-weighted expectations restated with NumPy / SciPy from the algorithm's statement -- the smoothed log-weights
``w`` of ``_psis_numpy.psis_column`` (Vehtari et al.; the Zhang-Stephens fit is ``_psis_numpy.gpdfit``), then the
self-normalised sum ``sum_d softmax(w)_d g_d`` (what ArviZ's ``loo_pit`` / ``loo_expectation`` do) -- not from
``include/pgbart_psis.h``: the arithmetic ``pgb_psis_row_expect`` is held against."""
import numpy as np
from scipy.special import logsumexp

from _psis_numpy import LOG_DBL_MIN, gpdfit, tail_length

G_MAX = 1e150


def log_weights(ll: np.ndarray, M: int):
    """(w, k) of one row: the Pareto-smoothed log importance ratios over the draws (not normalised), the Pareto k."""
    ll = np.asarray(ll, float)
    x = -ll - np.max(-ll)
    order = np.argsort(x, kind="stable")
    xs = x[order]
    cutoff = max(xs[-(M + 1)], LOG_DBL_MIN)
    tail = order[xs > cutoff]
    T = tail.size
    k = np.inf
    w = x.copy()
    if T > 4:
        with np.errstate(all="ignore"):
            ecut = np.exp(cutoff)
            k, sigma = gpdfit(np.exp(x[tail]) - ecut)
            if np.isfinite(k):
                p = (np.arange(1, T + 1) - 0.5) / T
                q = -sigma * np.log1p(-p) if k == 0.0 else sigma * np.expm1(-k * np.log1p(-p)) / k
                w[tail] = np.minimum(np.log(q + ecut), 0.0)
    return w, float(k)


def weights_matrix(ll, reff: float = 1.0):
    """(p (D, n), k (n,)): the normalised Pareto-smoothed weights softmax(w) of every row of ``ll`` (D, n)."""
    ll = np.asarray(ll, float)
    M = tail_length(ll.shape[0], reff)
    cols = [log_weights(ll[:, i], M) for i in range(ll.shape[1])]
    w = np.stack([c[0] for c in cols], axis=1)
    return np.exp(w - logsumexp(w, axis=0)[None, :]), np.array([c[1] for c in cols])


def expect_from_weights(p, g, y=None, kind: str = "value"):
    """E (n_e, n) = sum_d p_d g_c(d) of the clamped ``g`` (D, n)."""
    v = np.clip(np.asarray(g, float), -G_MAX, G_MAX)
    if kind == "pit":
        return np.sum(p * ((v < y[None, :]) + 0.5 * (v == y[None, :])), axis=0)[None, :]
    return np.stack([np.sum(p * v, axis=0), np.sum(p * v * v, axis=0)])


def expect_matrix(ll, g, y=None, kind: str = "value", reff: float = 1.0):
    """(E (n_e, n), k (n,)) of the matrices ``ll``, ``g`` (D, n)."""
    p, k = weights_matrix(ll, reff)
    return expect_from_weights(p, g, None if y is None else np.asarray(y, float), kind), k
