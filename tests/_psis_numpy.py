"""PSIS-LOO restated with NumPy / SciPy (libm ``log1p``, ``expm1``, ``logsumexp``) from the algorithm's statement --
Vehtari, Simpson, Gelman, Yao, Gabry, with the Zhang-Stephens generalised-Pareto fit; what ArviZ's ``psislw`` /
``_gpdfit`` / ``_gpinv`` do -- not from ``include/pgbart_psis.h``: the arithmetic the header is held against."""
import numpy as np
from scipy.special import logsumexp

LOG_DBL_MIN = np.log(np.finfo(float).tiny)


def tail_length(D: int, reff: float = 1.0) -> int:
    return int(np.ceil(min(D / 5.0, 3.0 * np.sqrt(D / reff))))


def gpdfit(a: np.ndarray):
    """(k, sigma) of the sorted exceedances ``a`` (ascending)."""
    T = a.size
    m_est = 30 + int(np.floor(np.sqrt(T)))
    j = np.arange(1, m_est + 1, dtype=float)
    b = (1.0 - np.sqrt(m_est / (j - 0.5))) / (3.0 * a[int(T / 4 + 0.5) - 1]) + 1.0 / a[-1]
    k = np.log1p(-b[:, None] * a[None, :]).mean(axis=1)
    L = T * (np.log(-b / k) - k - 1.0)
    w = 1.0 / np.exp(L[None, :] - L[:, None]).sum(axis=1)
    keep = w >= 10.0 * np.finfo(float).eps
    w = w[keep] / w[keep].sum()
    bb = float(np.sum(w * b[keep]))
    kp = float(np.log1p(-bb * a).mean())
    sigma = -kp / bb
    return (T * kp + 5.0) / (T + 10.0), sigma


def psis_column(ll: np.ndarray, M: int):
    """(elpd_loo_i, k_i, T) of one row's values over the draws."""
    ll = np.asarray(ll, float)
    x = -ll - np.max(-ll)
    order = np.argsort(x, kind="stable")
    xs = x[order]
    cutoff = max(xs[-(M + 1)], LOG_DBL_MIN)
    tail = order[xs > cutoff]                      # ascending
    T = tail.size
    k = np.inf
    w = x.copy()
    if T > 4:
        with np.errstate(all="ignore"):
            ecut = np.exp(cutoff)
            k, sigma = gpdfit(np.exp(x[tail]) - ecut)
            if np.isfinite(k):
                p = (np.arange(1, T + 1) - 0.5) / T
                if k == 0.0:
                    q = -sigma * np.log1p(-p)
                else:
                    q = sigma * np.expm1(-k * np.log1p(-p)) / k
                w[tail] = np.minimum(np.log(q + ecut), 0.0)
    return float(logsumexp(w + ll) - logsumexp(w)), float(k), int(T)


def psis_matrix(ll: np.ndarray, reff: float = 1.0):
    """(elpd_loo_i, k_i, T_i) of the matrix ``ll`` (D, n)."""
    ll = np.asarray(ll, float)
    M = tail_length(ll.shape[0], reff)
    out = [psis_column(ll[:, i], M) for i in range(ll.shape[1])]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]))
