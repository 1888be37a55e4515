"""An independent NumPy / SciPy restatement of the published convergence diagnostics (Vehtari, Gelman, Simpson,
Carpenter, Buerkner 2021, "Rank-normalization, folding, and localization: an improved R-hat"; the form ArviZ's
``rhat`` / ``ess`` give them): split chains, ``scipy.stats.rankdata(method="average")``, ``scipy.special.ndtri``,
autocovariances by ``np.fft``, ``np.quantile`` and ``np.median``.  It takes nothing from ``include/pgbart_diag.h``.

One column is an array ``(n_chains, n_per_chain)``.  With an odd ``n_per_chain`` the middle draw is dropped before
anything else (the split), from the ranks and the quantiles too."""
import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata


def split(x: np.ndarray) -> np.ndarray:
    """(n_chains, n) -> (2 n_chains, n // 2): the first and the last half of every chain."""
    n = x.shape[1]
    h = n // 2
    return np.stack([part for chain in x for part in (chain[:h], chain[n - h:])])


def z_scale(s: np.ndarray) -> np.ndarray:
    r = rankdata(s, method="average").reshape(s.shape)
    return ndtri((r - 0.375) / (s.size + 0.25))


def autocov(s: np.ndarray) -> np.ndarray:
    """Biased autocovariance of every row by FFT."""
    n = s.shape[1]
    m = 1
    while m < 2 * n:
        m *= 2
    d = s - s.mean(axis=1, keepdims=True)
    f = np.fft.rfft(d, n=m, axis=1)
    return np.fft.irfft(f * np.conj(f), n=m, axis=1)[:, :n] / n


def rhat2(s: np.ndarray) -> float:
    n = s.shape[1]
    between = n * np.var(s.mean(axis=1), ddof=1)
    within = np.mean(np.var(s, axis=1, ddof=1))
    if between == 0.0 and within == 0.0:
        return 1.0
    with np.errstate(divide="ignore"):
        return float((between / within + n - 1) / n)


def ess(s: np.ndarray) -> float:
    n_chain, n_draw = s.shape
    acov = autocov(s)
    chain_mean = s.mean(axis=1)
    mean_var = np.mean(acov[:, 0]) * n_draw / (n_draw - 1.0)
    var_plus = mean_var * (n_draw - 1.0) / n_draw + np.var(chain_mean, ddof=1)
    if np.ptp(s) == 0.0:
        return float(n_chain * n_draw)
    rho = np.zeros(n_draw + 2)
    even = 1.0
    rho[0] = even
    odd = 1.0 - (mean_var - np.mean(acov[:, 1])) / var_plus
    rho[1] = odd
    t = 1
    while t < n_draw - 3 and even + odd > 0.0:
        even = 1.0 - (mean_var - np.mean(acov[:, t + 1])) / var_plus
        odd = 1.0 - (mean_var - np.mean(acov[:, t + 2])) / var_plus
        if even + odd >= 0.0:
            rho[t + 1] = even
            rho[t + 2] = odd
        t += 2
    max_t = t - 2
    if even > 0.0:
        rho[max_t + 1] = even
    t = 1
    while t <= max_t - 2:
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = (rho[t - 1] + rho[t]) / 2.0
            rho[t + 2] = rho[t + 1]
        t += 2
    size = n_chain * n_draw
    tau = -1.0 + 2.0 * np.sum(rho[:max_t + 1]) + np.sum(rho[max_t + 1:max_t + 2])
    tau = max(tau, 1.0 / np.log10(size))
    return float(size / tau)


def column(x: np.ndarray) -> dict:
    """Every diagnostic of one column ``(n_chains, n_per_chain)``."""
    s = split(np.asarray(x, np.float64))
    q05, q95 = np.quantile(s, 0.05), np.quantile(s, 0.95)
    z = z_scale(s)
    folded = z_scale(np.abs(s - np.median(s)))
    return {"rhat2_bulk": rhat2(z), "rhat2_folded": rhat2(folded), "ess_bulk": ess(z),
            "ess_tail_lo": ess((s <= q05).astype(np.float64)), "ess_tail_hi": ess((s >= q95).astype(np.float64)),
            "ess_mean": ess(s), "mean": float(s.mean()), "var": float(s.var(ddof=1)) if np.ptp(s) > 0.0 else 0.0,
            "constant": float(np.ptp(s) == 0.0)}


ROWS = ("rhat2_bulk", "rhat2_folded", "ess_bulk", "ess_tail_lo", "ess_tail_hi", "ess_mean", "mean", "var", "constant")


def columns(a, n_chains: int, transform: str = "identity") -> np.ndarray:
    """``(9, n)`` of the columns of ``a`` (n_chains * n_per_chain, n), the rows in the order of ``ROWS``."""
    a = np.asarray(a, np.float64)
    D, n = a.shape
    out = np.empty((len(ROWS), n))
    for c in range(n):
        x = a[:, c].reshape(n_chains, D // n_chains)
        if transform == "exp_shift":
            x = np.exp(x - split(x).max())
        res = column(x)
        out[:, c] = [res[k] for k in ROWS]
    return out


def public(a, n_chains: int, transform: str = "identity") -> dict:
    s = columns(a, n_chains, transform)
    return {"rhat": np.sqrt(np.maximum(s[0], s[1])), "ess_bulk": s[2], "ess_tail": np.minimum(s[3], s[4]), "ess_mean": s[5],
            "mcse_mean": np.sqrt(s[7] / s[5]), "mean": s[6], "sd": np.sqrt(s[7])}
