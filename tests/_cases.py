"""Seeded parity cases shared by the golden-fixture generator and the GPU parity tests."""
from __future__ import annotations

import hashlib

import numpy as np

from pymc_bart_amd.sampler import PyBartSettings, PySampler, range_exponent


def make_case(name: str):
    if name.startswith("upstream/"):  # the same case under the upstream-semantics switches (PGB_COMPAT_*: both bits)
        c = make_case(name[len("upstream/"):])
        c.update(name=name, compat=3)
        return c
    rng = np.random.default_rng(abs(hash(name)) % (2 ** 31) if False else int(hashlib.sha1(name.encode()).hexdigest()[:8], 16))
    c = dict(name=name, m=10, P=10, steps=24, batch=(0.1, 0.1), rules=None, prior=None, seed=3415)
    if name == "cfg1_friedman":  # BASELINE.json configs[0]
        n, p = 500, 5
        X = rng.uniform(0, 1, (n, p))
        Y = (10 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 20 * (X[:, 2] - 0.5) ** 2 + 10 * X[:, 3]
             + 5 * X[:, 4] + rng.normal(0, 1, n))
        c.update(m=50, P=10, steps=40)
    elif name == "nan_onehot_prior":
        n, p = 5000, 8
        X = rng.normal(size=(n, p))
        X[:, 6] = rng.integers(0, 5, n)
        X[:, 7] = rng.integers(0, 2, n)
        X[rng.random(n) < 0.1, 1] = np.nan
        X[rng.random(n) < 0.3, 6] = np.nan
        Y = X[:, 0] * 2 + np.where(X[:, 7] > 0, 1.5, -1.5) + rng.normal(0, 0.5, n)
        rules = np.zeros(p, np.int32)
        rules[6:] = 1
        c.update(m=20, P=20, steps=40, rules=rules, prior=np.array([3, 1, 1, 1, 1, 0.5, 2, 2.0]))
    elif name == "ragged_1025":
        n, p = 1025, 3
        X = rng.normal(size=(n, p))
        Y = np.abs(X[:, 0]) + rng.normal(0, 0.1, n)
        c.update(m=7, P=6, steps=30, batch=(3, 2))
    elif name == "tiny_n3":
        n, p = 3, 2
        X = rng.normal(size=(n, p))
        Y = np.array([0.0, 1.0, 5.0])
        c.update(m=4, P=4, steps=16)
    elif name == "one_tree_two_particles":
        n, p = 300, 2
        X = rng.normal(size=(n, p))
        Y = X[:, 0] + rng.normal(0, 0.1, n)
        c.update(m=1, P=2, steps=30)
    elif name == "max_particles":
        n, p = 2100, 4
        X = rng.normal(size=(n, p))
        Y = np.sin(3 * X[:, 0]) * 4 + rng.normal(0, 0.3, n)
        c.update(m=6, P=64, steps=12)
    elif name == "particles_128":  # beyond one particle per lane: the 128-particle build of the library (two per lane)
        n, p = 2600, 5
        X = rng.normal(size=(n, p))
        X[rng.random(n) < 0.08, 2] = np.nan
        Y = np.sin(3 * X[:, 0]) * 3 + X[:, 1] * np.nan_to_num(X[:, 2]) + rng.normal(0, 0.3, n)
        c.update(m=5, P=128, steps=12)
    elif name == "particles_100_probit":  # an odd count above 64, a per-row family
        n, p = 1800, 4
        X = rng.normal(size=(n, p))
        Y = (rng.random(n) < 1 / (1 + np.exp(-2 * X[:, 0] + X[:, 1]))).astype(float)
        c.update(m=4, P=100, steps=10, family="bernoulli_probit")
    elif name == "categorical_k4_particles_100":  # K-vector leaves above 64 particles: both blocks of 64 have jobs whose
        n, p, K = 3000, 6, 4                      # extension outputs the likelihood pass lists (one lane per pair) and hands on
        X = rng.normal(size=(n, p))
        F = np.stack([X[:, 0], -X[:, 0], 1.5 * X[:, 1], 0 * X[:, 0]])
        pr = np.exp(F) / np.exp(F).sum(0)
        Y = (rng.random(n)[None, :] > np.cumsum(pr, axis=0)).sum(0).clip(0, K - 1).astype(float)
        c.update(m=4, P=100, steps=10, family="categorical", K=K)
    elif name == "duplicates":
        n, p = 4096, 3
        X = rng.integers(0, 3, (n, p)).astype(float)  # heavy ties, no jitter at this level
        Y = X[:, 0] - X[:, 1] + rng.normal(0, 0.2, n)
        rules = np.array([0, 1, 1], np.int32)
        c.update(m=8, P=12, steps=30, rules=rules)
    elif name == "deep_trees":
        n, p = 3000, 3
        X = rng.normal(size=(n, p))
        Y = np.sin(5 * X[:, 0]) + np.cos(3 * X[:, 1]) + rng.normal(0, 0.05, n)
        c.update(m=5, P=10, steps=20, alpha=0.999, beta=0.3)
    elif name == "probit_cfg4_small":  # BASELINE.json configs[3] at test size
        from scipy.special import ndtr
        n, p = 6000, 10
        X = rng.normal(size=(n, p))
        f = 1.5 * X[:, 0] - (X[:, 1] > 0) + 0.5 * X[:, 2] * X[:, 0]
        Y = (rng.random(n) < ndtr(f / 1.0)).astype(float)
        c.update(m=20, P=12, steps=30, family="bernoulli_probit")
    elif name == "logit_nan_onehot":
        n, p = 3000, 5
        X = rng.normal(size=(n, p))
        X[:, 3] = rng.integers(0, 3, n)
        X[:, 4] = 1.0  # constant one-hot column: every split attempt on it fails
        X[rng.random(n) < 0.15, 0] = np.nan
        X[rng.random(n) < 0.2, 4] = np.nan
        f = np.where(np.isnan(X[:, 0]), 0.0, 2 * X[:, 0]) + (X[:, 3] == 1) * 1.5
        Y = (rng.random(n) < 1 / (1 + np.exp(-f))).astype(float)
        c.update(m=10, P=16, steps=30, family="bernoulli_logit", rules=np.array([0, 0, 0, 1, 1], np.int32))
    elif name == "categorical_k3_reference":  # reference tests/test_bart.py:140-164 (shape=(3, 9))
        Y = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2], float)
        X = np.concatenate([Y[:, None], rng.integers(0, 6, size=(9, 4))], axis=1).astype(float)
        c.update(m=2, P=10, steps=60, family="categorical", K=3, rules=np.array([1] * 5, np.int32))
        n = 9
    elif name == "categorical_k4_cfg5_small":  # BASELINE.json configs[4] at test size
        n, p, K = 5000, 12, 4
        X = rng.normal(size=(n, p))
        X[rng.random(n) < 0.1, 2] = np.nan
        F = np.stack([X[:, 0], -X[:, 0], 1.5 * X[:, 1], 0 * X[:, 0]])
        pr = np.exp(F) / np.exp(F).sum(0)
        Y = (rng.random(n)[None, :] > np.cumsum(pr, axis=0)).sum(0).clip(0, K - 1).astype(float)
        c.update(m=15, P=12, steps=24, family="categorical", K=K)
    elif name == "categorical_k6_generic":  # more than 4 outputs: the run-time-K kernel instances
        n, p, K = 3000, 6, 6
        X = rng.normal(size=(n, p))
        X[rng.random(n) < 0.1, 1] = np.nan
        F = np.stack([X[:, 0], -X[:, 0], X[:, 2], -X[:, 2], 0.5 * X[:, 3], 0 * X[:, 0]])
        pr = np.exp(F) / np.exp(F).sum(0)
        Y = (rng.random(n)[None, :] > np.cumsum(pr, axis=0)).sum(0).clip(0, K - 1).astype(float)
        c.update(m=8, P=10, steps=20, family="categorical", K=K)
    elif name == "categorical_k12":  # beyond the former cap of 8 outputs (a 10-class softmax model raised): three tiles
        n, p, K = 2500, 7, 12
        X = rng.normal(size=(n, p))
        X[rng.random(n) < 0.1, 1] = np.nan
        X[:, 6] = rng.integers(0, 4, n)
        F = np.stack([np.cos(0.5 * k) * X[:, k % 4] + 0.3 * np.sin(k) * X[:, (k + 1) % 5] + 0.4 * (X[:, 6] == k % 4)
                      for k in range(K)])
        pr = np.exp(F) / np.exp(F).sum(0)
        Y = (rng.random(n)[None, :] > np.cumsum(pr, axis=0)).sum(0).clip(0, K - 1).astype(float)
        c.update(m=6, P=10, steps=16, family="categorical", K=K, rules=np.array([0, 0, 0, 0, 0, 0, 1], np.int32))
    elif name == "categorical_k16_linear":  # the largest K, linear leaves (run-time-K instances with LIN)
        n, p, K = 1500, 4, 16
        X = rng.normal(size=(n, p))
        F = np.stack([np.cos(0.4 * k) * X[:, k % 3] + 0.2 * k / K * X[:, 3] for k in range(K)])
        pr = np.exp(F) / np.exp(F).sum(0)
        Y = (rng.random(n)[None, :] > np.cumsum(pr, axis=0)).sum(0).clip(0, K - 1).astype(float)
        c.update(m=4, P=8, steps=12, family="categorical", K=K, response="linear")
    elif name in ("poisson_counts", "negbin_counts"):  # the count models of the PyMC-BART docs (log link)
        n, p = 4000, 5
        X = rng.normal(size=(n, p))
        X[rng.random(n) < 0.1, 2] = np.nan
        rate = np.exp(0.8 * X[:, 0] - 0.5 * (X[:, 1] > 0) + 1.0)
        if name == "poisson_counts":
            Y = rng.poisson(rate).astype(float)
            c.update(family="poisson_log")
        else:
            Y = rng.negative_binomial(2.0, 2.0 / (2.0 + rate)).astype(float)
            c.update(family="negbin_log", lik_params=[2.0])
        c.update(m=12, P=12, steps=30, bart_Y=np.log(Y + 0.5))
    elif name in ("linear_poisson", "mix_probit"):  # linear leaves with per-row families
        n, p = 3000, 3
        X = rng.uniform(-2, 2, size=(n, p))
        X[rng.random(n) < 0.1, 2] = np.nan
        f = np.where(X[:, 0] < 0, 1.0 * X[:, 0] + 0.5, -0.8 * X[:, 0] + 0.5)
        if name == "linear_poisson":
            Y = rng.poisson(np.exp(f)).astype(float)
            c.update(family="poisson_log", response="linear", bart_Y=np.log(Y + 0.5))
        else:
            from scipy.special import ndtr
            Y = (rng.random(n) < ndtr(f)).astype(float)
            c.update(family="bernoulli_probit", response="mix")
        c.update(m=8, P=12, steps=30)
    elif name == "gamma_positive":  # positive continuous response, log link
        n, p = 3000, 4
        X = rng.normal(size=(n, p))
        mean = np.exp(0.6 * X[:, 0] - 0.4 * (X[:, 1] > 0) + 0.5)
        Y = rng.gamma(3.0, mean / 3.0)
        c.update(family="gamma_log", lik_params=[3.0], m=10, P=12, steps=30, bart_Y=np.log(Y))
    elif name == "poisson_exposure":  # per-row offset of the linear predictor (log-exposure of a count model)
        n, p = 3000, 4
        X = rng.normal(size=(n, p))
        expo = rng.uniform(0.2, 5.0, n)
        lograte = 0.7 * X[:, 0] + 0.5
        Y = rng.poisson(expo * np.exp(lograte)).astype(float)
        c.update(family="poisson_log", m=10, P=12, steps=30, bart_Y=np.log((Y + 0.5) / expo), offset=np.log(expo))
    elif name in ("quantile_asymlaplace", "robust_student_t"):  # two-parameter per-row families
        n, p = 3500, 4
        X = rng.uniform(-2, 2, size=(n, p))
        X[rng.random(n) < 0.1, 3] = np.nan
        f = np.sin(2 * X[:, 0]) + 0.5 * X[:, 1]
        if name == "quantile_asymlaplace":
            Y = f + rng.normal(0, 0.2 + 0.3 * (X[:, 0] > 0), n)      # heteroscedastic: quantiles differ from the mean
            c.update(family="asymmetric_laplace", lik_params=[0.25, 0.9])
        else:
            Y = f + 0.2 * rng.standard_t(3, n)                        # heavy tails
            c.update(family="student_t", lik_params=[0.2, 3.0])
        c.update(m=10, P=12, steps=30)
    elif name in ("linear_response", "mix_response"):  # reference tests parametrise response=["constant","linear"]
        n, p = 3000, 4
        X = rng.uniform(-2, 2, size=(n, p))
        X[:, 3] = np.round(X[:, 3])            # ties
        X[rng.random(n) < 0.1, 1] = np.nan     # missing values in a regressor
        f = np.where(X[:, 0] < 0, 2 * X[:, 0] + 1, -1.5 * X[:, 0] + 1) + 0.5 * np.nan_to_num(X[:, 1])
        Y = f + rng.normal(0, 0.1, n)
        c.update(m=8, P=12, steps=30, response="linear" if name == "linear_response" else "mix")
    elif name in ("linear_mixed_rules", "mix_probit_mixed_rules", "categorical_k3_linear_mixed_rules"):
        # linear / mix leaves next to OneHot / Subset columns: a leaf regresses on whatever column its parent
        # split on (upstream: fast_linear_fit on X[idx, selected_predictor], whatever the rule, bart.py:88-103)
        n, p = 3000, 5
        X = rng.uniform(-2, 2, size=(n, p))
        X[:, 2] = rng.integers(0, 3, n)        # one-hot column
        X[:, 3] = rng.integers(0, 9, n)        # subset column, 9 categories
        X[:, 4] = 1.0                          # subset column with a single category (every split fails)
        X[rng.random(n) < 0.1, 1] = np.nan
        X[rng.random(n) < 0.1, 3] = np.nan
        f = np.where(X[:, 0] < 0, 2 * X[:, 0] + 1, -1.5 * X[:, 0] + 1) + (X[:, 2] == 1) + 0.3 * np.nan_to_num(X[:, 3])
        c.update(m=8, P=12, steps=30, rules=np.array([0, 0, 1, 2, 2], np.int32), prior=np.array([1.0, 1.0, 2.0, 2.0, 1.0]))
        if name == "linear_mixed_rules":
            Y = f + rng.normal(0, 0.2, n)
            c.update(response="linear")
        elif name == "mix_probit_mixed_rules":
            from scipy.special import ndtr
            Y = (rng.random(n) < ndtr(f - 1.0)).astype(float)
            c.update(family="bernoulli_probit", response="mix")
        else:
            K = 3
            F = np.stack([f, -f, 0.5 * (X[:, 2] == 2)])
            pr = np.exp(F) / np.exp(F).sum(0)
            Y = (rng.random(n)[None, :] > np.cumsum(pr, axis=0)).sum(0).clip(0, K - 1).astype(float)
            c.update(family="categorical", K=K, response="linear", steps=20)
    elif name.startswith("stump_first_"):
        # deviation 12 on the per-row families: tiny forest, three particles, and a key under which the untouched
        # stump wins the first tree updates -- the running sd of the accepted predictions is exactly 0 when leaf_sd
        # is first tuned, in k_ctrl AND in the likelihood pass's own copy of that rule (a 429-of-11 674 fuzz
        # divergence in round 3 when only one of the two had it)
        r77 = np.random.default_rng(77)
        n, p = 600, 3
        X = r77.normal(size=(n, p))
        f = 1.2 * X[:, 0]
        Yb = (r77.random(n) < 1 / (1 + np.exp(-f))).astype(float)
        Yc = np.clip(np.round(f + r77.normal(0, 0.5, n) + 1), 0, 2)
        Yp = r77.poisson(np.exp(f)).astype(float)
        c.update(m=2, P=3, steps=14, batch=(0.5, 0.5))
        if name == "stump_first_probit":
            Y = Yb
            c.update(family="bernoulli_probit", seed=0)
        elif name == "stump_first_categorical":
            Y = Yc
            c.update(family="categorical", K=3, seed=3)
        else:
            Y = Yp
            c.update(family="poisson_log", seed=0, bart_Y=np.log(Yp + 0.5))
    elif name == "meanscale_k2_reference":  # reference tests/test_bart.py:107-123 (shape=(2, 250))
        n, p = 250, 3
        X = rng.normal(0, 1, size=(n, p))
        Y = rng.normal(0, 1, size=n) * (0.5 + (X[:, 0] > 0)) + X[:, 1]
        c.update(m=2, P=10, steps=60, family="normal_meanscale", K=2)
    elif name == "meanscale_k2_linear":  # reference tests/test_bart.py:107-123 with response="linear"
        n, p = 250, 3
        X = rng.normal(0, 1, size=(n, p))
        Y = rng.normal(0, 1, size=n) * (0.5 + (X[:, 0] > 0)) + X[:, 1]
        c.update(m=2, P=10, steps=60, family="normal_meanscale", K=2, response="linear")
    elif name == "categorical_k3_mix":  # K-vector leaves with a slope per output, "mix", missing values
        n, p, K = 3000, 4, 3
        X = rng.uniform(-2, 2, size=(n, p))
        X[rng.random(n) < 0.1, 1] = np.nan
        F = np.stack([1.2 * X[:, 0], -1.2 * X[:, 0], 0.5 * np.nan_to_num(X[:, 1])])
        pr = np.exp(F) / np.exp(F).sum(0)
        Y = (rng.random(n)[None, :] > np.cumsum(pr, axis=0)).sum(0).clip(0, K - 1).astype(float)
        c.update(m=8, P=12, steps=24, family="categorical", K=K, response="mix")
    elif name == "categorical_k3_offset":  # additive multi-output model: per-row, per-output offsets of the predictors
        n, p, K = 2500, 4, 3
        X = rng.normal(size=(n, p))
        Z = rng.normal(size=n)                                   # a covariate handled by another model term
        off = np.stack([0.8 * Z, -0.8 * Z, np.zeros(n)])
        F = np.stack([X[:, 0], -X[:, 0], 0.7 * X[:, 1]]) + off
        pr = np.exp(F) / np.exp(F).sum(0)
        Y = (rng.random(n)[None, :] > np.cumsum(pr, axis=0)).sum(0).clip(0, K - 1).astype(float)
        c.update(m=8, P=10, steps=24, family="categorical", K=K, offset=off)
    elif name == "onehot_fail_nan":  # failed one-hot splits that shed NaN rows (Normal family)
        n, p = 2500, 3
        X = rng.normal(size=(n, p))
        X[:, 1] = 2.0
        X[rng.random(n) < 0.25, 1] = np.nan
        X[:, 2] = rng.integers(0, 2, n)
        Y = X[:, 0] + (X[:, 2] > 0) + rng.normal(0, 0.3, n)
        c.update(m=6, P=10, steps=30, rules=np.array([0, 1, 1], np.int32), prior=np.array([1.0, 3.0, 1.0]))
    elif name == "subset_rule":  # SubsetSplitRule (bart.py:100-103): categorical codes, set-valued splits
        n, p = 4000, 5
        X = rng.normal(size=(n, p))
        X[:, 2] = rng.integers(0, 7, n)       # 7 categories, effect of the set {1, 4, 6}
        X[:, 3] = rng.integers(0, 2, n)       # binary category
        X[:, 4] = 3.0                         # a single category: every subset split on it fails
        X[rng.random(n) < 0.1, 2] = np.nan
        X[rng.random(n) < 0.2, 4] = np.nan
        Y = (np.isin(X[:, 2], [1, 4, 6]) * 3.0 + (X[:, 3] > 0) * 1.0 + 0.5 * X[:, 0]
             + rng.normal(0, 0.3, n))
        c.update(m=12, P=14, steps=30, rules=np.array([0, 0, 2, 2, 2], np.int32),
                 prior=np.array([1.0, 1.0, 3.0, 1.0, 1.0]))
    else:
        raise KeyError(name)
    c.update(X=X, Y=Y)
    return c


CASES = ["cfg1_friedman", "nan_onehot_prior", "ragged_1025", "tiny_n3", "one_tree_two_particles",
         "max_particles", "particles_128", "particles_100_probit", "categorical_k4_particles_100", "duplicates", "deep_trees", "onehot_fail_nan", "probit_cfg4_small",
         "logit_nan_onehot", "categorical_k3_reference", "categorical_k4_cfg5_small",
         "meanscale_k2_reference", "subset_rule", "categorical_k6_generic", "categorical_k12", "categorical_k16_linear", "linear_response", "mix_response", "poisson_counts", "negbin_counts", "quantile_asymlaplace", "robust_student_t", "poisson_exposure", "gamma_positive", "linear_poisson", "mix_probit",
         "meanscale_k2_linear", "categorical_k3_mix", "categorical_k3_offset",
         "linear_mixed_rules", "mix_probit_mixed_rules", "categorical_k3_linear_mixed_rules",
         "stump_first_probit", "stump_first_categorical", "stump_first_poisson",
         # pgb_settings.compat = 3: fresh particles at log-weight 0, empty right leaves of one-hot splits
         "upstream/cfg1_friedman", "upstream/nan_onehot_prior", "upstream/onehot_fail_nan", "upstream/probit_cfg4_small",
         "upstream/categorical_k3_reference", "upstream/subset_rule", "upstream/linear_mixed_rules",
         "upstream/categorical_k3_linear_mixed_rules", "upstream/particles_128", "upstream/logit_nan_onehot"]


def run_case(c, backend, record_every: int = 1, checkpoint_at=(), setup=None):
    """Run the case on a backend; returns everything the two backends must agree on.
    ``setup``: called with every freshly built sampler before anything else is done with it (e.g. to hand the
    data over again in another layout).
    ``checkpoint_at``: step indices before which the chain is checkpointed, its sampler destroyed
    and a freshly built sampler restored from the image (must not change anything); a dict
    ``{step: backend}`` moves the chain to ANOTHER backend there (the image belongs to none:
    include/pgbart_image.h)."""
    X, Y = c["X"], c["Y"]
    p = X.shape[1]
    family = c.get("family", "normal")
    st = PyBartSettings.from_data(X, c.get("bart_Y", Y), m=c["m"], num_particles=c["P"], seed=c["seed"], batch=c["batch"],
                                  alpha=c.get("alpha", 0.95), beta=c.get("beta", 2.0), family=family,
                                  n_outputs=c.get("K", 1), response=c.get("response", "constant"),
                                  compat=c.get("compat", 0))
    rules = np.zeros(p, np.int32) if c["rules"] is None else c["rules"]
    prior = np.ones(p) if c["prior"] is None else c["prior"]
    s = PySampler(st, X, Y, rules, prior, backend=backend)
    if setup is not None:
        setup(s)
    if c.get("offset") is not None:
        s.set_offset(c["offset"])
    weights0 = s.split_weights()
    sig_rng = np.random.default_rng(99)
    sums, vis, trees, split_vars = [], [], [], []
    half = c.get("tune_steps", c["steps"] // 2)   # ("tune_steps": the schedule of a longer run, cut short)
    for it in range(c["steps"]):
        if it in checkpoint_at:
            blob = s.checkpoint()
            del s
            if isinstance(checkpoint_at, dict):
                backend = checkpoint_at[it]
            s = PySampler(st, X, Y, rules, prior, backend=backend)
            if setup is not None:
                setup(s)
            if c.get("offset") is not None:
                s.set_offset(c["offset"])
            s.restore(blob)
        sig = float(0.5 + sig_rng.random())  # sigma moves like a Gibbs/NUTS neighbour
        s.set_likelihood([sig] if family == "normal" else c.get("lik_params", []))
        stv, vi = s.step(tune=it < half)
        if it % record_every == 0:
            sums.append(stv)
            vis.append(vi)
            ta = s.export_trees(0)
            parts = [ta.tree_id, ta.node_off, ta.var, ta.left, ta.right, ta.count, ta.split.view(np.int64),
                     ta.value.ravel().view(np.int64)]
            if c.get("response", "constant") != "constant":  # linear leaves are part of the fingerprint
                parts += [ta.slope.ravel().view(np.int64), ta.xbar.view(np.int64), ta.svar]
            trees.append(np.concatenate(parts))
            split_vars.append(np.asarray(ta.var)[np.asarray(ta.var) >= 0].astype(np.int64))
    forest = s.export_trees(1)
    ctr = s.counters.as_dict()
    ctr.pop("slots")
    return dict(sum_trees=np.array(sums), vi=np.array(vis), trees=trees, forest=forest, counters=ctr,
                state=s.state(), split_weights=s.split_weights(), sampler=s, split_vars=split_vars,
                split_weights_init=weights0)


def digest(res) -> dict:
    """Compact, exact fingerprint of a run (what the golden fixture stores)."""
    h = hashlib.sha256()
    h.update(res["sum_trees"].tobytes())
    h.update(res["vi"].astype(np.int32).tobytes())
    for t in res["trees"]:
        h.update(np.ascontiguousarray(t).tobytes())
    f = res["forest"]
    for a in (f.var, f.left, f.right, f.count, f.split, f.value):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(res["split_weights"].tobytes())
    h.update(np.asarray(res["state"]["leaf_sd"]).tobytes())
    return {
        "sha256": h.hexdigest(),
        "counters": {k: int(v) for k, v in res["counters"].items()},
        "last_sum_trees_head": np.asarray(res["sum_trees"][-1]).ravel()[:8].tolist(),
        "leaf_sd": float(res["state"]["leaf_sd"][0]),
        "iter": int(res["state"]["iter"]),
    }


def random_case(seed, large=False, compat=0):
    """A random configuration for the fuzz parity test: sizes around the chunk / wave boundaries,
    every family, every split rule, NaNs, ties, priors, batch sizes, alpha / beta.
    `large`: hundreds of chunks per pass (work items beyond one per workgroup, particle groups of
    more than one particle), few trees and steps so that the oracle still answers in seconds."""
    rng = np.random.default_rng(seed)
    fam = rng.choice(["normal", "normal", "normal", "bernoulli_probit", "bernoulli_logit", "categorical", "normal_meanscale",
                      "poisson_log", "negbin_log", "asymmetric_laplace", "student_t", "gamma_log"])
    n = int(rng.choice([3, 17, 255, 256, 257, 1023, 1024, 1025, 2049, 5000, 20000]))
    p = int(rng.integers(1, 9))
    m = int(rng.integers(1, 12))
    P = int(rng.choice([2, 3, 5, 10, 20, 40, 64, 65, 97, 128]))  # (> 64: the two-particles-per-lane build)
    if large:
        n = int(rng.choice([50_000, 131_072, 200_001, 400_000, 1_048_577]))
        m = int(rng.integers(1, 5))
        P = int(rng.choice([5, 20, 40, 64, 128]))
    X = rng.normal(size=(n, p))
    rules = np.zeros(p, np.int32)
    for j in range(p):
        r = rng.random()
        if r < 0.2:
            X[:, j] = rng.integers(0, int(rng.integers(1, 6)), n); rules[j] = 1
        elif r < 0.35:
            X[:, j] = rng.integers(0, int(rng.integers(1, 9)), n); rules[j] = 2
        elif r < 0.45:
            X[:, j] = np.round(X[:, j])  # heavy ties, continuous rule
        if rng.random() < 0.3:
            X[rng.random(n) < rng.uniform(0.01, 0.5), j] = np.nan
    f = np.nan_to_num(X[:, 0]) * 1.5 + (np.nan_to_num(X[:, -1]) > 0)
    K = 1
    if fam == "normal":
        Y = f + rng.normal(0, 0.5, n)
    elif fam.startswith("bernoulli"):
        Y = (rng.random(n) < 1 / (1 + np.exp(-f))).astype(float)
    elif fam in ("poisson_log", "negbin_log"):
        Y = rng.poisson(np.exp(np.clip(f, -3, 3))).astype(float)
    elif fam in ("asymmetric_laplace", "student_t"):
        Y = f + rng.standard_t(3, n) * 0.5
    elif fam == "gamma_log":
        Y = rng.gamma(2.0, np.exp(np.clip(f, -3, 3)) / 2.0) + 1e-6
    elif fam == "categorical":
        # classes that DEPEND on the covariates (Gumbel-max over logits that fan out with f): with a pure-noise
        # response the stump wins nearly every update and the K-vector growth paths are hardly exercised
        K = int(rng.integers(2, 17)) if rng.random() < 0.35 else int(rng.integers(2, 8))  # (up to PGB_MAX_OUTPUTS = 16)
        logits = np.stack([f * (k - 0.5 * (K - 1)) for k in range(K)]) + rng.gumbel(size=(K, n))
        Y = np.argmax(logits, axis=0).astype(float)
    else:
        K = 2; Y = f + rng.normal(0, 1, n) * (0.5 + (np.nan_to_num(X[:, 0]) > 0))
    batch = (float(rng.choice([0.1, 0.34, 1.0])), float(rng.choice([0.1, 0.5])))
    response = "constant"
    if not rules.any():
        response = str(rng.choice(["constant", "linear", "mix"]))
    elif rng.random() < 0.25:  # linear / mix leaves next to one-hot / subset columns
        response = str(rng.choice(["linear", "mix"]))
    extra = {}
    if fam in ("poisson_log", "negbin_log"):
        extra["bart_Y"] = np.log(Y + 0.5)
        if fam == "negbin_log":
            extra["lik_params"] = [float(rng.uniform(0.3, 5.0))]
    if fam == "gamma_log":
        extra["bart_Y"] = np.log(Y)
        extra["lik_params"] = [float(rng.uniform(0.5, 5.0))]
    if fam == "asymmetric_laplace":
        extra["lik_params"] = [float(rng.uniform(0.1, 2.0)), float(rng.uniform(0.05, 0.95))]
    if fam == "student_t":
        extra["lik_params"] = [float(rng.uniform(0.1, 2.0)), float(rng.uniform(1.0, 30.0))]
    if fam not in ("normal", "categorical", "normal_meanscale") and rng.random() < 0.3:
        extra["offset"] = rng.normal(0, 0.3, n)  # another additive term of the linear predictor
    elif fam in ("categorical", "normal_meanscale") and rng.random() < 0.3:
        extra["offset"] = rng.normal(0, 0.3, (K, n))  # ... of every linear predictor of a K-vector model
    return dict(**extra, name=f"fuzz{seed}", compat=int(compat), response=response, X=X, Y=Y, m=m, P=P, steps=int(rng.integers(2, 5) if large else rng.integers(4, 14)), batch=batch, rules=rules,
                prior=rng.uniform(0.5, 3.0, p), seed=int(rng.integers(0, 2**31)), family=fam, K=K,
                alpha=float(rng.choice([0.95, 0.5, 0.999])), beta=float(rng.choice([2.0, 0.5, 1.0])))


def random_cap_case(seed):
    """A random configuration at the tree-size limits for the fuzz parity test (tests/test_caps_gpu.py): the data of
    cap_case at row counts around the chunk / wave boundaries, 2 .. 128 particles, missing values, the upstream
    switches, alpha = 0.9999 with beta = 0 or 0.05 (P(split) >= 0.81 down to depth 64).  Every tree is re-sampled at
    every step, so cap_reach reads the run."""
    rng = np.random.default_rng([77, int(seed)])
    n = int(rng.choice([128, 129, 255, 257, 1025, 2049]))
    # the one-hot column needs rows in 65 codes and more: the small row counts mostly take the continuous columns
    kind = str(rng.choice(["bushy", "chain", "both"], p=[0.8, 0.1, 0.1] if n < 1025 else [0.3, 0.3, 0.4]))
    fam = str(rng.choice(["normal", "normal", "bernoulli_probit", "categorical", "poisson_log"]))
    if kind == "chain" and fam == "bernoulli_probit":   # (leaves only the stump on the pure one-hot column)
        fam = "normal"
    response = str(rng.choice(["constant", "constant", "linear", "mix"]))
    P = int(rng.choice([2, 10, 64, 65, 128], p=[0.1, 0.3, 0.2, 0.2, 0.2]))   # (two particles mostly keep the stump)
    nan_frac = float(rng.choice([0.0, 0.0, 0.05, 0.3]))
    compat = int(rng.choice([0, 0, 1, 2, 3]))
    beta = float(rng.choice([0.0, 0.05], p=[0.75, 0.25]))
    if kind != "bushy" or n < 255:   # P(split) = 0.81 at depth 64 under beta = 0.05: no chain of 64, no 255 nodes from 129 rows
        beta = 0.0
    code = rng.integers(0, 100, n).astype(float)
    z = rng.normal(size=(n, 2))
    fc = np.sin(0.7 * code) + 0.02 * code
    fz = np.sin(3 * z[:, 0]) + np.where(z[:, 1] < 0, z[:, 1], -0.5 * z[:, 1])
    if kind == "chain":
        X, rules, prior, f = code[:, None].copy(), np.array([1], np.int32), np.ones(1), fc
    elif kind == "bushy":
        X, rules, prior, f = z.copy(), np.zeros(2, np.int32), np.ones(2), fz
    else:
        X, rules, prior, f = np.stack([code, z[:, 1]], axis=1), np.array([1, 0], np.int32), np.array([20.0, 1.0]), fc + fz
    if nan_frac > 0:
        X[rng.random(n) < nan_frac, 0] = np.nan
    K, extra = 1, {}
    if fam == "normal":
        Y = f + rng.normal(0, 0.3, n)
    elif fam == "bernoulli_probit":
        from scipy.special import ndtr
        Y = (rng.random(n) < ndtr(2.0 * f)).astype(float)
    elif fam == "poisson_log":
        Y = rng.poisson(np.exp(np.clip(f, -3, 3))).astype(float)
        extra["bart_Y"] = np.log(Y + 0.5)
    else:
        K = int(rng.integers(2, 6))
        logits = np.stack([2.0 * f * (k - 0.5 * (K - 1)) for k in range(K)]) + rng.gumbel(size=(K, n))
        Y = np.argmax(logits, axis=0).astype(float)
    return dict(**extra, name=f"capfuzz{seed}", kind=kind, variant=fam, X=X, Y=Y, m=int(rng.integers(1, 4 if P < 64 else 3)), P=P,
                steps=int(rng.integers(6, 13 if P < 64 else 9)), batch=(1.0, 1.0), rules=rules, prior=prior, seed=int(rng.integers(0, 2 ** 31)),
                family=fam, K=K, response=response, compat=compat, alpha=0.9999, beta=beta)


# ------------------------------------------------------------------ handle history (tests/test_handle_history*.py)
# "A handle's history leaves no trace": after any sequence of setter calls, refused calls and loads the chain continues
# bit for bit like a fresh handle given the same image and the same final inputs.

HISTORY_STEPS = 12


def make_history_case(kind, n=1025, P=10, rules="continuous", seed=0):
    """The small model the history tests drive: n = 1025 rows (two chunks, a single row in the second), p = 5, m = 10
    trees in batches of 3 (a tree lives through three changes of the inputs before it is rebuilt), 12 asteps, half of
    them tuning.  `kind`: family, or family:K, with an optional /linear or /mix response."""
    fam, _, response = kind.partition("/")
    fam, _, K = fam.partition(":")
    K = int(K) if K else 1
    rng = np.random.default_rng(int(hashlib.sha1(f"history {kind} {n} {rules} {seed}".encode()).hexdigest()[:8], 16))
    p = 5
    X = rng.uniform(-2, 2, size=(n, p))
    rl = np.zeros(p, np.int32)
    prior = np.array([1.0, 1.0, 2.0, 2.0, 1.0])
    if rules == "mixed":  # the rules of linear_mixed_rules: one-hot, subset (9 categories), subset with a single category
        X[:, 2] = rng.integers(0, 3, n)
        X[:, 3] = rng.integers(0, 9, n)
        X[:, 4] = 1.0
        X[rng.random(n) < 0.1, 3] = np.nan
        rl = np.array([0, 0, 1, 2, 2], np.int32)
    X[rng.random(n) < 0.1, 1] = np.nan
    f = np.where(X[:, 0] < 0, 1.2 * X[:, 0] + 0.5, -0.8 * X[:, 0] + 0.5) + 0.4 * (X[:, 2] > 0)
    c = dict(name=f"history/{kind}", X=X, m=10, P=P, steps=HISTORY_STEPS, batch=(3, 3), rules=rl, prior=prior, seed=2718 + seed,
             family=fam, K=K, response=response or "constant", lik=lambda r: [])
    if fam == "normal":
        Y = f + rng.normal(0, 0.3, n)
        c.update(lik=lambda r: [float(0.5 + r.random())])
    elif fam in ("bernoulli_probit", "bernoulli_logit"):
        Y = (rng.random(n) < 1 / (1 + np.exp(-1.5 * f))).astype(float)
    elif fam in ("poisson_log", "negbin_log"):
        Y = rng.poisson(np.exp(f)).astype(float)
        c.update(bart_Y=np.log(Y + 0.5))
        if fam == "negbin_log":
            c.update(lik=lambda r: [float(r.uniform(1.0, 4.0))])
    elif fam == "gamma_log":
        Y = rng.gamma(3.0, np.exp(f) / 3.0) + 1e-6
        c.update(bart_Y=np.log(Y), lik=lambda r: [float(r.uniform(1.0, 4.0))])
    elif fam == "asymmetric_laplace":
        Y = f + rng.normal(0, 0.3, n)
        c.update(lik=lambda r: [float(r.uniform(0.2, 0.5)), float(r.uniform(0.2, 0.9))])
    elif fam == "student_t":
        Y = f + 0.2 * rng.standard_t(3, n)
        c.update(lik=lambda r: [float(r.uniform(0.15, 0.4)), float(r.uniform(2.0, 8.0))])
    elif fam == "categorical":
        logits = np.stack([f * (k - 0.5 * (K - 1)) for k in range(K)]) + rng.gumbel(size=(K, n))
        Y = np.argmax(logits, axis=0).astype(float)
    elif fam == "normal_meanscale":
        Y = f + rng.normal(0, 1, n) * (0.5 + (X[:, 0] > 0))
    else:
        raise KeyError(kind)
    c.update(Y=Y)
    return c


def moving_inputs(c, swap=False, none_at=4, zero_at=8):
    """The schedule of a model whose other terms move at every astep, as PGBART.astep drives the handle: a Normal
    model gets `set_response(y - o_t)` and a moving sigma, a per-row family `set_offset(o_t)` ([K][n] for K-vector
    leaves) and moving parameters.  One step inside the run resets the offset (`None`), another sets an all-zero
    array (`swap` exchanges the two): both mean "no offset", through has_off = 0 and through adding 0.0."""
    n, K, fam = c["X"].shape[0], c["K"], c["family"]

    def schedule(it):
        r = np.random.default_rng(1000 + it)
        o = r.normal(0, 0.3, n if K == 1 else (K, n))
        inp = {"lik": c["lik"](r)}
        if fam == "normal":
            inp["response"] = c["Y"] - o
            return inp
        a, b = (zero_at, none_at) if swap else (none_at, zero_at)
        inp["offset"] = None if it == a else np.zeros_like(o) if it == b else o
        return inp

    return schedule


def history_sampler(c, backend, in_force):
    """A FRESH handle of `backend` with the inputs in force (what the setters were last given)."""
    X, Y = c["X"], c["Y"]
    st = PyBartSettings.from_data(X, c.get("bart_Y", Y), m=c["m"], num_particles=c["P"], seed=c["seed"], batch=c["batch"],
                                  family=c["family"], n_outputs=c["K"], response=c["response"], compat=c.get("compat", 0))
    s = PySampler(st, in_force.get("X", X), in_force.get("response", Y), in_force.get("rules", c["rules"]), c["prior"],
                  backend=backend)
    if c.get("setup") is not None:
        c["setup"](s, in_force)
    if in_force.get("offset") is not None:
        s.set_offset(in_force["offset"])
    if in_force.get("lik") is not None:
        s.set_likelihood(in_force["lik"])
    return s


def apply_inputs(c, s, inp):
    if "response" in inp:
        s.set_response(inp["response"])
    if "offset" in inp:
        s.set_offset(inp["offset"])
    if c.get("apply") is not None:
        c["apply"](s, inp)
    if "lik" in inp:
        s.set_likelihood(inp["lik"])


def step_record(c, s, tune):
    """One astep and everything it gives back, as bytes."""
    stv, vi = s.step(tune)
    ta = s.export_trees(0)
    parts = [ta.tree_id, ta.node_off, ta.var, ta.left, ta.right, ta.count, ta.split.view(np.int64),
             ta.value.ravel().view(np.int64), ta.slope.ravel().view(np.int64), ta.xbar.view(np.int64), ta.svar]
    return dict(sum_trees=np.ascontiguousarray(stv).tobytes(), vi=np.asarray(vi, np.int32).tobytes(),
                trees=b"".join(np.ascontiguousarray(a).tobytes() for a in parts))


def end_record(s):
    from pymc_bart_amd.image import ImageHeader

    stt = s.state()
    ctr = s.counters.as_dict()
    ctr.pop("slots")
    blob = bytearray(s.checkpoint())
    if s.backend.lib.backend_name == "hip-gfx950":
        # (`slots` counts launches, idle ones included: it belongs to the handle, not to the chain -- pgbart_image.h)
        off = ImageHeader.ctr.offset + type(s.counters).slots.offset
        blob[off: off + 8] = bytes(8)
    return dict(leaf_sd=np.asarray(stt["leaf_sd"]).tobytes(), iter=stt["iter"], lower=stt["lower"],
                split_weights=s.split_weights().tobytes(), counters=ctr, image=bytes(blob))


def run_schedule(c, schedule, backend, start=0, image=None, in_force=None, cuts=()):
    """Steps `start` .. steps - 1 of the schedule.  start > 0: on a fresh handle built with `in_force` that loads
    `image`.  Before every step in `cuts` the image and the inputs in force are kept (the setters of that step have
    not been called yet)."""
    in_force = dict(in_force or {})
    if start == 0:
        first = schedule(0)
        s = history_sampler(c, backend, {k: v for k, v in first.items() if k in ("response", "X", "rules")})
    else:
        s = history_sampler(c, backend, in_force)
        s.restore(image)
    steps, kept = [], {}
    half = c["steps"] // 2
    for it in range(start, c["steps"]):
        if it in cuts:
            kept[it] = (s.checkpoint(), dict(in_force))
        inp = schedule(it)
        apply_inputs(c, s, inp)
        in_force.update(inp)
        steps.append(step_record(c, s, it < half))
    return dict(steps=steps, end=end_record(s), kept=kept, sampler=s)


def assert_same_run(a, b, what, first=0, ignore=()):
    assert len(a["steps"]) == len(b["steps"])
    for i, (x, y) in enumerate(zip(a["steps"], b["steps"])):
        for k in x:
            assert x[k] == y[k], f"{what}: {k} differs at step {first + i}"
    for k in a["end"]:
        if k == "image" and a["end"][k] != b["end"][k]:
            from pymc_bart_amd.image import ChainImage, differing_fields

            ia, ib = ChainImage.parse(a["end"][k]), ChainImage.parse(b["end"][k])
            if ia.writer != ib.writer:  # two backends: everything but who wrote it and the launch counter
                bad = [f for f in differing_fields(ia, ib) if f not in ignore]
                assert bad == [], f"{what}: the end images differ in {bad}"
                continue
            raise AssertionError(f"{what}: the end images differ in {differing_fields(ia, ib) or 'bytes outside the chain fields'}")
        assert a["end"][k] == b["end"][k], f"{what}: {k} differs after the last step"


def check_schedule(c, schedule, backend, cuts, reference=None, ignore=()):
    """The two assertions of the history tests: (1) `backend` equals `reference` (a run of the same schedule on the
    oracle) on every step's outputs and at the end; (2) at every cut a fresh handle of `backend` -- built with the
    inputs in force there, then `restore(image)` -- continues identically to the end and ends with the same image.
    `ignore`: image fields the two backends cannot share (the compiled family is the oracle's callback family: the
    family code in the settings)."""
    full = run_schedule(c, schedule, backend, cuts=cuts)
    assert sorted(full["kept"]) == sorted(cuts)
    if reference is not None:
        assert_same_run(full, reference, f"{c['name']}: {backend.lib.backend_name} against the oracle", ignore=ignore)
    for cut in cuts:
        image, in_force = full["kept"][cut]
        tail = run_schedule(c, schedule, backend, start=cut, image=image, in_force=in_force)
        whole = dict(steps=full["steps"][cut:], end=full["end"])
        assert_same_run(tail, whole, f"{c['name']}: fresh handle from the image before step {cut}", first=cut)
    return full


def set_data_rc(s, X, rules, prior, ldx=None):
    """`pgb_set_data` on a live sampler through the ABI: returns (code, message) instead of raising."""
    lib, mem = s.backend.lib, s.backend.mem
    X = np.ascontiguousarray(X, np.float64)
    rules = np.ascontiguousarray(rules, np.int32)
    prior = np.ascontiguousarray(prior, np.float64)
    xd = mem.from_host(X)
    rc = lib.lib.pgb_set_data(s._h, mem.ptr(xd), X.shape[1] if ldx is None else ldx, rules.ctypes.data, prior.ctypes.data)
    msg = lib.lib.pgb_last_error()
    if hasattr(mem, "synchronize"):
        mem.synchronize()
    del xd
    s._rules = rules
    return rc, (msg.decode() if msg and rc != 0 else "")


# ------------------------------------------------------------------ wide design matrices (tests/test_wide*.py)
# The sampler's device code branches on the column count p: the split-variable draw in blocks of 64 lanes (one loop
# up to 64, four blocks requested together up to 256, the loop again beyond), the 64-bit carry between the blocks
# while the prefix sums are rebuilt in tuning, the 32 x 32 tiles of the transpose, one workgroup per column in the
# checks, `vi` copied in trips of 256 and laid out in 64-byte lines, the split prior staged in a row buffer when
# p < n_pad and in an allocation of its own when p >= n_pad.  Every p below sits on one of those edges.
WIDE_P = [31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 1023, 1024, 1025, 1500]
WIDE_VARIANTS = ["normal", "linear", "probit_mix", "categorical_k3", "normal_p100"]
WIDE_HOT = (0, 31, 32, 63, 64, 65, 255, 256, 257)   # ... and p - 1
WIDE_ROWS = {257: 1025, 1025: 1025}                # two chunks (n_pad = 2048: p = 1025 < n_pad); every other p: 130 rows
# (p, variant) -> the first seed whose oracle run meets check_wide_reach, where seed 0 does not
WIDE_SEEDS = {(63, "categorical_k3"): 1, (64, "linear"): 1, (255, "normal"): 1, (256, "normal"): 1, (257, "categorical_k3"): 3,
              (1023, "linear"): 2, (1024, "normal"): 3, (1024, "linear"): 1, (1025, "normal"): 1, (1025, "linear"): 2,
              (1025, "probit_mix"): 13, (1025, "categorical_k3"): 9, (1500, "normal"): 2, (1500, "linear"): 5,
              (1500, "probit_mix"): 7, (1500, "categorical_k3"): 1, (1500, "normal_p100"): 1}


def wide_layout(p):
    """(hot columns, one-hot column or None, subset column or None, NaN column) of the p-column wide case."""
    hot = sorted({h for h in WIDE_HOT + (p - 1,) if 0 <= h < p})
    late = [h for h in hot if h > 256]
    if len(late) < 2:
        late = [h for h in hot if h > 64]
    onehot, subset = (late[0], late[-1]) if len(late) >= 2 else (None, None)
    return hot, onehot, subset, p - 1   # (p - 1 is hot, and the last column of the last transpose tile)


def wide_case(p, variant, seed):
    """n = 130 rows (1025 for two widths), m = 3 trees all re-sampled at every step, 12 steps of which 6 tune:
    iter > m is reached while tuning, so the split-variable draw runs on the weights being rebuilt.  Column j is
    scaled by 10^(j % 7 - 3); the hot columns carry the signal and a large split prior."""
    rng = np.random.default_rng([int(p), WIDE_VARIANTS.index(variant), int(seed)])
    n = WIDE_ROWS.get(p, 130)
    hot, onehot, subset, nancol = wide_layout(p)
    scale = 10.0 ** (np.arange(p) % 7 - 3)
    Z = rng.normal(size=(n, p))
    rules = np.zeros(p, np.int32)
    if onehot is not None:
        Z[:, onehot] = rng.integers(0, 3, n)
        Z[:, subset] = rng.integers(0, 7, n)
        rules[onehot], rules[subset] = 1, 2
    X = Z * scale
    if onehot is not None:
        X[:, onehot], X[:, subset] = Z[:, onehot], Z[:, subset]   # category codes are not scaled
    X[rng.random(n) < 0.15, nancol] = np.nan
    prior = np.ones(p)
    prior[hot] = max(4.0, 0.25 * (p - len(hot)) / len(hot))       # the hot columns: a fifth of the prior mass or more
    f = np.zeros(n)
    for k, h in enumerate(hot):
        z = np.nan_to_num(Z[:, h])
        sgn = 1.0 if k % 2 == 0 else -1.0
        if h == onehot:
            f += 1.5 * sgn * (z == 1)
        elif h == subset:
            f += 1.5 * sgn * np.isin(z, [1, 4])
        elif variant == "linear" and h >= 32:
            f += 0.8 * sgn * np.where(z < 0, z, -0.5 * z)
        else:
            f += 1.5 * sgn * (z > 0)
    c = dict(name=f"wide/p{p}/{variant}", m=3, P=10, steps=12, batch=(1.0, 1.0), rules=rules, prior=prior,
             seed=1000 + int(seed), beta=0.7, X=X)
    if variant in ("normal", "linear", "normal_p100"):
        c.update(Y=f + rng.normal(0, 0.3, n))
        if variant == "linear":
            c.update(response="linear")
        elif variant == "normal_p100":
            c.update(P=100)
    elif variant == "probit_mix":
        from scipy.special import ndtr
        c.update(Y=(rng.random(n) < ndtr(f)).astype(float), family="bernoulli_probit", response="mix")
    elif variant == "categorical_k3":
        logits = np.stack([f, -f, np.zeros(n)]) + rng.gumbel(size=(3, n))
        c.update(Y=np.argmax(logits, axis=0).astype(float), family="categorical", K=3)
    else:
        raise KeyError(variant)
    return c


def make_wide(p, variant):
    return wide_case(p, variant, WIDE_SEEDS.get((p, variant), 0))


def wide_reach(c, res):
    """What a run of a wide case reached, from its result alone: the 64-blocks of columns its exported trees split
    on, whether tuning changed a split weight of the last block, `vi` beyond column 255, splits on the NaN column."""
    p = c["X"].shape[1]
    sv = np.concatenate(res["split_vars"]) if len(res["split_vars"]) else np.zeros(0, np.int64)
    last = 64 * ((p - 1) // 64)
    changed = np.flatnonzero(res["split_weights"] != res["split_weights_init"])
    return dict(p=p, n_blocks=(p + 63) // 64, blocks=sorted({int(v) // 64 for v in sv}), n_splits=int(sv.size),
                beyond_31=int((sv >= 32).sum()), last_column=int((sv == p - 1).sum()),
                nan_column=int((sv == wide_layout(p)[3]).sum()),
                tuned_in_last_block=int((changed >= last).sum()),
                vi_beyond_255=int(np.asarray(res["vi"])[:, 256:].sum()))


def check_wide_reach(c, res):
    """The conditions a wide case exists for (no pytest here: the golden generator calls it too)."""
    r = wide_reach(c, res)
    assert r["blocks"] == list(range(r["n_blocks"])), f"{c['name']}: no split in some 64-block of the columns: {r}"
    assert r["beyond_31"] > 0 or r["p"] <= 32, f"{c['name']}: no split beyond the first transpose tile: {r}"
    assert r["last_column"] > 0 and r["nan_column"] > 0, f"{c['name']}: no split on the last (NaN) column: {r}"
    assert r["tuned_in_last_block"] > 0, f"{c['name']}: tuning did not reach the last 64-block: {r}"
    assert r["vi_beyond_255"] > 0 or r["p"] <= 256, f"{c['name']}: vi is zero beyond column 255: {r}"
    return r



# ------------------------------------------------------------------ tree-size limits (tests/test_caps*.py)
# The sampler stops a tree at PGB_MAX_NODES = 255 nodes (node tables of 255 entries, the last index 254; a row's
# label is a byte, the ordinal of its leaf -- 0 .. 127 in a full tree -- or 255 for a dropped row) and at
# PGB_MAX_DEPTH = 64 (prior_leaf[64]; a node at depth 64 is a leaf with probability 1).  With alpha = 0.9999, beta = 0
# a node splits whenever it can, so a few steps of a tiny forest drive the accepted trees into both limits: the
# guards of the control kernel, label tables filled for 128 leaves next to label 255, the full particle tables, the
# export and the chain image.
CAP_MAX_NODES, CAP_MAX_DEPTH = 255, 64
CAP_KINDS = ["chain", "bushy", "bushy128", "bushy129", "both"]
CAP_VARIANTS = ["normal", "linear", "mix", "probit", "categorical_k3", "categorical_k5", "normal_p100", "normal_p128",
                "upstream", "categorical_k12_linear"]
CAP_ROWS = {"chain": 1000, "bushy": 300, "bushy128": 128, "bushy129": 129, "both": 2000}
# every (kind, variant) of the matrix.  Not on the pure one-hot column (chain): probit, which leaves only the stump
# there.  Under compat = 3 index 254 of every full tree on that column is an EMPTY right leaf, so chain / upstream is
# held to full trees with leaves that would still split (cap_targets: "full"); the column next to a continuous one,
# kind "both", ends full trees in a leaf that holds rows.  The two smallest row counts that can fill 255 nodes run
# the Normal family and the unrolled K-vector instance.
# K = 12 with linear leaves (three tiles of the run-time-K instances): two classes carry the signal, at logits of
# +-4 f, the other ten sit at -3 -- with a signal spread over all classes the accepted trees stay stumps.
ALL_CAPS = ([("chain", v) for v in CAP_VARIANTS if v != "probit"] + [("bushy", v) for v in CAP_VARIANTS]
            + [(k, v) for k in ("bushy128", "bushy129") for v in ("normal", "categorical_k3")]
            + [("both", v) for v in CAP_VARIANTS])
# (kind, variant) -> the first seed whose oracle run meets check_cap_reach, where seed 0 does not
CAP_SEEDS = {("both", "normal"): 3, ("both", "probit"): 9, ("both", "categorical_k5"): 14, ("both", "normal_p128"): 1}


def cap_targets(kind, variant):
    """(node cap, depth cap, dropped rows): the limits a case exists for.  Under compat = 3 an empty right leaf of a
    one-hot split grows, so the one-hot column fills the node table long before depth 64: that variant is held to the
    node cap alone -- on the pure one-hot column to "full": a 255-node tree with leaves that would still split, whose
    last node is an empty leaf."""
    node = kind != "chain" or (variant == "upstream" and "full")
    depth = kind in ("chain", "both") and variant != "upstream"
    return node, depth, kind == "both"


def cap_case(kind, variant, seed):
    """m = 2 trees (one for the 100 / 128 particle variants, except on "both": with a single tree none of 32 keys
    reaches depth 64 there), all re-sampled at every step, 8 steps of which 4 tune,
    alpha = 0.9999, beta = 0: P(split) = 0.9999 at every depth below 64.
    chain: one one-hot column of 100 codes -- every split peels one code off to the left, the rest goes right.
    bushy*: two continuous columns, 300 / 128 / 129 rows.
    both: the one-hot column (split prior 20, 10 % missing) next to a continuous column, 2000 rows."""
    rng = np.random.default_rng([CAP_KINDS.index(kind), CAP_VARIANTS.index(variant), int(seed)])
    n = CAP_ROWS[kind]
    if kind == "chain":
        code = rng.integers(0, 100, n).astype(float)
        X, rules, prior = code[:, None], np.array([1], np.int32), np.ones(1)
        f = np.sin(0.7 * code) + 0.02 * code
    elif kind.startswith("bushy"):
        X, rules, prior = rng.normal(size=(n, 2)), np.zeros(2, np.int32), np.ones(2)
        f = np.sin(3 * X[:, 0]) + np.where(X[:, 1] < 0, X[:, 1], -0.5 * X[:, 1])
    elif kind == "both":
        code = rng.integers(0, 100, n).astype(float)
        f = np.sin(0.7 * code) + 0.02 * code
        code[rng.random(n) < 0.1] = np.nan
        z = rng.normal(size=n)
        X, rules, prior = np.stack([code, z], axis=1), np.array([1, 0], np.int32), np.array([20.0, 1.0])
        f = np.where(np.isnan(code), 0.0, f) + np.where(z < 0, z, -0.5 * z)
    else:
        raise KeyError(kind)
    c = dict(name=f"cap/{kind}/{variant}", kind=kind, variant=variant, m=2, P=10, steps=8, batch=(1.0, 1.0), rules=rules,
             prior=prior, seed=2000 + int(seed), alpha=0.9999, beta=0.0, X=X)
    if variant in ("normal", "linear", "mix", "normal_p100", "normal_p128", "upstream"):
        c.update(Y=f + rng.normal(0, 0.3, n))
        if variant in ("linear", "mix"):
            c.update(response=variant)
        elif variant == "normal_p100":
            c.update(P=100, m=2 if kind == "both" else 1)
        elif variant == "normal_p128":
            c.update(P=128, m=2 if kind == "both" else 1)
        elif variant == "upstream":
            c.update(compat=3)
    elif variant == "probit":
        from scipy.special import ndtr
        c.update(Y=(rng.random(n) < ndtr(2.0 * f)).astype(float), family="bernoulli_probit")
    elif variant in ("categorical_k3", "categorical_k5"):
        K = int(variant[-1])
        logits = np.stack([2.0 * f * (k - 0.5 * (K - 1)) for k in range(K)]) + rng.gumbel(size=(K, n))
        c.update(Y=np.argmax(logits, axis=0).astype(float), family="categorical", K=K)
    elif variant == "categorical_k12_linear":
        logits = np.full((12, n), -3.0)
        logits[0], logits[1] = 4.0 * f, -4.0 * f
        logits += rng.gumbel(size=(12, n))
        c.update(Y=np.argmax(logits, axis=0).astype(float), family="categorical", K=12, response="linear")
    else:
        raise KeyError(variant)
    return c


def make_cap(kind, variant):
    return cap_case(kind, variant, CAP_SEEDS.get((kind, variant), 0))


def tree_depths(left, right, var):
    """Depth of every node of one tree (tree-local child indices), by a walk from the root."""
    depth = np.full(len(var), -1, np.int64)
    todo = [(0, 0)]
    while todo:
        k, d = todo.pop()
        assert depth[k] < 0, "a node is reached twice"
        depth[k] = d
        if var[k] >= 0:
            todo += [(int(left[k]), d + 1), (int(right[k]), d + 1)]
    assert (depth >= 0).all(), "a node is not reached from the root"
    return depth


def step_trees(c, packed):
    """The trees of one entry of run_case's `trees` (the arrays of a step's export_trees(0), concatenated) as
    (var, left, right, count) per tree.  Every tree is re-sampled at every step: the batch holds m trees."""
    m = c["m"]
    packed = np.asarray(packed)
    off = packed[m: 2 * m + 1].astype(np.int64)
    assert off[0] == 0 and np.array_equal(np.sort(packed[:m]), np.arange(m)), "not a batch of all m trees"
    N = int(off[-1])
    var, left, right, count = (packed[2 * m + 1 + k * N: 2 * m + 1 + (k + 1) * N].astype(np.int64) for k in range(4))
    return [(var[a:b], left[a:b], right[a:b], count[a:b]) for a, b in zip(off[:-1], off[1:])]


def forest_trees(forest):
    off = np.asarray(forest.node_off, np.int64)
    return [tuple(np.asarray(getattr(forest, f))[a:b].astype(np.int64) for f in ("var", "left", "right", "count"))
            for a, b in zip(off[:-1], off[1:])]


def tree_at_caps(tree, n):
    """What one exported tree says about the two limits."""
    var, left, right, count = tree
    depth = tree_depths(left, right, var)
    leaf = var < 0
    full = len(var) == CAP_MAX_NODES
    return dict(nodes=len(var), depth=int(depth.max()),
                # the last node index is a live leaf, and growth was still wanted: the cap is what stopped it
                node_cap=bool(full and leaf[-1] and count[-1] > 0 and (leaf & (depth < CAP_MAX_DEPTH) & (count >= 2)).any()),
                depth_cap=bool((leaf & (depth == CAP_MAX_DEPTH) & (count >= 2)).any()),
                full_open=bool(full and (leaf & (depth < CAP_MAX_DEPTH) & (count >= 2)).any()),
                dropped=bool(full and count[leaf].sum() < n),
                open_leaves=int((leaf & (depth < CAP_MAX_DEPTH) & (count >= 2)).sum()),
                held_at_depth=int((leaf & (depth == CAP_MAX_DEPTH) & (count >= 2)).sum()),
                empty_leaves=int((leaf & (count == 0)).sum()))


def cap_reach(c, res):
    """What a run of a cap case reached, from its exports alone (every step's accepted batch, not only the final
    forest): see check_cap_reach.  `first_full`: the first step after which a tree at a limit is stored (`first_deep`: at the depth limit)."""
    n = c["X"].shape[0]
    stats, first_full, first_deep = [], None, None
    for it, packed in enumerate(res["trees"]):
        for t in step_trees(c, packed):
            s = tree_at_caps(t, n)
            stats.append(s)
            if first_full is None and (s["full_open"] or s["depth_cap"]):
                first_full = it
            if first_deep is None and s["depth_cap"]:
                first_deep = it
    st0 = PyBartSettings.from_data(c["X"], c.get("bart_Y", c["Y"]), m=c["m"], num_particles=c["P"])
    return dict(max_nodes=max(s["nodes"] for s in stats), max_depth=max(s["depth"] for s in stats),
                node_cap=sum(s["node_cap"] for s in stats), full_open=sum(s["full_open"] for s in stats), depth_cap=sum(s["depth_cap"] for s in stats),
                dropped=sum(s["dropped"] for s in stats), both_in_one_tree=sum(s["node_cap"] and s["depth_cap"] for s in stats),
                open_leaves=max(s["open_leaves"] for s in stats), held_at_depth=max(s["held_at_depth"] for s in stats),
                empty_leaves=max(s["empty_leaves"] for s in stats), first_full=first_full, first_deep=first_deep,
                saturations=int(res["counters"]["saturations"]),
                leaf_sd_tuned=bool(np.any(np.asarray(res["state"]["leaf_sd"]) != st0.init_leaf_sd)))


def cap_prefix(c, steps):
    """The first `steps` steps of the case, tuning as the whole run tunes."""
    return dict(c, steps=int(steps), tune_steps=c["steps"] // 2)


def check_cap_reach(c, res):
    """The conditions a cap case exists for (no pytest here: the golden generator calls it too)."""
    r = cap_reach(c, res)
    node, depth, dropped = cap_targets(c["kind"], c["variant"])
    assert not node or r["full_open" if node == "full" else "node_cap"] > 0, \
        f"{c['name']}: no accepted tree is stopped by the node cap: {r}"
    assert not depth or r["depth_cap"] > 0, f"{c['name']}: no accepted tree holds rows in a leaf at depth 64: {r}"
    assert not dropped or r["dropped"] > 0, f"{c['name']}: no 255-node tree has dropped rows: {r}"
    assert r["saturations"] == 0, f"{c['name']}: fixed-point saturation: {r}"
    assert r["leaf_sd_tuned"], f"{c['name']}: tuning did not change leaf_sd: {r}"
    return r


# ------------------------------------------------------------------ saturating steps (tests/test_saturation*.py)
# Every term of the sampler's sums is quantised to fixed point (pgb_quant, include/pgbart_spec.h): a term beyond the
# declared range 2^range_exp is clamped to +-2^50 and COUNTED in counters.saturations, and PySampler turns a moved
# counter into an error.  The cases below make that counter move: a response that leaves the range for one step
# (set_response, as the other terms of an additive model move it), for the whole run, or a range set below the
# data's.  One tree is re-sampled per step, so a step's events are those of one tree update -- on the device, a row
# pass that starts a tree (INIT) and a pass of its own that ends it (the lone FINAL).  The two */two_per_step cases
# re-sample two: the first tree of a step ends in the pass that starts the second (FINAL + INIT in one launch).
SAT_CASES = ["sat/normal_outliers", "sat/normal_linear", "sat/normal_all_rows_top", "sat/normal_one_tree", "sat/edge_exact",
             "sat/poisson_small_range", "sat/probit_small_range", "sat/categorical_k3", "sat/categorical_k6",
             "sat/particles_100", "sat/probit_two_per_step", "sat/categorical_k3_two_per_step"]
SAT_OUTLIER_CASES = ("sat/normal_outliers", "sat/normal_linear", "sat/particles_100")
SAT_OUTLIER_ROWS = (0, 3, 255, 256, 512, 1023, 1024)   # chunk edges of 256 and 1024 rows; 1024: the lone row of the second chunk
SAT_OUTLIER_MULT = (1.5, -2.0, 3.0, -3.0, -1.0001, 2.5, 1.25)   # (-1.0001: back inside once sum_trees_noi is taken off)
# name -> the first seed whose oracle run meets check_sat_reach, where seed 0 does not
SAT_SEEDS = {}
SAT_QLIM = 2.0 ** 50


def sat_scales(n, range_exp):
    """pgb_make_scales (include/pgbart_spec.h): (frac, c1, c2)."""
    bits = 0
    while (1 << bits) < n + 1:
        bits += 1
    frac = min(61 - bits, 50)
    return frac, 2.0 ** (frac - range_exp), 2.0 ** (frac - 2 * range_exp)


def sat_quant(x, scale):
    """pgb_quant on arrays: (the integers, the number of terms counted).  NaN -> 0, counted."""
    t = np.asarray(x, np.float64) * scale
    nan = np.isnan(t)
    t = np.where(nan, 0.0, t)
    over = np.abs(t) > SAT_QLIM
    q = np.rint(np.clip(t, -SAT_QLIM, SAT_QLIM)).astype(np.int64)   # (rint: to nearest even, exact below 2^51)
    return q, int(nan.sum() + over.sum())


def sat_case(name, seed):
    rng = np.random.default_rng([SAT_CASES.index(name), int(seed)])
    c = dict(name=name, m=5, P=10, steps=8, batch=(0.1, 0.1), rules=None, prior=None, seed=4000 + int(seed), range_exp=None,
             responses={}, sat_steps=(), beta=1.0)
    if name in SAT_OUTLIER_CASES:
        # steps 0-2 clean; before step 3 seven rows leave +-2^range_exp, both signs; before step 4 they are back
        n, p = 1025, 3
        X = rng.uniform(-2, 2, size=(n, p))
        Y = np.where(X[:, 0] < 0, 2 * X[:, 0] + 1, -1.5 * X[:, 0] + 1) + rng.normal(0, 0.3, n)
        out = Y.copy()
        out[list(SAT_OUTLIER_ROWS)] = np.array(SAT_OUTLIER_MULT) * 2.0 ** range_exponent(Y)
        c.update(responses={3: out, 4: Y}, sat_steps=(3,), hot_rows=SAT_OUTLIER_ROWS)
        if name == "sat/normal_linear":
            c.update(response="linear")
        elif name == "sat/particles_100":
            c.update(P=100, m=3)
    elif name == "sat/normal_all_rows_top":
        # every row at 64 * 2^range_exp, then at 2 * 2^range_exp, then the data: n = 2049 has frac = 49, so a term
        # x c1 saturates beyond 2 * 2^range_exp and a squared term beyond sqrt(2) * 2^range_exp.  The sums B, C and E0
        # of the first update are n * 2^50.  sum_trees itself stays in range -- leaf values are drawn from the clamped
        # sums -- so A is not among them (sat/categorical_k*: A and Ax at n * 2^50 in the first update)
        n, p = 2049, 2
        X = rng.normal(size=(n, p))
        Y = X[:, 0] + rng.normal(0, 0.3, n)
        top = 2.0 ** range_exponent(Y)
        c.update(m=3, steps=8, responses={0: np.full(n, 64.0 * top), 1: np.full(n, 2.0 * top), 2: Y}, sat_steps=(0, 1))
    elif name == "sat/normal_one_tree":
        # a few rows out of range for the whole run, no tuning: every term counted is one of A, B, C, E0 of the
        # row pass that starts a tree, which NumPy recounts from the returned sum_trees and the exported trees
        n, p = 257, 2
        X = rng.normal(size=(n, p))
        clean = np.sin(2 * X[:, 0]) + rng.normal(0, 0.2, n)
        Y = clean.copy()
        Y[[0, 100, 255, 256]] = np.array([1.5, -1.004, 1.002, -1.01]) * 2.0 ** 4   # (three of them within reach of a leaf value)
        c.update(m=4, batch=(1, 1), steps=12, tune_steps=0, range_exp=4, bart_Y=clean, sat_steps="all",
                 hot_rows=(0, 100, 255, 256))
    elif name == "sat/edge_exact":
        # responses exactly +-2^range_exp are not counted (the compare is strict), their neighbours beyond are.  The
        # settings are sized on a response of dyadic values in +- pairs: init_leaf is exactly 0, so with one tree
        # r = y exactly at every update
        n, p, e = 130, 2, 4
        X = rng.normal(size=(n, p))
        half = np.round(rng.normal(0, 1, n // 2) * 64) / 64
        clean = np.concatenate([half, -half])
        Y = clean.copy()
        top = 2.0 ** e
        edge = {0: top, 1: -top, 2: np.nextafter(top, np.inf), 3: np.nextafter(-top, -np.inf), 64: np.nextafter(top, 0.0),
                129: np.nextafter(-top, 0.0)}
        for i, v in edge.items():
            Y[i] = v
        clean[sorted(set(edge) | {(i + n // 2) % n for i in edge})] = 0.0   # (the edge rows and their partners: the mean stays exactly 0)
        c.update(m=1, batch=(1, 1), steps=4, range_exp=e, bart_Y=clean, sat_steps="all", hot_rows=(2, 3), edge=edge)
    elif name == "sat/poisson_small_range":
        n, p = 1025, 3
        X = rng.normal(size=(n, p))
        Y = rng.poisson(np.exp(np.clip(1 + 1.5 * X[:, 0], -3, 6))).astype(float)
        c.update(family="poisson_log", bart_Y=np.log(Y + 0.5), range_exp=1, sat_steps=tuple(range(1, 8)))   # (step 0: sum_trees is init_sum < 2)
    elif name == "sat/probit_small_range":
        # range 2^0 with leaf_sd = 1.5: the running sd of a tree's predictions (tuning) leaves it next to sum_trees
        from scipy.special import ndtr
        n, p = 255, 3
        X = rng.normal(size=(n, p))
        Y = (rng.random(n) < ndtr(1.5 * X[:, 0])).astype(float)
        c.update(family="bernoulli_probit", range_exp=0, sat_steps=tuple(range(1, 10)), steps=10, tune_steps=8, m=4, batch=(1, 1))
    elif name == "sat/probit_two_per_step":
        # range 2^-2, below most of what moves: a tuning step of two tree updates counts sum_trees twice, the running sd
        # in the pass that starts the second tree and in the lone FINAL -- more events than three of those can give
        from scipy.special import ndtr
        n, p = 255, 3
        X = rng.normal(size=(n, p))
        Y = (rng.random(n) < ndtr(1.5 * X[:, 0])).astype(float)
        c.update(family="bernoulli_probit", range_exp=-2, sat_steps="all", steps=6, tune_steps=4, m=4, batch=(2, 2))
    elif name == "sat/categorical_k3_two_per_step":
        n, p, K = 257, 3, 3
        X = rng.normal(size=(n, p))
        logits = np.stack([1.5 * X[:, 0] * (k - 0.5 * (K - 1)) for k in range(K)]) + rng.gumbel(size=(K, n))
        Y = np.argmax(logits, axis=0).astype(float)
        c.update(family="categorical", K=K, range_exp=-4, sat_steps="all", steps=6, tune_steps=4, m=4, batch=(2, 2))
    elif name in ("sat/categorical_k3", "sat/categorical_k6"):
        K = int(name[-1])
        n, p = (1025, 3) if K == 3 else (257, 3)
        X = rng.normal(size=(n, p))
        logits = np.stack([1.5 * X[:, 0] * (k - 0.5 * (K - 1)) for k in range(K)]) + rng.gumbel(size=(K, n))
        Y = np.argmax(logits, axis=0).astype(float)
        c.update(family="categorical", K=K, range_exp=-1, sat_steps="all", m=4, batch=(1, 1))
    else:
        raise KeyError(name)
    c.update(X=X, Y=Y)
    return c


def make_sat(name):
    return sat_case(name, SAT_SEEDS.get(name, 0))


def sat_settings(c):
    X = c["X"]
    return PyBartSettings.from_data(X, c.get("bart_Y", c["Y"]), m=c["m"], num_particles=c["P"], seed=c["seed"], batch=c["batch"],
                                    alpha=c.get("alpha", 0.95), beta=c.get("beta", 2.0), family=c.get("family", "normal"),
                                    n_outputs=c.get("K", 1), response=c.get("response", "constant"),
                                    compat=c.get("compat", 0), range_exp=c.get("range_exp"))


def step_keeping_outputs(s, tune, how="host"):
    """One astep as PySampler runs it, keeping the outputs of a step whose saturation check raises:
    (sum_trees, vi, the PGBError or None).  `how`: "host" -- pgb_step_host and PySampler's own check, as `step(tune)`;
    "device" -- `step(tune, fetch=False)`, sum_trees read from the device buffer; "async" -- `step_async(tune, 1)` and
    `sync()`, sum_trees read from the chain image."""
    import ctypes as C

    from pymc_bart_amd import _abi

    lib, mem = s.backend.lib, s.backend.mem
    K, n = s.settings.n_outputs, s.settings.n
    err = None
    if how == "host":
        st = mem.host_result(K * n)
        s._steps += 1
        s._check(lib.lib.pgb_step_host(s._h, int(bool(tune)), st.ctypes.data, s._vi.ctypes.data, C.byref(s.counters)),
                 "pgb_step_host")
        try:
            s._check_saturation()
        except _abi.PGBError as e:
            err = e
    else:
        try:
            if how == "device":
                s.step(tune, fetch=False)
            else:
                assert how == "async", how
                s.step_async(tune, 1)
                s.sync()
        except _abi.PGBError as e:
            if "saturation events" not in str(e):
                raise
            err = e
        if how == "device":
            st = np.asarray(mem.to_host(s.sum_trees_device()), np.float64).ravel()[: K * n].copy()
        else:
            from pymc_bart_amd.image import ChainImage

            st = np.array(ChainImage.parse(s.checkpoint()).sum_trees, np.float64).ravel()
    return (st.reshape(K, n) if K > 1 else st), s._vi.copy(), err


def run_sat_case(c, backend, checkpoint_at=(), setup=None, how="host"):
    """run_case for a saturating case: the same loop, driven by the case's schedule of responses (`responses`:
    {step: y}, handed to set_response before that step), through steps that raise.  Next to everything run_case
    returns: per step `sat` (counters.saturations after it), `raised` (whether the step raised the saturation error)
    and `raised_count` (the count in its text, or -1); `exports`, the decoded trees of every step.
    `checkpoint_at` as in run_case (the fresh sampler is built on the response in force)."""
    import re

    X, y = c["X"], c["Y"]
    p = X.shape[1]
    family = c.get("family", "normal")
    st = sat_settings(c)
    rules = np.zeros(p, np.int32) if c["rules"] is None else c["rules"]
    prior = np.ones(p) if c["prior"] is None else c["prior"]
    s = PySampler(st, X, y, rules, prior, backend=backend)
    if setup is not None:
        setup(s)
    weights0 = s.split_weights()
    sig_rng = np.random.default_rng(99)
    sums, vis, trees, split_vars, sat, raised, raised_count, exports = [], [], [], [], [], [], [], []
    half = c.get("tune_steps", c["steps"] // 2)
    for it in range(c["steps"]):
        if it in checkpoint_at:
            blob = s.checkpoint()
            del s
            if isinstance(checkpoint_at, dict):
                backend = checkpoint_at[it]
            s = PySampler(st, X, y, rules, prior, backend=backend)
            if setup is not None:
                setup(s)
            s.restore(blob)
        if it in c["responses"]:
            y = c["responses"][it]
            s.set_response(y)
        sig = float(0.5 + sig_rng.random())
        s.set_likelihood([sig] if family == "normal" else c.get("lik_params", []))
        stv, vi, err = step_keeping_outputs(s, it < half, how)
        sums.append(stv)
        vis.append(vi)
        sat.append(int(s.counters.saturations))
        raised.append(err is not None)
        mt = re.match(r"(\d+) fixed-point saturation events by astep \d+:", str(err)) if err is not None else None
        assert err is None or mt is not None, str(err)
        raised_count.append(int(mt.group(1)) if mt else -1)
        ta = s.export_trees(0)
        parts = [ta.tree_id, ta.node_off, ta.var, ta.left, ta.right, ta.count, ta.split.view(np.int64),
                 ta.value.ravel().view(np.int64)]
        if c.get("response", "constant") != "constant":
            parts += [ta.slope.ravel().view(np.int64), ta.xbar.view(np.int64), ta.svar]
        trees.append(np.concatenate(parts))
        exports.append(ta.decoded())
        split_vars.append(np.asarray(ta.var)[np.asarray(ta.var) >= 0].astype(np.int64))
    forest = s.export_trees(1)
    ctr = s.counters.as_dict()
    ctr.pop("slots")
    return dict(sum_trees=np.array(sums), vi=np.array(vis), trees=trees, forest=forest, counters=ctr,
                state=s.state(), split_weights=s.split_weights(), sampler=s, split_vars=split_vars,
                split_weights_init=weights0, sat=sat, raised=raised, raised_count=raised_count, exports=exports,
                settings=st, response_in_force=y)


def sat_digest(res) -> dict:
    """`digest` plus the per-step saturation counts and raised flags (what tests/golden/sat_runs.json stores)."""
    d = digest(res)
    d.update(sat=[int(v) for v in res["sat"]], raised=[bool(v) for v in res["raised"]],
             raised_count=[int(v) for v in res["raised_count"]])
    return d


def sat_events(res):
    """Events of every step (one tree update each): the differences of the counter."""
    return np.diff(np.concatenate([[0], np.asarray(res["sat"], np.int64)]))


def sat_response_at(c, it):
    y = c["Y"]
    for k in sorted(c["responses"]):
        if k <= it:
            y = c["responses"][k]
    return y


def sat_route(ta, t, X):
    """Leaf (node index in `ta`) of every row of X in tree `t` of an export: continuous rules, no missing values."""
    base = int(ta.node_off[t])
    node = np.full(X.shape[0], base, np.int64)
    for _ in range(256):
        j = ta.var[node]
        inner = j >= 0
        if not inner.any():
            return node
        rows = np.flatnonzero(inner)
        left = X[rows, j[rows]] <= ta.split[node[rows]]
        node[rows] = base + np.where(left, ta.left[node[rows]], ta.right[node[rows]])
    raise AssertionError("the walk does not end")


def sat_recount_first(c, st):
    """The terms counted by the first tree update of a Normal case, from include/pgbart_spec.h alone: sum_trees is
    init_sum and the tree being replaced predicts init_leaf in every row.  Returns (count, sums A, B, C, E0)."""
    y = sat_response_at(c, 0)
    n = y.shape[0]
    _, c1, c2 = sat_scales(n, st.range_exp)
    stv = np.full(n, st.init_sum)
    return sat_recount_update(stv, np.full(n, st.init_leaf), y, c1, c2)


def sat_recount_update(stv, o, y, c1, c2):
    """The sums that start a Normal tree update, written from include/pgbart_spec.h alone (pgb_quant, pgb_make_scales,
    "r = y - sum_trees_noi"): with sum_trees `stv` and the replaced tree's predictions `o`, [U] sum_trees_noi =
    sum_trees - old_tree.predict(), r = y - noi, and e = r - o is the residual under the current tree; the terms are
    st c1 (A), r c1 (B), r^2 c2 (C), e^2 c2 (E0).  Returns (terms counted, A, B, C, E0)."""
    noi = stv - o
    r = y - noi
    e = r - o
    (A, na), (B, nb), (Cq, nc), (E0, ne) = sat_quant(stv, c1), sat_quant(r, c1), sat_quant(r * r, c2), sat_quant(e * e, c2)
    return na + nb + nc + ne, int(A.sum()), int(B.sum()), int(Cq.sum()), int(E0.sum())


def sat_terms_per_row(stv, o, y, c1, c2):
    """sat_recount_update's count, row by row."""
    noi = stv - o
    r = y - noi
    e = r - o
    return sum((np.abs(x * k) > SAT_QLIM).astype(np.int64) for x, k in ((stv, c1), (r, c1), (r * r, c2), (e * e, c2)))


def sat_outlier_step_per_row(c, res):
    """Terms counted per row in the saturating step of an outlier case: the tree replaced there is still the initial
    stump, or (constant leaves) its last export is routed in NumPy."""
    it = c["sat_steps"][0]
    st = res["settings"]
    n = c["X"].shape[0]
    _, c1, c2 = sat_scales(n, st.range_exp)
    t = int(res["exports"][it].tree_id[0])
    before = [j for j in range(it) if int(res["exports"][j].tree_id[0]) == t]
    if not before:
        o = np.full(n, st.init_leaf)
    else:
        assert c.get("response", "constant") == "constant"
        old = res["exports"][before[-1]]
        o = old.value[sat_route(old, 0, c["X"]), 0]
    return sat_terms_per_row(np.asarray(res["sum_trees"][it - 1]), o, sat_response_at(c, it), c1, c2)


def sat_recount_run(c, res):
    """Events of every step of a Normal case without tuning and with constant leaves, recounted in NumPy from the
    previous step's returned sum_trees, the previous export of the tree being replaced and the response in force."""
    assert c.get("family", "normal") == "normal" and c.get("tune_steps", 1) == 0 and c.get("response", "constant") == "constant"
    st = res["settings"]
    n, m = c["X"].shape[0], c["m"]
    _, c1, c2 = sat_scales(n, st.range_exp)
    last = {}     # tree -> (export, index in it)
    out = []
    for it in range(c["steps"]):
        ta = res["exports"][it]
        assert ta.n_trees == 1
        t = int(ta.tree_id[0])
        stv = np.full(n, st.init_sum) if it == 0 else np.asarray(res["sum_trees"][it - 1])
        if t in last:
            old, k = last[t]
            o = old.value[sat_route(old, k, c["X"]), 0]
        else:
            o = np.full(n, st.init_leaf)
        out.append(sat_recount_update(stv, o, sat_response_at(c, it), c1, c2)[0])
        last[t] = (ta, 0)
    return np.array(out, np.int64)


def sat_recount_sum_trees(c, res):
    """Per-row families: the events of every step that come from sum_trees itself (st c1 of every output, counted by
    the row pass that starts the update), recounted from the previous step's returned sum_trees.  What a tuning step
    counts beyond them is the running sd of the new tree's predictions; a log-likelihood term cannot saturate."""
    st = res["settings"]
    n, K = c["X"].shape[0], c.get("K", 1)
    _, c1, _ = sat_scales(n, st.range_exp)
    out = []
    for it in range(c["steps"]):
        stv = np.full((K, n), st.init_sum) if it == 0 else np.asarray(res["sum_trees"][it - 1]).reshape(K, n)
        out.append(sat_quant(stv, c1)[1])
    return np.array(out, np.int64)


def sat_reach(c, res):
    n = c["X"].shape[0]
    ev = sat_events(res)
    half = c.get("tune_steps", c["steps"] // 2)
    moved = tuple(int(i) for i in np.flatnonzero(ev > 0))
    r = dict(events=ev.tolist(), moved=moved, n=n,
             nodes=[int(np.diff(ta.node_off).max()) for ta in res["exports"]], tune_steps=half)
    if c.get("family", "normal") != "normal":
        base = sat_recount_sum_trees(c, res)
        r.update(from_sum_trees=base.tolist(), from_running_sd=(ev - base).tolist())
    return r


def check_sat_reach(c, res):
    """The conditions a saturating case exists for, evaluated on the oracle's run (no pytest here: the golden generator
    calls it too)."""
    r = sat_reach(c, res)
    name, n, ev = c["name"], r["n"], np.asarray(r["events"])
    steps = range(c["steps"])
    named = c["sat_steps"]
    if named == "all":
        named = tuple(steps)
    assert r["moved"] == tuple(named), f"{name}: the counter moved in steps {r['moved']}, the case names {named}: {r}"
    assert res["raised"] == [it in named for it in steps], f"{name}: raised {res['raised']}"
    assert [k for k in res["raised_count"] if k >= 0] == [int(ev[it]) for it in named], f"{name}: {res['raised_count']} {r}"
    if name.endswith("two_per_step"):
        # a step's events: sum_trees at the start of both updates (the first recounted, the second at most K n), the
        # running sd at the end of the first (in the pass that starts the second) and of the second (the lone FINAL,
        # at most K n): what is left over all bounds is a lower bound of the events of the FINAL + INIT pass
        Kn = c.get("K", 1) * n
        fused = ev - np.asarray(r["from_sum_trees"]) - 2 * Kn
        r.update(running_sd_of_first_update_at_least=fused.tolist())
        assert fused[:r["tune_steps"]].max() > 0, f"{name}: the running sd of a step's first update is not shown to saturate: {r}"
        assert np.all(ev[r["tune_steps"]:] <= 2 * Kn), f"{name}: {r}"
        return r
    if name not in ("sat/normal_all_rows_top", "sat/categorical_k3", "sat/categorical_k6"):
        assert all(0 < ev[it] < n for it in named), f"{name}: events not strictly between 0 and n = {n}: {r}"
    assert any(r["nodes"][it] > 1 for it in named), f"{name}: only stumps grown on saturated sums: {r}"
    if name in SAT_OUTLIER_CASES:   # the lone row of the second chunk is among the rows counted, and only moved rows are
        per_row = sat_outlier_step_per_row(c, res)
        assert per_row.sum() == ev[named[0]] and per_row[n - 1] > 0, f"{name}: {per_row[list(c['hot_rows'])]} {r}"
        assert set(np.flatnonzero(per_row).tolist()) <= set(c["hot_rows"]) and np.count_nonzero(per_row) >= 6, f"{name}: {r}"
        r.update(terms_of_the_moved_rows=per_row[list(c["hot_rows"])].tolist())
    if c.get("family", "normal") != "normal":
        sd = np.asarray(r["from_running_sd"])
        assert np.all(sd >= 0) and np.all(sd[r["tune_steps"]:] == 0), f"{name}: events beyond sum_trees outside tuning: {r}"
        assert np.asarray(r["from_sum_trees"]).sum() > 0, f"{name}: sum_trees never saturates: {r}"
        if name != "sat/poisson_small_range":
            assert sd.sum() > 0, f"{name}: the running sd never leaves the range: {r}"
        if c.get("K", 1) > 1:   # outputs 1 .. K-1 are counted on their own (Ax): A and every Ax at n * 2^50 in the first update
            st = res["settings"]
            q, cnt = sat_quant(np.full((c["K"], n), st.init_sum), sat_scales(n, st.range_exp)[1])
            assert cnt == ev[0] == c["K"] * n and np.all(np.abs(q.sum(axis=1)) == n * 2 ** 50), f"{name}: {r}"
    if name == "sat/normal_all_rows_top":
        st = res["settings"]
        frac, c1, c2 = sat_scales(n, st.range_exp)
        assert frac < 50
        cnt, A, B, Cq, E0 = sat_recount_first(c, st)
        assert (B, Cq, E0) == (n * 2 ** 50,) * 3 and cnt == ev[0] == 3 * n, f"{name}: {(cnt, A, B, Cq, E0)} {r}"
        assert 0 < ev[1] < ev[0] and ev[1] % n == 0, f"{name}: {r}"   # (2 * 2^range_exp: fewer terms per row than 64 *)
        r.update(per_row=[int(e) // n for e in ev[:2]])
    return r
