"""Wide design matrices -- CPU half: the oracle on the column-count edges of the sampler (tests/_cases.py: WIDE_P).

Every other small sampler test has p <= 12; the device code branches on p at 64, 256, 1024 (against n_pad) and at
the 32-column tiles of the transpose.  The GPU half (tests/test_wide_gpu.py) holds the HIP library to the oracle's
chains at those widths; here the oracle's side is pinned:

* every (p, variant) reaches what it is for (`check_wide_reach`: splits in every 64-block of the columns, on the
  last column with its missing values, tuning in the last block, `vi` beyond column 255) and reproduces its committed
  fingerprint (tests/golden/wide_runs.json, written by tests/golden/make_oracle_golden.py);
* chain images, which hold arrays of length p, resume bit for bit;
* the split-variable draw equals NumPy's inverse CDF on thresholds placed exactly on, just below and just above the
  prefix sums (the vectors the device probe is given in tests/test_spec_device_gpu.py);
* oracle-independent: under a flat likelihood the split variables of a p = 300 chain follow the split prior, in a
  chi-square test over (block of 64) x (lane 0, lanes 1..62, lane 63) that a draw one lane or one block off fails.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
from scipy import stats

from _cases import WIDE_P, WIDE_VARIANTS, check_wide_reach, digest, make_wide, run_case
from pymc_bart_amd.sampler import PyBartSettings, PySampler

WIDE_GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "wide_runs.json")))
ALL_WIDE = [(p, v) for p in WIDE_P for v in WIDE_VARIANTS]
WIDE_IDS = [f"p{p}-{v}" for p, v in ALL_WIDE]


@pytest.mark.parametrize("p,variant", ALL_WIDE, ids=WIDE_IDS)
def test_wide_case_reaches_its_edges_and_reproduces_its_fingerprint(oracle, p, variant):
    c = make_wide(p, variant)
    res = run_case(c, oracle)
    check_wide_reach(c, res)
    assert digest(res) == WIDE_GOLD[c["name"]]
    assert res["counters"]["saturations"] == 0


@pytest.mark.parametrize("variant", WIDE_VARIANTS)
@pytest.mark.parametrize("p", [257, 1025])
def test_wide_chain_images_resume_bit_for_bit(oracle, p, variant):
    """alpha, cdfS and vi of an image are arrays of length p: one cut inside tuning (iter > m: the draw runs on the
    weights being rebuilt right after the load)."""
    c = make_wide(p, variant)
    assert digest(run_case(c, oracle, checkpoint_at=(5,))) == WIDE_GOLD[c["name"]]


# ------------------------------------------------------------------ the split-variable draw against NumPy
def split_draw_vectors(p):
    """(weights, thresholds) for the inverse-CDF checks, here and on the device: integer split weights of the
    sampler's own magnitude -- rne(prior 2^24 / max prior) plus tuning counts of 2^24 / max prior each -- and
    thresholds u: 0, the largest double below 1, for EVERY column j the three doubles around S_j / S_{p-1} (the block
    boundaries 63 | 64, 255 | 256 and the last two columns among them; beyond 1 the draw falls back to p - 1), and
    300 uniform draws."""
    rng = np.random.default_rng([p, 7])
    prior = rng.choice([1.0, 1.0, 1.0, 0.37, 2.5, 40.0], p)
    unit = np.rint(2.0 ** 24 / prior.max())
    A = np.maximum(np.rint(prior * (2.0 ** 24 / prior.max())), 1.0) + unit * rng.poisson(0.7, p)
    A = A.astype(np.int64)
    S = np.cumsum(A)
    assert S[-1] < 2 ** 53
    q = S.astype(float) / float(S[-1])
    u = np.concatenate([[0.0, np.nextafter(1.0, 0.0)], np.nextafter(q, 0.0), q, np.nextafter(q, 2.0), rng.random(300)])
    return A, np.ascontiguousarray(u)


def numpy_sample_var(A, u):
    """The first j with u * float(S[-1]) <= float(S[j]), else p - 1 (include/pgbart_spec.h: pgb_sample_var)."""
    S = np.cumsum(A)
    return np.minimum(np.searchsorted(S.astype(float), u * float(S[-1]), side="left"), len(S) - 1)


def oracle_sample_var(oracle, A, u):
    f = oracle.lib.lib.pgbo_sample_var
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_double]
    S = np.ascontiguousarray(np.cumsum(A), np.int64)
    return np.array([f(S.ctypes.data, len(S), float(x)) for x in u])


@pytest.mark.parametrize("p", [1] + WIDE_P)
def test_split_variable_draw_is_the_inverse_cdf_at_every_prefix_sum(oracle, p):
    A, u = split_draw_vectors(p)
    want = numpy_sample_var(A, u)
    assert np.array_equal(oracle_sample_var(oracle, A, u), want)
    # the vectors do what they are for: every column is drawn, and each exact threshold separates j from j + 1
    assert set(want.tolist()) == set(range(p))
    q = np.cumsum(A).astype(float) / float(A.sum())
    for j in sorted({63, 64, 255, 256, p - 2, p - 1} & set(range(p))):
        around = numpy_sample_var(A, np.array([np.nextafter(q[j], 0.0), q[j], np.nextafter(q[j], 2.0)]))
        assert around[0] == j and j <= around[1] <= around[2] <= min(j + 1, p - 1), (j, around)


# ------------------------------------------------------------------ flat likelihood: the split prior at p = 300
FLAT_P, FLAT_N, FLAT_M, FLAT_STEPS, FLAT_BURN, FLAT_THIN = 300, 400, 40, 140, 20, 4


def flat_design():
    """The split prior of the flat-likelihood test and the class of every column.  A class is (block of 64) x
    (lane 0 | lanes 1..62 | lane 63); p = 300: four whole blocks and columns 256..299, 14 classes.  The weight is
    constant within a class, 1 or 2 inside a block (neighbouring blocks differ) and 14 / 18 on lanes 0 / 63: a draw
    that lands one lane off moves the mass of an edge column into its neighbour, a draw one block off exchanges
    blocks of different mass."""
    j = np.arange(FLAT_P)
    block, lane = j // 64, j % 64
    prior = np.where(block % 2 == 0, 1.0, 2.0)
    prior[lane == 0] = 14.0
    prior[lane == 63] = 18.0
    cls = 3 * block + np.where(lane == 0, 0, np.where(lane == 63, 2, 1))
    _, cls = np.unique(cls, return_inverse=True)
    return prior, cls


def flat_split_counts(backend, seed, P):
    """Split variables of EVERY internal node of the forests recorded every 4th step after 20, sigma = 1e6: each is a
    draw from the split prior (a continuous split never fails, whatever the column), and with every tree re-sampled at
    every step a recorded tree is either the one of four steps ago (probability P^-4) or grown afresh."""
    rng = np.random.default_rng(2)
    X, Y = rng.normal(size=(FLAT_N, FLAT_P)), rng.normal(size=FLAT_N)
    prior, cls = flat_design()
    st = PyBartSettings.from_data(X, Y, m=FLAT_M, num_particles=P, seed=seed, batch=(1.0, 1.0))
    s = PySampler(st, X, Y, np.zeros(FLAT_P, np.int32), prior, backend=backend)
    s.set_likelihood([1e6])
    counts = np.zeros(FLAT_P, np.int64)
    for it in range(FLAT_STEPS):
        s.step(False)
        if it >= FLAT_BURN and it % FLAT_THIN == 0:
            v = np.asarray(s.export_trees(1).var)
            counts += np.bincount(v[v >= 0], minlength=FLAT_P)
    return counts, np.bincount(cls, weights=counts), s


def pearson(observed, expected):
    return float(np.sum((observed - expected) ** 2 / expected))


def flat_chi_square(counts_by_class):
    """(statistic, bound, expected counts): Pearson's chi-square of the class counts against the split prior; the
    bound is the 1e-6 upper quantile of chi-square with (classes - 1) degrees of freedom."""
    prior, cls = flat_design()
    mass = np.bincount(cls, weights=prior)
    expected = counts_by_class.sum() * mass / mass.sum()
    return pearson(counts_by_class, expected), float(stats.chi2.isf(1e-6, len(mass) - 1)), expected


def test_flat_likelihood_split_variables_follow_a_wide_split_prior(oracle):
    """Oracle-independent.  On the oracle: 1792 split variables, chi-square 3.94 at 13 degrees of freedom against the
    bound 52.75 (chi2.isf(1e-6, 13)); the smallest expected class count is 45."""
    counts, by_class, _ = flat_split_counts(oracle, seed=11, P=8)
    stat, bound, expected = flat_chi_square(by_class)
    print(f"flat likelihood, p = {FLAT_P}: {int(by_class.sum())} split variables, chi-square {stat:.2f}, "
          f"bound {bound:.2f}, smallest expected count {expected.min():.1f}")
    assert len(expected) == 14 and expected.min() >= 20.0
    assert stat < bound
    assert stat < 0.5 * bound   # (the design's own margin: thin further rather than raise the bound)
    # the statistic has power: the mass of lane 63 of block 1 landing on the next column (lane 0 of block 2) ...
    _, cls = flat_design()
    one_lane_off = expected.copy()
    one_lane_off[cls[128]] += one_lane_off[cls[127]]
    one_lane_off[cls[127]] = 0.0
    assert pearson(one_lane_off, expected) > bound
    # ... and the draws of block 1 landing in block 2
    one_block_off = expected.copy()
    for lane in (0, 1, 63):
        one_block_off[cls[128 + lane]] += expected[cls[64 + lane]]
        one_block_off[cls[64 + lane]] -= expected[cls[64 + lane]]
    assert pearson(one_block_off, expected) > bound
