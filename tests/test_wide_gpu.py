"""Wide design matrices -- GPU half: the HIP library on the column-count edges of the sampler.

p = 31 .. 1500 (tests/_cases.py: WIDE_P) puts a chain on both sides of every place the device code branches on the
column count: the three regimes of `sample_var_prefix` (<= 64, 65..256, > 256), the carry between 64-blocks in
`sample_var_weights` and in the owner's rebuild of the prefix sums while tuning, tile columns of `k_transpose` beyond
the first and its `col_nan` flags, the per-column workgroups of `k_colmax` / `k_subset_check` / the order keys, the
second trip of the `vi` copy and its 64-byte lines in the step output, `pgb_set_data`'s staging of the split prior
on both sides of p = n_pad, and chain images with arrays of length p.  Every comparison is exact; what each case
reaches is pinned on the oracle in tests/test_wide.py."""
import ctypes as C

import numpy as np
import pytest

from _cases import digest, make_wide, run_case, set_data_rc, wide_case, wide_layout
from pymc_bart_amd import _abi
from pymc_bart_amd.sampler import PyBartSettings, PySampler
from test_parity_gpu import _assert_same
from test_wide import ALL_WIDE, WIDE_GOLD, WIDE_IDS, flat_chi_square, flat_split_counts

pytestmark = pytest.mark.gpu

PGB_E_INVALID = -1  # include/pgbart.h


def _same_forest(a, b):
    for f in ("node_off", "var", "left", "right", "count", "split", "value"):
        assert np.array_equal(getattr(a["forest"], f), getattr(b["forest"], f)), f


@pytest.mark.parametrize("p,variant", ALL_WIDE, ids=WIDE_IDS)
def test_wide_hip_equals_oracle_and_golden(hip, oracle, p, variant):
    c = make_wide(p, variant)
    g = run_case(c, hip)
    o = run_case(c, oracle)
    lib = g["sampler"].backend.lib
    assert lib.backend_name == "hip-gfx950" and lib.max_particles == (128 if c["P"] > 64 else 64)
    _assert_same(g, o)
    _same_forest(g, o)
    assert digest(g) == WIDE_GOLD[c["name"]]
    assert g["counters"]["saturations"] == 0


@pytest.mark.parametrize("variant", ["normal", "linear", "categorical_k3"])
@pytest.mark.parametrize("p", [257, 1025])
def test_wide_host_output_step_equals_the_device_output_step(hip, p, variant):
    """pgb_step_host against pgb_step with more than 256 columns: the `vi` copy takes a second trip, and its segment
    of the step output spans many 64-byte lines.  The chain is the case's own (run_case's key and moving sigma), whose
    `vi` is known to be non-zero beyond column 255."""
    c = make_wide(p, variant)
    X, Y = c["X"], c["Y"]
    fam = c.get("family", "normal")
    st = PyBartSettings.from_data(X, Y, m=c["m"], num_particles=c["P"], seed=c["seed"], family=fam,
                                  n_outputs=c.get("K", 1), response=c.get("response", "constant"), batch=c["batch"],
                                  beta=c["beta"])
    a = PySampler(st, X, Y, c["rules"], c["prior"], backend=hip)
    b = PySampler(st, X, Y, c["rules"], c["prior"], backend=hip)
    K, n = st.n_outputs, st.n
    vi_total = np.zeros(p, np.int64)
    sig_rng = np.random.default_rng(99)
    for it in range(12):
        sig = float(0.5 + sig_rng.random())
        for s in (a, b):
            s.set_likelihood([sig] if fam == "normal" else [])
        sa, va = a.step(it < 6)                    # host path
        _, vb = b.step(it < 6, fetch=False)        # device path
        sb = hip.mem.to_host(b.sum_trees_device())
        sb = sb.reshape(K, n) if K > 1 else sb
        assert np.array_equal(sa, sb) and np.array_equal(va, vb)
        vi_total += va
        ta, tb = a.export_trees(0), b.export_trees(0)
        for f in ("tree_id", "node_off", "var", "left", "right", "count", "split", "value", "slope", "xbar", "svar"):
            assert np.array_equal(getattr(ta, f), getattr(tb, f)), f
        assert a.counters.as_dict() == b.counters.as_dict()
    assert vi_total[256:].sum() > 0   # (the second trip carried something)


@pytest.mark.parametrize("p,variant", [(257, "normal"), (1025, "categorical_k3")])
def test_wide_chain_migrates_between_the_backends(hip, oracle, p, variant):
    """GPU -> oracle inside tuning (iter > m: the next draw runs on the weights being rebuilt) -> GPU in the draws:
    the images carry alpha, cdfS and vi, arrays of length p."""
    c = make_wide(p, variant)
    g = run_case(c, hip, checkpoint_at={4: oracle, 9: hip})
    assert g["sampler"].backend.lib.backend_name == "hip-gfx950"
    _assert_same(g, run_case(c, oracle))
    assert digest(g) == WIDE_GOLD[c["name"]]


def _padded(c, pad):
    n, p = c["X"].shape
    wide = np.full((n, p + pad), np.nan)
    wide[:, p + 1::2] = 1e300
    wide[:, :p] = c["X"]
    return wide


@pytest.mark.parametrize("p,variant", [(33, "linear"), (257, "linear"), (1025, "linear"), (1025, "normal")])
def test_wide_padded_matrix_is_the_same_data(hip, p, variant):
    """ldx = p + 3 with NaN and 1e300 in the pad columns (a transpose that read them would flag a missing value or
    find a huge column exponent): the chain of the contiguous matrix."""
    c = make_wide(p, variant)

    def hand_over_padded(s):
        rc, msg = set_data_rc(s, _padded(c, 3), c["rules"], c["prior"], ldx=p + 3)
        assert rc == _abi.PGB_OK, msg

    g = run_case(c, hip, setup=hand_over_padded)
    assert g["sampler"].backend.lib.backend_name == "hip-gfx950"
    assert digest(g) == WIDE_GOLD[c["name"]]


@pytest.mark.parametrize("variant", ["normal", "probit_mix"])
@pytest.mark.parametrize("p", [65, 257])
def test_wide_order_keys_forced(hip, oracle, monkeypatch, p, variant):
    """The 16-bit order keys are built one column at a time; the library uses them for constant leaves without
    SubsetSplit columns, so the case is run that way (the subset column as one-hot): the oracle's chain."""
    monkeypatch.setenv("PGB_X32_MIN_MB", "0")
    c = make_wide(p, variant)
    c["rules"] = np.where(c["rules"] == 2, 1, c["rules"]).astype(np.int32)
    c["response"] = "constant"
    g = run_case(c, hip)
    assert g["sampler"].backend.lib.backend_name == "hip-gfx950"
    o = run_case(c, oracle)
    _assert_same(g, o)
    _same_forest(g, o)
    assert sum((v >= 64).sum() for v in o["split_vars"]) > 0


# ------------------------------------------------------------------ refusals name the right column
def _refused_then_good(c, bad_X, bad_prior, expect):
    """setup hook for run_case: a refused pgb_set_data (the message must satisfy `expect`), after which every step is
    refused for want of data, then the good data again."""
    def setup(s):
        lib, mem = s.backend.lib.lib, s.backend.mem
        rc, msg = set_data_rc(s, bad_X, c["rules"], bad_prior)
        assert rc == PGB_E_INVALID and expect(msg), (rc, msg)
        K, (n, p) = c.get("K", 1), c["X"].shape
        dev = mem.empty((K * n,), np.float64)
        vi = np.zeros(p, np.int32)
        ctr = _abi.Counters()
        assert lib.pgb_step(s._h, 1, mem.ptr(dev), vi.ctypes.data, C.byref(ctr)) == PGB_E_INVALID
        assert "set_data" in lib.pgb_last_error().decode()
        rc, msg = set_data_rc(s, c["X"], c["rules"], c["prior"])
        assert rc == _abi.PGB_OK, msg
    return setup


def _case_301():
    """p = 301: the SubsetSplit column is column 300 (the last one, with missing values); column 40 becomes one too."""
    c = wide_case(301, "normal", 0)
    assert wide_layout(301)[2] == 300
    c["rules"] = c["rules"].copy()
    c["rules"][40] = 2
    c["X"][:, 40] = np.random.default_rng(40).integers(0, 5, c["X"].shape[0])
    return c


@pytest.mark.parametrize("columns", [(300,), (40, 300)], ids=["column 300", "columns 40 and 300"])
def test_wide_refused_subset_codes_name_their_column(hip, oracle, columns):
    c = _case_301()
    bad = c["X"].copy()
    rows = np.flatnonzero(~np.isnan(bad[:, 300]))
    for k, col in enumerate(columns):
        bad[rows[k], col] = 52.0   # one category code past PGB_SUBSET_BITS - 1
    names = [f"SubsetSplit column {col}:" for col in columns]
    want = run_case(c, oracle)
    for backend in (hip, oracle):
        g = run_case(c, backend, setup=_refused_then_good(c, bad, c["prior"], lambda msg: any(t in msg for t in names)))
        assert g["sampler"].backend.lib.backend_name == backend.lib.backend_name
        _assert_same(g, want)
        _same_forest(g, want)


def test_wide_refused_prior_beyond_the_padded_rows(hip, oracle):
    """p = 1025 columns: a non-positive split prior at index 1024 is refused; the good call after it gives the chain."""
    c = make_wide(1025, "normal")
    bad_prior = c["prior"].copy()
    bad_prior[1024] = 0.0
    for backend in (hip, oracle):
        g = run_case(c, backend, setup=_refused_then_good(c, c["X"], bad_prior, lambda msg: "split_prior must be positive" in msg))
        assert digest(g) == WIDE_GOLD[c["name"]]


def test_wide_flat_likelihood_split_variables_follow_the_split_prior_on_gpu(hip):
    """The chi-square test of tests/test_wide.py on the device, another key and 100 particles (two per lane)."""
    counts, by_class, s = flat_split_counts(hip, seed=23, P=100)
    assert s.backend.lib.backend_name == "hip-gfx950" and s.backend.lib.max_particles == 128
    stat, bound, expected = flat_chi_square(by_class)
    print(f"flat likelihood on the device: {int(by_class.sum())} split variables, chi-square {stat:.2f}, bound {bound:.2f}, "
          f"smallest expected count {expected.min():.1f}")
    assert expected.min() >= 20.0
    assert stat < bound
