"""Chain diagnostics on the build box (no GPU): the numeric contract of ``include/pgbart_diag.h``
(``tests/_diag_host.py``) against an independent NumPy / SciPy restatement of the published definitions
(``tests/_diag_numpy.py``) within 8 x the measured difference (``profiles/diag_accuracy.json``,
``tools/diag_accuracy.py``), the exact properties the contract promises, a loose check against theory, the host-side
refusals of ``pymc_bart_amd.diagnostics`` and the library's export.

The header and the restatement differ by the order of their sums and by the rounding of the FFT only: ranks, the split,
quantiles and the stopping rule are the same functions of the same numbers.  (Where a pair sum of Geyer's sequence sat
within rounding of zero the two could stop at different lags; on the fixed inputs below they do not, and the measured
figures say so.)"""
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
from scipy.stats import rankdata

import _diag_host as host
import _diag_numpy as ref
from pymc_bart_amd import _abi, compiled, convergence, diagnose_matrix, diagnostics, relative_efficiency

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = os.path.join(ROOT, "profiles", "diag_accuracy.json")

# (n_chains, n_per_chain): the smallest, odd lengths, one and several lane strides per split chain, many chains
SHAPES = ((1, 4), (1, 5), (2, 7), (4, 64), (4, 65), (3, 127), (2, 129), (8, 512))
KINDS = ("normal", "ar95", "walk", "alternating", "ties", "zeros", "constant", "constant in one chain", "chain means",
         "q05 is the minimum")


def column(kind: str, n_chains: int, n: int, rng) -> np.ndarray:
    """One column (n_chains * n,), chain after chain."""
    D = n_chains * n
    if kind == "ar95":
        x = np.empty((n_chains, n))
        x[:, 0] = rng.normal(0, 1, n_chains) / math.sqrt(1.0 - 0.95 ** 2)
        for i in range(1, n):
            x[:, i] = 0.95 * x[:, i - 1] + rng.normal(0, 1, n_chains)
        return x.ravel()
    if kind == "walk":          # Geyer's loop runs to h - 3
        return np.cumsum(rng.normal(0, 1, D))
    if kind == "alternating":   # ... stops at the first pair
        return np.tile([1.0, -1.0], D)[:D] * (1.0 + 0.01 * rng.uniform(0, 1, D))
    if kind == "ties":
        return np.round(rng.normal(0, 1, D), 1)
    if kind == "zeros":
        return rng.choice([0.0, -0.0], D)
    if kind == "constant":
        return np.full(D, float(rng.choice([0.1, -3.0, 2.5])))
    if kind == "constant in one chain":
        x = rng.normal(0, 1, D)
        x[:n] = 0.25
        return x
    if kind == "chain means":   # R-hat >> 1
        return rng.normal(0, 1, D) + np.repeat(3.0 * np.arange(n_chains), n)
    if kind == "q05 is the minimum":
        x = rng.normal(0, 1, D)
        x[rng.permutation(D)[:max(D // 8, 1)]] = -6.0
        return x
    return rng.normal(0, 1, D)


def matrix(n_chains: int, n: int, n_cols: int, ld: int, shift: int, seed: int) -> np.ndarray:
    """(n_chains * n, ld): column c is of kind (c + shift) mod 10; the columns beyond n_cols hold a value no result
    may show."""
    rng = np.random.default_rng(seed)
    a = np.full((n_chains * n, ld), 7.0e77)
    for c in range(n_cols):
        a[:, c] = column(KINDS[(c + shift) % len(KINDS)], n_chains, n, rng)
    return a


def loglik_matrix(n_chains: int, n: int, n_cols: int, seed: int, kinds: int = 4) -> np.ndarray:
    """Log-likelihood-like values in [-2047, 0]: iid, autocorrelated, a few at the clamp, and (``kinds=4``) one column
    that is nearly constant."""
    rng = np.random.default_rng(seed)
    D = n_chains * n
    a = np.empty((D, n_cols))
    for c in range(n_cols):
        kind = c % kinds
        if kind == 0:
            a[:, c] = -rng.gamma(2.0, 1.5, D)
        elif kind == 1:
            a[:, c] = -0.5 * column("ar95", n_chains, n, rng) ** 2 - 1.0
        elif kind == 2:
            a[:, c] = -rng.gamma(2.0, 40.0, D)
            a[rng.permutation(D)[:max(D // 16, 1)], c] = -2047.0
        else:
            a[:, c] = -3.0 - 1e-9 * rng.uniform(0, 1, D)
    return np.clip(a, -2047.0, 0.0)


def accuracy_inputs():
    """(transform, n_chains, matrix) of every input the header is held to the restatement on."""
    for k, (nc, n) in enumerate(SHAPES):
        yield "identity", nc, matrix(nc, n, len(KINDS), len(KINDS), 0, seed=500 + k)
        # (without the nearly constant column: its sd is 1e-10 of its mean, so a mean that is right to 1e-16 leaves
        # the variance right to 1e-6 on either side -- the column's conditioning, not a figure to hold anything to)
        yield "exp_shift", nc, loglik_matrix(nc, n, 6, seed=600 + k, kinds=3)
    yield "identity", 4, matrix(4, 1000, len(KINDS), len(KINDS), 0, seed=700)


def shifted_exponentials(a: np.ndarray, n_chains: int) -> np.ndarray:
    """``pgb_exp_t(a - amax)`` per column, amax over the draws the split keeps."""
    n = a.shape[0] // n_chains
    kept = np.ones(n, bool)
    if n % 2:
        kept[n // 2] = False
    amax = a.reshape(n_chains, n, -1)[:, kept, :].max(axis=(0, 1))
    return host.exp_t(a - amax[None, :])


def differences() -> dict:
    """The largest relative difference of every output between the header and the restatement, per transform.

    For ``exp_shift`` the restatement is given the header's own exponentials: the header's table exp and ``np.exp``
    differ in the last place (measured by ``tools/rowsummary_accuracy.py``), and S is even, so the two middle values
    are EQUALLY far from the median and which of them is ranked first in ``|x - median|`` is decided by that last
    place -- with 4 draws that moves the folded R-hat by half its value.  That would measure the exponential, not the
    order of the sums; that the header applies the exponential it says is an exact test below."""
    worst = {t: {name: 0.0 for name in ref.ROWS} for t in ("identity", "exp_shift")}
    for transform, nc, a in accuracy_inputs():
        got = host.columns(a, nc, transform)[:len(ref.ROWS)]
        want = ref.columns(a if transform == "identity" else shifted_exponentials(a, nc), nc)
        for r, name in enumerate(ref.ROWS):
            same = (got[r] == want[r]) | (np.isnan(got[r]) & np.isnan(want[r]))
            with np.errstate(all="ignore"):
                rel = np.where(same, 0.0, np.abs(got[r] - want[r]) / np.abs(want[r]))
            worst[transform][name] = max(worst[transform][name], float(np.max(rel)))
    return worst


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------ 1. the header against the restatement
def test_header_against_the_numpy_restatement():
    with open(ACCURACY) as fh:
        measured = json.load(fh)["largest_relative_difference"]
    worst = differences()
    print(json.dumps(worst))
    for transform, rows in worst.items():
        for name, figure in rows.items():
            assert figure <= 8.0 * measured[transform][name], (transform, name, figure, measured[transform][name])


# ------------------------------------------------------------------ 2. exact properties of the header
@pytest.mark.parametrize("transform", ["identity", "exp_shift"])
def test_permuting_whole_chains_changes_no_bit(transform):
    rng = np.random.default_rng(3)
    for nc, n in ((4, 65), (3, 127), (8, 16)):
        a = matrix(nc, n, 10, 10, 0, seed=nc * n) if transform == "identity" else loglik_matrix(nc, n, 4, seed=nc * n)
        one = host.columns(a, nc, transform)
        for _ in range(3):
            perm = rng.permutation(nc)
            b = a.reshape(nc, n, -1)[perm].reshape(a.shape)
            assert np.array_equal(bits(host.columns(b, nc, transform)), bits(one)), (nc, n, perm)
        mean_only = host.columns(a, nc, transform, stats=host.MEAN_ONLY)
        assert np.array_equal(bits(mean_only[5:9]), bits(one[5:9])) and not mean_only[:5].any() and not mean_only[9].any()


def test_average_ranks_on_heavy_ties():
    rng = np.random.default_rng(4)
    for x in (np.round(rng.normal(0, 1, 500), 1), rng.choice([0.0, -0.0, 1.0, -1.0], 257), np.full(64, 2.0),
              rng.integers(0, 3, 1000).astype(np.float64), rng.normal(0, 1, 100)):
        assert np.array_equal(host.ranks(x), rankdata(x, method="average"))
    # ... and the z-score is read at the average rank: with the table r -> r the "z-scores" are the ranks
    nc, n = 2, 32
    a = np.round(rng.normal(0, 1, (nc * n, 1)), 1)
    S = nc * n
    table = 1.0 + 0.5 * np.arange(2 * S - 1)
    out = host.columns(a, nc, z=table)
    r = rankdata(a[:, 0], method="average").reshape(nc, n)
    want = ref.rhat2(ref.split(r))
    assert abs(out[0, 0] - want) <= 1e-12 * want


def test_the_constant_rules():
    for nc, n in ((1, 4), (2, 7), (4, 64)):
        S = host.kept(nc, n)
        D = nc * n
        rng = np.random.default_rng(D)
        a = np.stack([np.full(D, 0.1), rng.choice([0.0, -0.0], D), np.repeat(np.arange(nc, dtype=np.float64), n),
                      column("constant in one chain", nc, n, rng)], axis=1)
        out = host.columns(a, nc)
        for c in (0, 1):          # constant, and +-0.0 (equal values): R-hat 1, every ESS = S, the flag
            assert out[0, c] == 1.0 and out[1, c] == 1.0 and np.all(out[2:6, c] == S) and out[8, c] == 1.0
            assert out[7, c] == 0.0 and abs(out[6, c] - a[0, c]) <= 1e-16
        if nc > 1:                # every chain constant at another level: W = 0, B > 0
            # (the mean of h copies of a z-score is that z-score only up to rounding: W is exactly 0 where the sums
            # are exact, as with the table r -> r of multiples of 1/2, and some 1e-32 otherwise)
            exact = host.columns(a, nc, z=1.0 + 0.5 * np.arange(2 * S - 1))
            assert exact[0, 2] == np.inf and out[0, 2] > 1e12
            assert out[8, 2] == 0.0 and np.all(np.isfinite(out[2:6, 2])) and np.all(out[2:6, 2] > 0)
            assert out[8, 3] == 0.0 and np.isfinite(out[0, 3]) and out[0, 3] > 0.0
        assert np.all(out[9] == 0.0)
        # an indicator that is all 1: the 95 % quantile of a two-valued column is its maximum ... and x >= max is not
        # constant; the all-0 / all-1 indicators of a constant column are (above)


def test_the_dropped_middle_draw_changes_nothing():
    for nc, n in ((1, 5), (2, 7), (4, 65), (3, 127)):
        for transform, a in (("identity", matrix(nc, n, 10, 10, 0, seed=n)), ("exp_shift", loglik_matrix(nc, n, 4, seed=n))):
            one = host.columns(a, nc, transform)
            b = a.copy()
            b.reshape(nc, n, -1)[:, n // 2, :] = 0.0 if transform == "exp_shift" else 1.0e6   # (the largest value of all)
            assert np.array_equal(bits(host.columns(b, nc, transform)), bits(one)), (nc, n, transform)
            # an even chain has no middle draw: the same edit changes the result
        a = matrix(2, 8, 10, 10, 0, seed=8)
        b = a.copy()
        b.reshape(2, 8, -1)[:, 4, :] = 1.0e6
        assert not np.array_equal(bits(host.columns(b, 2)), bits(host.columns(a, 2)))


def test_exp_shift_is_identity_on_the_shifted_exponentials():
    for nc, n in ((1, 4), (2, 7), (4, 64), (3, 127)):
        a = loglik_matrix(nc, n, 8, seed=7 * n)
        x = shifted_exponentials(a, nc)
        for stats in (host.ALL, host.MEAN_ONLY):
            assert np.array_equal(bits(host.columns(a, nc, "exp_shift", stats)), bits(host.columns(x, nc, "identity", stats)))


# ------------------------------------------------------------------ 3. against theory, loosely
def test_ar1_against_theory():
    """An AR(1) column with phi = 0.5 has ESS / S -> (1 - phi) / (1 + phi) = 1 / 3."""
    rng = np.random.default_rng(2024)
    nc, n, phi = 4, 1000, 0.5
    x = np.empty((nc, n))
    x[:, 0] = rng.normal(0, 1, nc) / math.sqrt(1.0 - phi * phi)
    for i in range(1, n):
        x[:, i] = phi * x[:, i - 1] + rng.normal(0, 1, nc)
    out = host.columns(x.reshape(-1, 1), nc)
    ratio = out[5, 0] / (nc * n)
    print("ess_mean / S =", ratio, "restatement:", ref.column(x)["ess_mean"] / (nc * n))
    assert (1.0 / 3.0) / 1.5 <= ratio <= (1.0 / 3.0) * 1.5
    assert out[0, 0] < 1.01 ** 2 and out[1, 0] < 1.01 ** 2


# ------------------------------------------------------------------ 4. refusals of the Python layer, before a backend
class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the backend was touched ({name})")


def _fake_sampler(lengths):
    def no_backend():
        raise AssertionError("the backend was touched")

    parts = [types.SimpleNamespace(pool=None, forest_idx=np.zeros((L, 5), np.int32), m=5, n_outputs=1, _get_backend=no_backend)
             for L in lengths]
    return types.SimpleNamespace(_chain_samplers=parts)


def test_refusals_of_diagnose_matrix():
    be = _Untouchable()
    with pytest.raises(ValueError, match="unknown transform 'log'"):
        diagnose_matrix(np.zeros((16, 3)), 2, transform="log", backend=be)
    with pytest.raises(ValueError, match="do not divide into n_chains = 5"):
        diagnose_matrix(np.zeros((16, 3)), 5, backend=be)
    with pytest.raises(ValueError, match="at least 4 draws per chain, got 3"):
        diagnose_matrix(np.zeros((6, 3)), 2, backend=be)
    with pytest.raises(ValueError, match=r"n_chains must be in \[1, 64\], got 65"):
        diagnose_matrix(np.zeros((65 * 4, 3)), 65, backend=be)
    with pytest.raises(ValueError, match="at most 8192 draws after the split, got 8194"):
        diagnose_matrix(np.zeros((8194, 1)), 1, backend=be)
    with pytest.raises(ValueError, match="matrix"):
        diagnose_matrix(np.zeros(16), 2, backend=be)
    for bad in (np.nan, np.inf, -np.inf):
        a = np.zeros((16, 3))
        a[5, 1] = bad
        with pytest.raises(ValueError, match="a must be finite"):
            diagnose_matrix(a, 2, backend=be)
    assert diagnostics.kept_draws(1, 8193) == 8192 and diagnostics.kept_draws(2, 4096, diagnostics.MEAN_ONLY) == 8192
    assert diagnostics.kept_draws(4, 4096, diagnostics.MEAN_ONLY) == 16384
    assert diagnostics.MAX_DRAWS == host.max_draws() and diagnostics.MAX_DRAWS_MEAN == host.max_draws_mean()
    assert diagnostics.MAX_CHAINS == host.max_chains() and diagnostics.NOUT == len(host.ROWS)
    assert diagnostics.TRANSFORMS == host.TRANSFORMS


def test_refusals_of_the_fit_calls():
    X = np.zeros((5, 3))
    with pytest.raises(ValueError, match=r"the chains hold \[16, 12\] draws"):
        convergence(_fake_sampler([16, 12]), X)
    with pytest.raises(ValueError, match=r"draws_per_chain = 13, but the chains hold \[16, 12\]"):
        convergence(_fake_sampler([16, 12]), X, draws_per_chain=13)
    with pytest.raises(ValueError, match="at least 4 draws per chain, got 3"):
        convergence(_fake_sampler([3, 3]), X)
    with pytest.raises(ValueError, match="at least 4 draws per chain, got 2"):
        convergence(_fake_sampler([16, 12]), X, draws_per_chain=2)
    with pytest.raises(ValueError, match="at most 8192 draws after the split, got 8200"):
        convergence(_fake_sampler([4100, 4100]), X)
    for transform in ("exp_shift", "exp", "logistic"):
        with pytest.raises(ValueError, match=f"'identity' only for now, not '{transform}'"):
            convergence(_fake_sampler([16, 16]), X, transform=transform)
    with pytest.raises(TypeError, match="sampler must be"):
        convergence(object(), X)
    y = np.zeros(5)
    with pytest.raises(ValueError, match=r"the chains hold \[16, 12\] draws"):
        relative_efficiency(_fake_sampler([16, 12]), X, y, None)
    with pytest.raises(ValueError, match="at most 16384 draws after the split, got 16400"):
        relative_efficiency(_fake_sampler([8200, 8200]), X, y, None)
    with pytest.raises(ValueError, match="at least 4 draws per chain"):
        relative_efficiency(_fake_sampler([3]), X, y, None)


def test_the_z_table():
    from scipy.special import ndtri

    for S in (4, 64, 1000):
        z = diagnostics.z_table(S)
        r = 1.0 + 0.5 * np.arange(2 * S - 1)
        assert z.shape == (2 * S - 1,) and np.allclose(z, ndtri((r - 0.375) / (S + 0.25)), rtol=1e-13, atol=0.0)
        assert np.all(np.diff(z) > 0.0)


# ------------------------------------------------------------------ 5. the library
def test_the_entry_point_is_bound_by_name():
    assert "pgb_chain_diag" not in _abi.SYMBOLS
    fake = types.SimpleNamespace(lib=types.SimpleNamespace(), path="liboracle.so")
    with pytest.raises(NotImplementedError, match="pgb_chain_diag"):
        _abi.PGBLibrary.chain_diag_entry_point(fake)


@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_point(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    if not os.path.exists(path):
        pytest.skip(f"{so} has not been built")
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    assert " pgb_chain_diag\n" in syms


UNIT = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <vector>
#include "pgbart.h"
#include "pgbart_spec.h"
#include "pgbart_diag.h"
#define PGB_STR2(x) #x
#define PGB_STR(x) PGB_STR2(x)
static thread_local char g_err[512];
static int fail(int code, const char* msg) { snprintf(g_err, sizeof g_err, "%s", msg); return code; }
static int fail_hip(hipError_t e, const char* what) { snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e)); return PGB_E_DEVICE; }
#include "k_diag.h"
"""


def test_the_kernel_cross_compiles_for_gfx950_and_is_budgeted(tmp_path):
    """``csrc/k_diag.h`` with the library's flags for gfx950: one kernel, no scratch; the committed occupancy budget
    knows it; and its static LDS leaves room for the 128 KiB of dynamic LDS a column of 8192 draws takes."""
    src, out = tmp_path / "unit.hip", tmp_path / "unit.s"
    src.write_text(UNIT)
    r = subprocess.run([compiled.hipcc_path(), *compiled.DEVICE_FLAGS, f"-I{compiled.CSRC}", "--cuda-device-only", "-S",
                        str(src), "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    assert asm.count(".amdhsa_kernel ") == 1 and ".amdhsa_kernel _Z12k_chain_diag" in asm
    meta = asm[asm.index("amdhsa.kernels"):]
    assert ".private_segment_fixed_size: 0" in meta and ".vgpr_spill_count: 0" in meta
    static_lds = int(meta.split(".group_segment_fixed_size:")[1].split()[0])
    assert static_lds + 8 * (8192 + 8192) <= 160 * 1024 and static_lds + 8 * 16384 <= 160 * 1024
    budget = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    row = budget["k_chain_diag"]
    assert row["max_scratch_bytes"] == 0 and row["max_vgpr_spills"] == 0 and row["min_wgs_per_cu"] >= 2


if __name__ == "__main__":
    sys.exit(pytest.main([__file__, "-q"]))
