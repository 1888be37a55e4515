"""Exact SHAP interaction values (``include/pgbart_shap_interaction.h``, ``pymc_bart_amd/shap_interaction.py``) without a
GPU: the host build of the header against the definition -- all ``2^p`` coalitions, each evaluated by
``_predict_exact.walk`` in ``Fraction`` arithmetic --, its exact properties, the slot limit and every refusal.

The tolerance.  For entry (d, k, i) ``M`` is ``_shap_host.magnitude``'s sum of ``|coef|`` over the leaf terms of forest d
and ``T`` their number.  ``tools/shap_interaction_accuracy.py`` measures ``max |host - exact| / M`` on the pools below and
on chain trees over 16 and 32 distinct columns (``profiles/shap_interaction_accuracy.json``); the tolerance here is 8 x
that figure x M, and the figure itself must lie below the crude ceiling ``(5000 + 17 T) 2^-53``:

  one term of u <= 33 slots, in units of 2^-53 x |coef|.  A coefficient c_k is a sum of products of at most u
  non-negative factors, two roundings per factor: 2 u relative.  s and s2 add at most u non-negative products
  W c (W itself within 2 u): 5 u + 1 relative, s, s2 <= 1.  g = (o - z) s: 5 u + 3, |g| <= 1.  h = 0.5 ((o - z)(o - z)) s2:
  5 u + 5 relative, |h| <= 1/2.  r = g - h - h - ...: the errors of g and of u - 1 values h, (5 u + 3) + (u - 1)(5 u + 5) / 2,
  and u - 1 subtractions of partial sums below 1 + u / 2: at u = 33 at most 168 + 2720 + 560 < 3500.  cw = coef w and
  cw h or cw r: a few more, on values below (1 + u / 2) |coef| <= 17.5 |coef|.  A cell adds T such terms, each addition
  rounding a partial sum below 17.5 M: 17.5 T.  In all below (5000 + 17.5 T) 2^-53 M -- stated as (5000 + 17 T) 2^-53,
  a little stricter."""
import ctypes as C
import json
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _shap_host as host
import _shap_interaction_host as hx
from pymc_bart_amd import _abi, compiled, shap_interaction_summary, shap_interaction_values
from pymc_bart_amd import shap_interaction as mod
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _MultiChainSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1  # PGB_E_INVALID (include/pgbart.h)
U = 2.0 ** -53
FAST = _abi.SHAP_FAST_U
LIMIT = _abi.SHAPX_MAX_U


@pytest.fixture(scope="module")
def accuracy():
    with open(os.path.join(ROOT, "profiles", "shap_interaction_accuracy.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def cases():
    """Per pool: the host build's result and the exact reference, computed once and left unchanged."""
    out = {}
    for name, pool, fidx, X in host.pools():
        got, base = hx.rows(pool, fidx, X)
        Phi, phi, b, R = hx.brute_force(pool, fidx, X)
        M, T = host.magnitude(pool, fidx, X)
        out[name] = dict(pool=pool, fidx=fidx, X=X, got=got, base=base, Phi=Phi, phi=phi, b=b, R=R, M=M, T=T)
    return out


def tolerance(accuracy, M):
    return 8.0 * accuracy["max"] * M


def with_regressor(pool, col):
    """Every leaf of the pool regresses on ``col``."""
    for g in np.flatnonzero(np.asarray(pool.var) < 0):
        pool.svar[g], pool.xbar[g] = col, 0.25
        pool.slope[g] = 0.5
    return pool


# ------------------------------------------------------------------ 1. against the definition
def test_the_measured_figure_lies_below_the_ceiling(accuracy):
    print(f"measured max |host - exact| / M = {accuracy['max']:.3e}; ceiling (5000 + 17 T_min) 2^-53 = "
          f"{(5000 + 17 * accuracy['T_min']) * U:.3e}")
    assert 0.0 < accuracy["max"] < (5000 + 17 * accuracy["T_min"]) * U
    assert {"chain-16-left", "chain-16-right-linear", "chain-32-left-linear", "chain-32-right", "mixed-K3",
            "edges-K1"} <= set(accuracy["cases"])
    assert accuracy["max"] == max(c["max_err_over_M"] for c in accuracy["cases"].values())


@pytest.mark.parametrize("name", ["mixed-K3", "edges-K1"])
def test_the_host_build_against_all_coalitions(cases, accuracy, name):
    c = cases[name]
    got, Phi, M = c["got"], c["Phi"], c["M"]
    D, K, p, _, n = got.shape
    assert np.all(np.isfinite(got))
    worst, nonzero, off = 0.0, 0, 0
    for d in range(D):
        for k in range(K):
            for i in range(n):
                tol = Fraction(tolerance(accuracy, M[d, k, i]))
                for a in range(p):
                    for b in range(p):
                        err = abs(Fraction(float(got[d, k, a, b, i])) - Phi[d, k, a, b, i])
                        if a != b:
                            off += 1
                            nonzero += Phi[d, k, a, b, i] != 0
                        if M[d, k, i] > 0:
                            worst = max(worst, float(err / Fraction(float(M[d, k, i]))))
                        assert err <= tol, (d, k, a, b, i, float(err), float(tol))
    print(f"{name}: max |host - exact| / M = {worst:.3e} (tolerance 8 x {accuracy['max']:.3e}), {nonzero} of {off} "
          f"off-diagonal entries non-zero")
    if name == "mixed-K3":
        assert 3 * nonzero >= off                                   # not a comparison of zeros


def test_the_leafwise_form_is_the_definition(cases):
    for name, c in cases.items():
        assert np.all(hx.restated(c["pool"], c["fidx"], c["X"], Fraction) == c["Phi"]), name


def test_the_definition_has_its_three_properties(cases):
    for name, c in cases.items():
        Phi = c["Phi"]
        assert np.all(Phi == np.swapaxes(Phi, 2, 3)), name
        assert np.all(Phi.sum(axis=3) == c["phi"]), name
        assert np.all(Phi.sum(axis=(2, 3)) + c["b"][:, :, None] == c["R"]), name


# ------------------------------------------------------------------ 2. exact properties of the host build
def test_the_stated_order_of_operations(cases):
    """The header restated in Python floats -- the same operations in the stated order -- gives the same bits; so do
    the rule dispatch on a continuous pool and the general evaluation of every leaf."""
    for name, c in cases.items():
        assert np.array_equal(hx.restated(c["pool"], c["fidx"], c["X"], float), c["got"]), name
        for kw in (dict(general=True), dict(slow=True)):
            again, ab = hx.rows(c["pool"], c["fidx"], c["X"], **kw)
            assert np.array_equal(again, c["got"]) and np.array_equal(ab, c["base"]), (name, kw)
        sb = host.rows(c["pool"], c["fidx"], c["X"])[1]
        assert np.array_equal(c["base"], sb), name                  # base is pgb_shap_base


def test_symmetry_and_nan_entries_are_exact(cases):
    for name, c in cases.items():
        got, X = c["got"], c["X"]
        assert np.array_equal(got, np.swapaxes(got, 2, 3)), name    # bitwise
        nan = np.isnan(X)                                           # (n, p)
        assert nan.any()
        for i, j in zip(*np.nonzero(nan)):
            for cells in (got[:, :, j, :, i], got[:, :, :, j, i]):
                assert np.all(cells == 0.0) and not np.signbit(cells).any(), (name, i, j)
    e = cases["edges-K1"]
    assert np.all(e["got"][:, :, 3] == 0.0) and np.all(e["got"][:, :, :, 3] == 0.0)   # a column no tree uses
    assert np.all(e["got"][1] == 0.0)                                                  # stumps: u = 0


@pytest.mark.parametrize("name", ["mixed-K3", "edges-K1"])
def test_row_sums_and_the_total(cases, accuracy, name):
    """Row a sums to the attribution of ``pgbart_shap.h``'s host build: both are within the tolerance of their exact
    values entry by entry, p entries and one attribution.  The total: p p entries and the base."""
    c = cases[name]
    got, base, M = c["got"], c["base"], c["M"]
    shap, _ = host.rows(c["pool"], c["fidx"], c["X"])
    D, K, p, _, n = got.shape
    for d in range(D):
        for k in range(K):
            for i in range(n):
                tol = Fraction(tolerance(accuracy, M[d, k, i]))
                for a in range(p):
                    row = sum(Fraction(float(v)) for v in got[d, k, a, :, i])
                    assert abs(row - Fraction(float(shap[d, k, a, i]))) <= (p + 1) * tol, (d, k, a, i)
                total = Fraction(float(base[d, k])) + sum(Fraction(float(v)) for v in got[d, k, :, :, i].ravel())
                assert abs(total - c["R"][d, k, i]) <= (p * p + 1) * tol, (d, k, i)


def test_subsets_permutations_leading_dimension_and_picks_are_slices(cases):
    for name, c in cases.items():
        pool, fidx, X, got = c["pool"], c["fidx"], c["X"], c["got"]
        p = X.shape[1]
        for cols in ([2, 0], [1], list(range(p))[::-1], [3, 1, 2]):
            sub, sb = hx.rows(pool, fidx, X, cols=cols)
            assert np.array_equal(sub, got[:, :, cols][:, :, :, cols]) and np.array_equal(sb, c["base"]), (name, cols)
        wide, _ = hx.rows(pool, fidx, X, ldx=p + 3)
        assert np.array_equal(wide, got), name
        picks = [2, 0, 2]
        again, ab = hx.rows(pool, fidx, X, picks=picks, cols=[0, 2])
        assert np.array_equal(again, got[picks][:, :, [0, 2]][:, :, :, [0, 2]]) and np.array_equal(ab, c["base"][picks]), name


@pytest.mark.parametrize("depth,linear", [(1, ()), (FAST - 1, ()), (FAST - 1, (FAST,)), (FAST, ()), (FAST, (FAST + 1,)),
                                          (FAST + 1, ()), (FAST + 1, (2,))])
def test_paths_around_the_fast_length(depth, linear):
    """Path lengths FAST_U - 1, FAST_U and FAST_U + 1, reached by the path alone and by the regressor's slot: the
    unrolled and the general evaluation give the same bits, and they are those of the Python restatement."""
    pool, fidx, rng = host.chain_pool(depth, K=2, side="right" if depth % 2 else "left", linear=linear)
    if linear:
        with_regressor(pool, linear[0])
    X = host.chain_rows(pool, depth, depth + 3, rng, n=4)
    assert hx.slots(pool, depth + 3) == depth + (1 if linear and linear[0] >= depth else 0)
    got, base = hx.rows(pool, fidx, X)
    slow, sb = hx.rows(pool, fidx, X, slow=True)
    assert np.array_equal(got, slow) and np.array_equal(base, sb)
    assert np.array_equal(hx.restated(pool, fidx, X, float), got)
    assert np.count_nonzero(got) >= depth


# ------------------------------------------------------------------ 3. the slot limit
def test_a_chain_of_32_columns_works(accuracy):
    assert LIMIT == hx.max_u() == 32
    pool, fidx, rng = host.chain_pool(LIMIT, K=1, side="left")
    with_regressor(pool, 5)                                         # on the path: no slot of its own
    X = host.chain_rows(pool, LIMIT, LIMIT + 2, rng, n=2)
    assert hx.slots(pool, LIMIT + 2) == LIMIT
    got, _ = hx.rows(pool, fidx, X)
    exact = hx.restated(pool, fidx, X, Fraction)
    M, _ = host.magnitude(pool, fidx, X)
    err = np.vectorize(lambda a, b: abs(Fraction(float(a)) - b), otypes=[object])(got, exact)
    tol = np.vectorize(lambda m: Fraction(tolerance(accuracy, m)), otypes=[object])(M)[:, :, None, None, :]
    assert np.all(err <= tol) and np.count_nonzero(got[0, 0, :, :, 0]) >= LIMIT * LIMIT // 2
    assert np.array_equal(got, np.swapaxes(got, 2, 3))


def _library_call(pool, table, width, cols_values=None, picks_values=None, **kw):
    """``pgb_predict_shap_interactions`` with stand-ins for device memory (never dereferenced: every check precedes the
    first HIP call) -> (rc, message)."""
    lib = _abi.load_hip_library()
    call = lib.shap_interactions_entry_point()
    fidx = np.ascontiguousarray(table, np.int32)
    carr = pool.as_c()
    buf = np.zeros(64)
    cols = np.ascontiguousarray(np.arange(min(width, 4)) if cols_values is None else cols_values, np.int32)
    picks = np.ascontiguousarray(np.zeros(3) if picks_values is None else picks_values, np.int32)
    a = dict(trees=C.byref(carr), fidx=fidx.ctypes.data, n_forests=fidx.shape[0], m=fidx.shape[1], X=buf.ctypes.data, n_rows=8,
             p=width, ldx=width, cols=cols.ctypes.data, n_cols=cols.size, picks=picks.ctypes.data, n_picks=picks.size,
             out=buf.ctypes.data, base=buf.ctypes.data)
    a.update(kw)
    rc = call(a["trees"], a["fidx"], a["n_forests"], a["m"], a["X"], a["n_rows"], a["p"], a["ldx"], a["cols"], a["n_cols"],
              a["picks"], a["n_picks"], a["out"], a["base"], None)
    return rc, lib.lib.pgb_last_error().decode()


@pytest.mark.parametrize("depth,regressor", [(LIMIT, LIMIT + 1), (LIMIT + 1, None)])
def test_more_than_32_slots_are_refused(depth, regressor):
    """32 columns on a path and a regressor off it, and 33 columns on a path: refused with the count and the limit --
    by the library before it touches a device, and by the host build."""
    pool, fidx, rng = host.chain_pool(depth, K=1, side="left")
    if regressor is not None:
        with_regressor(pool, regressor)
    p = depth + 3
    assert hx.slots(pool, p) == LIMIT + 1
    carr = pool.as_c()
    X = host.chain_rows(pool, depth, p, rng, n=1)
    out, cols, picks = np.zeros(p * p), np.arange(p, dtype=np.int32), np.zeros(1, np.int32)
    assert hx.lib().shapx_rows(C.byref(carr), fidx.ctypes.data, 1, X.ctypes.data, 1, p, p, cols.ctypes.data, p, picks.ctypes.data,
                               1, 0, 0, out.ctypes.data, out.ctypes.data) == -3
    rc, msg = _library_call(pool, fidx, p, picks_values=[0])
    assert rc == E_INVALID and "pgb_predict_shap_interactions: trees holds a leaf of 33 slots" in msg and "the limit is 32" in msg, msg
    lib = _abi.load_hip_library()
    with pytest.raises(Exception, match="leaf of 33 slots"):
        lib.check(rc, "pgb_predict_shap_interactions")


# ------------------------------------------------------------------ 4. refusals, the binding, the library
@pytest.fixture(scope="module")
def hand(oracle):
    name, pool, fidx, X = host.pools()[1]
    return PosteriorSampler(pool, fidx, fidx.shape[1], 1, backend=oracle), X


def test_refusals_of_the_python_layer(hand, oracle):
    s, X = hand
    with pytest.raises(ValueError, match="X must be a matrix"):
        s.shap_interactions(np.zeros((0, 4)), [0])
    with pytest.raises(ValueError, match="X must be a matrix"):
        s.shap_interactions(np.zeros((2, 3, 4)), [0])
    with pytest.raises(ValueError, match="picks must be a vector"):
        s.shap_interactions(X, [[0, 1]])
    with pytest.raises(ValueError, match="no draws to attribute"):
        s.shap_interactions(X, [])
    for bad in ([0, 3], [-1]):
        with pytest.raises(ValueError, match="picks must index the 3 stored draws"):
            s.shap_interactions(X, bad)
    with pytest.raises(ValueError, match="cols must be a vector"):
        s.shap_interactions(X, [0], cols=[[0, 1]])
    with pytest.raises(ValueError, match="no columns to relate"):
        s.shap_interactions(X, [0], cols=[])
    with pytest.raises(ValueError, match="cols must be integers"):
        s.shap_interactions(X, [0], cols=[0.5])
    for bad in ([0, 4], [-1, 2]):
        with pytest.raises(ValueError, match="cols must index the 4 columns of X"):
            s.shap_interactions(X, [0], cols=bad)
        with pytest.raises(ValueError, match="cols must index the 4 columns of X"):
            shap_interaction_summary(s, X, cols=bad)
    with pytest.raises(ValueError, match="cols must not name a column twice"):
        shap_interaction_values(s, X, cols=[1, 2, 1])
    with pytest.raises(ValueError, match="not both"):
        shap_interaction_values(s, X, draws=[0], samples=2)
    with pytest.raises(ValueError, match="samples must be >= 1"):
        shap_interaction_values(s, X, samples=0)
    with pytest.raises(ValueError, match="draws must be a vector"):
        shap_interaction_values(s, X, draws=[[0]])
    with pytest.raises(ValueError, match="at least 2 draws"):
        shap_interaction_summary(s, X, draws=[1])
    with pytest.raises(ValueError, match="quantiles must be in"):
        shap_interaction_summary(s, X, quantiles=[1.5])
    with pytest.raises(TypeError, match="sampler must be"):
        shap_interaction_values(object(), X)
    # a backend without the symbol (the oracle) says which one it lacks
    for call in (lambda: s.shap_interactions(X, [0, 1]), lambda: s.shap_interactions(X, [0], cols=[2, 0]),
                 lambda: shap_interaction_values(s, X), lambda: shap_interaction_summary(s, X, cols=[1]),
                 lambda: _MultiChainSampler([s, s]).shap_interactions(X, [0, 5]),
                 lambda: oracle.lib.shap_interactions_entry_point()):
        with pytest.raises(NotImplementedError, match="pgb_predict_shap_interactions"):
            call()


def test_blocks_account_for_the_square_of_the_columns(monkeypatch):
    monkeypatch.setenv("PGB_SHAP_BLOCK_BYTES", "65536")
    assert mod.blocks(2 * 1 * 2 * 2, 300) == [(0, 300)]                          # 64 B per row: 1024 rows fit
    assert mod.blocks(4 * 1 * 4 * 4, 300) == [(0, 128), (128, 256), (256, 300)]  # 512 B per row
    assert mod.blocks(4 * 3 * 5 * 5, 130) == [(0, 64), (64, 128), (128, 130)]    # 2400 B per row: never fewer than 64 rows
    monkeypatch.delenv("PGB_SHAP_BLOCK_BYTES")
    assert mod.blocks(50 * 1 * 10 * 10, 100000) == [(0, 26816), (26816, 53632), (53632, 80448), (80448, 100000)]  # 1 GiB: 40 000 B per row


@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_point(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    assert " pgb_predict_shap_interactions\n" in syms and " pgb_shap_interactions_kernel_ms\n" in syms
    assert "pgb_predict_shap_interactions" not in _abi.SYMBOLS


def test_the_library_validates_before_it_touches_a_device():
    """Every check of ``pgb_predict_shap_interactions`` precedes its first HIP call, so the library answers them
    without a GPU."""
    name, pool, fidx, X = host.pools()[1]

    def run(**kw):
        return _library_call(pool, kw.pop("table", fidx), kw.pop("width", 4), **kw)

    for name, arg in (("trees", "trees"), ("fidx", "forest_tree_idx"), ("X", "X_dev"), ("cols", "cols_host"),
                      ("picks", "picks_host"), ("out", "out_dev"), ("base", "base_host_out")):
        rc, msg = run(**{name: None})
        assert rc == E_INVALID and f"pgb_predict_shap_interactions: {arg} is null" in msg, (name, msg)
    for name in ("n_picks", "n_rows", "n_forests", "m", "n_cols"):
        for bad in (0, -1):
            rc, msg = run(**{name: bad})
            assert rc == E_INVALID and name in msg, (name, msg)
    for bad in (0, -1):
        rc, msg = run(p=bad)
        assert rc == E_INVALID and "n_forests, m and p must be >= 1" in msg, msg
    rc, msg = run(ldx=3)
    assert rc == E_INVALID and "ldx must be >= p" in msg, msg
    for bad in (4, -1):
        rc, msg = run(cols_values=[0, bad, 2])
        assert rc == E_INVALID and f"cols_host[1] = {bad} is outside [0, p = 4)" in msg, msg
    rc, msg = run(cols_values=[3, 1, 0, 1])
    assert rc == E_INVALID and "cols_host[3] = 1 repeats cols_host[1]" in msg, msg
    for bad in (3, -1):
        rc, msg = run(picks_values=[0, bad, 0])
        assert rc == E_INVALID and "picks_host[1]" in msg and "outside [0, n_forests = 3)" in msg, msg
    big = np.arange(2 ** 16, dtype=np.int32)
    rc, msg = run(width=2 ** 16, cols_values=big, n_rows=2 ** 36)
    assert rc == E_INVALID and "out_dev" in msg and "overflows" in msg, msg
    rc, msg = run(n_rows=2 ** 38)
    assert rc == E_INVALID and "n_rows exceeds" in msg, msg
    broken = np.array(fidx, np.int32)
    broken[2, 1] = 7                                              # the history, through pred_validate
    rc, msg = run(table=broken)
    assert rc == E_INVALID and "forest_tree_idx entry outside" in msg, msg
    rc, msg = run(width=2, cols_values=[0, 1])
    assert rc == E_INVALID and "column X does not have" in msg, msg
    pool.left[0] = 0                                              # a node that is its own child
    rc, msg = run()
    assert rc == E_INVALID and "do not form a tree" in msg, msg


def test_the_binding_mirrors_the_header():
    text = open(os.path.join(ROOT, "include", "pgbart_shap_interaction.h")).read()
    assert int(re.search(r"#define PGB_SHAPX_MAX_U (\d+)", text).group(1)) == _abi.SHAPX_MAX_U
    assert '#include "pgbart_shap.h"' in text and "O(u^4)" in text
    budget = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    assert sum(k.startswith("k_shap_interaction<") for k in budget) == 4
    guard = open(os.path.join(ROOT, "tools", "occupancy_guard.py")).read()
    assert '"k_shap_interaction<"' in guard                       # one wave per workgroup: 64 threads, not 256
