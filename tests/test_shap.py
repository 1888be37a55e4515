"""Exact Shapley attributions (``include/pgbart_shap.h``, ``pymc_bart_amd/shap.py``) without a GPU: the host build of
the header against the definition -- all ``2^p`` coalitions, each evaluated by ``_predict_exact.walk`` in ``Fraction``
arithmetic --, its exact properties, the packer against a Python restatement, and every refusal.

The tolerance.  For entry (d, k, i) ``M`` is the sum of ``|coef|`` over the leaf terms of forest d (it bounds every
``|phi_j|``) and ``T`` their number.  ``tools/shap_accuracy.py`` measures ``max |host - exact| / M`` on the pools below
and on chain trees over 16, 32 and 64 distinct columns (``profiles/shap_accuracy.json``); the tolerance here is 8 x
that figure x M, and the figure itself must lie below the crude ceiling ``(5000 + T) 2^-53``."""
import ctypes as C
import json
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import _predict_exact as ex
import _shap_host as host
from _predict_exact import Leaf, Split
from pymc_bart_amd import _abi, compiled, shap_summary, shap_values
from pymc_bart_amd import shap as shap_mod
from pymc_bart_amd.trees import PosteriorSampler
from pymc_bart_amd.utils import _MultiChainSampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1  # PGB_E_INVALID (include/pgbart.h)
U = 2.0 ** -53


@pytest.fixture(scope="module")
def accuracy():
    with open(os.path.join(ROOT, "profiles", "shap_accuracy.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def cases():
    """Per pool: the host build's result and the exact reference, computed once and left unchanged."""
    out = {}
    for name, pool, fidx, X in host.pools():
        got, base = host.rows(pool, fidx, X)
        phi, b, R = host.brute_force(pool, fidx, X)
        M, T = host.magnitude(pool, fidx, X)
        out[name] = dict(pool=pool, fidx=fidx, X=X, got=got, base=base, phi=phi, b=b, R=R, M=M, T=T)
    return out


def tolerance(accuracy, M):
    return 8.0 * accuracy["max"] * M


# ------------------------------------------------------------------ 1. against the definition
def test_the_measured_figure_lies_below_the_ceiling(accuracy):
    print(f"measured max |host - exact| / M = {accuracy['max']:.3e}; ceiling (5000 + T_min) 2^-53 = "
          f"{(5000 + accuracy['T_min']) * U:.3e}")
    assert 0.0 < accuracy["max"] < (5000 + accuracy["T_min"]) * U
    assert {"chain-16-left", "chain-32-right", "chain-64-left", "chain-64-right-linear", "mixed-K3", "edges-K1"} <= set(accuracy["cases"])
    assert accuracy["max"] == max(c["max_err_over_M"] for c in accuracy["cases"].values())


@pytest.mark.parametrize("name", ["mixed-K3", "edges-K1"])
def test_the_host_build_against_all_coalitions(cases, accuracy, name):
    c = cases[name]
    got, phi, M = c["got"], c["phi"], c["M"]
    D, K, p, n = got.shape
    assert np.all(np.isfinite(got))
    worst, nonzero = 0.0, 0
    for d in range(D):
        for k in range(K):
            for i in range(n):
                tol = tolerance(accuracy, M[d, k, i])
                for j in range(p):
                    err = abs(Fraction(float(got[d, k, j, i])) - phi[d, k, j, i])
                    nonzero += phi[d, k, j, i] != 0
                    assert abs(phi[d, k, j, i]) <= Fraction(float(M[d, k, i])), (d, k, j, i)   # M bounds every |phi_j|
                    if M[d, k, i] > 0:
                        worst = max(worst, float(err / Fraction(float(M[d, k, i]))))
                    assert err <= Fraction(tol), (d, k, j, i, float(err), tol)
    print(f"{name}: max |host - exact| / M = {worst:.3e} (tolerance 8 x {accuracy['max']:.3e}), {nonzero} of {got.size} "
          f"attributions non-zero")
    assert nonzero >= got.size // 3


@pytest.mark.parametrize("name", ["mixed-K3", "edges-K1"])
def test_efficiency_and_base(cases, accuracy, name):
    c = cases[name]
    got, base, R, M = c["got"], c["base"], c["R"], c["M"]
    D, K, p, n = got.shape
    for d in range(D):
        for k in range(K):
            assert abs(Fraction(float(base[d, k])) - c["b"][d, k]) <= Fraction(tolerance(accuracy, float(M[d, k].max())))
            for i in range(n):
                total = Fraction(float(base[d, k])) + sum(Fraction(float(v)) for v in got[d, k, :, i])
                assert abs(total - R[d, k, i]) <= (p + 1) * Fraction(tolerance(accuracy, M[d, k, i])), (d, k, i)
                assert sum(c["phi"][d, k, :, i]) + c["b"][d, k] == R[d, k, i]       # (exactly, in the definition)


def test_the_leafwise_form_is_the_definition(cases):
    for name, c in cases.items():
        lw, lb, _, _ = host.restated(c["pool"], c["fidx"], c["X"], Fraction)
        assert np.all(lw == c["phi"]) and np.all(lb == c["b"]), name


# ------------------------------------------------------------------ 2. exact properties
def test_the_stated_order_of_operations(cases):
    """The header restated in Python floats -- the same operations in the stated order -- gives the same bits; the
    forests [5, 0, 0] and [1, 1, 4, 4, 3] repeat trees: their sums are the ones the order implies."""
    for name, c in cases.items():
        phi, base, _, _ = host.restated(c["pool"], c["fidx"], c["X"], float)
        assert np.array_equal(phi, c["got"]) and np.array_equal(base, c["base"]), name
        general, gb = host.rows(c["pool"], c["fidx"], c["X"], general=True)
        assert np.array_equal(general, c["got"]) and np.array_equal(gb, c["base"]), name
        wide, wb = host.rows(c["pool"], c["fidx"], c["X"], ldx=c["X"].shape[1] + 3)
        assert np.array_equal(wide, c["got"]), name
        picks = [2, 0, 2]
        again, ab = host.rows(c["pool"], c["fidx"], c["X"], picks=picks)
        assert np.array_equal(again, c["got"][picks]) and np.array_equal(ab, c["base"][picks]), name


def test_one_tree_repeated_twice():
    """A forest that names one tree twice adds the tree's leaf terms twice, in order: for a single split (u = 1, W = 1)
    a row that goes left gets (((0 + a (1 - fl)) + b (0 - fr)) + a (1 - fl)) + b (0 - fr)."""
    a, b, fl, fr = 0.3, -1.7, 3 / 10, 7 / 10
    pool = ex.build_pool([Split(0, 0.5, Leaf([a], count=3), Leaf([b], count=7))], 1)
    X = np.array([[0.25, 0.0], [0.75, 0.0], [math.nan, 0.5]])
    twice, b2 = host.rows(pool, np.array([[0, 0]], np.int32), X)
    phi, base, _, _ = host.restated(pool, np.array([[0, 0]]), X, float)
    assert np.array_equal(twice, phi) and np.array_equal(b2, base)
    tl, tr = (a * 1.0) * ((1.0 - fl) * 1.0), (b * 1.0) * ((0.0 - fr) * 1.0)
    assert twice[0, 0, 0, 0] == (((0.0 + tl) + tr) + tl) + tr
    tl, tr = (a * 1.0) * ((0.0 - fl) * 1.0), (b * 1.0) * ((1.0 - fr) * 1.0)
    assert twice[0, 0, 0, 1] == (((0.0 + tl) + tr) + tl) + tr
    assert twice[0, 0, 0, 2] == 0.0 and np.all(twice[0, 0, 1] == 0.0)
    assert b2[0, 0] == (((0.0 + a * fl) + b * fr) + a * fl) + b * fr


def test_nan_entries_unused_columns_and_stumps(cases):
    for name, c in cases.items():
        got, X = c["got"], c["X"]
        nan = np.isnan(X)                                            # (n, p)
        assert nan.any()
        where = np.broadcast_to(nan.T[None, None], got.shape)
        assert np.all(got[where] == 0.0) and not np.signbit(got[where]).any(), name
    e = cases["edges-K1"]
    assert not (np.asarray(e["pool"].var) == 3).any() and not (np.asarray(e["pool"].svar) == 3).any()
    assert np.all(e["got"][:, :, 3, :] == 0.0)                       # a column no tree uses
    assert np.all(e["got"][1] == 0.0) and e["base"][1, 0] == 3.25 * 5 and all(v == 0 for v in e["phi"][1].ravel())  # stumps: u = 0
    all_nan = np.isnan(e["X"]).all(axis=1)
    assert all_nan.any() and np.all(e["got"][:, :, :, all_nan] == 0.0)
    for d in range(3):                                               # ... where the base value is the prediction
        assert abs(Fraction(float(e["base"][d, 0])) - e["R"][d, 0, int(np.flatnonzero(all_nan)[0])]) <= Fraction(1e-15)


def test_the_edges_are_the_walks():
    """-0.0 goes left at a split at 0.0 like 0.0; the smallest positive double goes right; infinities compare as the
    extended reals do: the attributions of rows that differ only there are the bits of each other or not at all."""
    pool = ex.build_pool([Split(0, 0.0, Leaf([1.5], count=3), Leaf([-2.25], count=5))], 1)
    X = np.array([[-0.0], [0.0], [5e-324], [-math.inf], [math.inf]])
    got, base = host.rows(pool, np.array([[0]], np.int32), X)
    left, right = 1.5 * (1.0 - 3 / 8) + -2.25 * (0.0 - 5 / 8), 1.5 * (0.0 - 3 / 8) + -2.25 * (1.0 - 5 / 8)
    assert got[0, 0, 0].tolist() == [left, left, right, left, right]
    assert base[0, 0] == (0.0 + 1.5 * (3 / 8)) + -2.25 * (5 / 8)


def test_the_weights_follow_their_recurrence():
    f = math.factorial
    for u in (1, 2, 3, 8, 9, 33, 64, host.max_u()):
        w = host.weights(u)
        v, want = 1.0 / u, []
        for k in range(u):
            if k:
                v = (v * k) / (u - k)
            want.append(v)
        assert w.tolist() == want
        exact = [Fraction(f(k) * f(u - k - 1), f(u)) for k in range(u)]
        assert sum(exact[k] * math.comb(u - 1, k) for k in range(u)) == 1
        assert max(abs(Fraction(float(w[k])) / exact[k] - 1) for k in range(u)) <= 2 * u * Fraction(U)
    assert host.max_u() == _abi.MAX_DEPTH + 1 and host.fast_u() == _abi.SHAP_FAST_U


def test_paths_around_the_fast_length():
    """Chain trees of u = 1, the unrolled evaluation's last length, the next one and 20, with and without a regressor
    that adds a slot: the host build against its Python restatement, bit for bit, and against exact arithmetic."""
    fast = host.fast_u()
    for depth, linear in ((1, ()), (fast - 1, (fast,)), (fast, ()), (fast, (fast + 1,)), (fast + 1, ()), (20, (3, 21))):
        pool, fidx, rng = host.chain_pool(depth, K=2, side="right" if depth % 2 else "left", linear=linear)
        X = host.chain_rows(pool, depth, depth + 3, rng, n=4)
        got, base = host.rows(pool, fidx, X)
        phi, b, _, _ = host.restated(pool, fidx, X, float)
        assert np.array_equal(got, phi) and np.array_equal(base, b), depth
        assert np.count_nonzero(got) >= depth


# ------------------------------------------------------------------ 3. the packer
def test_the_packer_on_a_three_leaf_tree():
    root = Split(2, 0.5, Leaf([1.0, 2.0], count=3, svar=1, slope=[0.5, 0.25], xbar=0.125),
                 Split(2, 0.75, Leaf([3.0, 4.0], count=0, svar=2, slope=[1.0, -1.0], xbar=0.5), Leaf([5.0, 6.0], count=9, svar=7,
                                                                                                      slope=[1.0, 1.0]),
                       rule=ex.ONEHOT, count=9), count=12)
    pool = ex.build_pool([Leaf([9.0, 9.0]), root], 2)
    leaf, member, off = host.records(pool, 3)
    assert off.tolist() == [0, 1, 4]
    assert leaf[0].tolist() == (0, 0, 0, 0, -1, -1, 0.0)                                   # the stump
    base = int(pool.node_off[1])
    want_nodes = [g for g, _ in host.leaves(pool, 1)]
    assert leaf["node"][1:].tolist() == want_nodes == [base + 1, base + 3, base + 4]       # depth-first, left first
    assert leaf["n_members"][1:].tolist() == [1, 2, 2] and leaf["n_groups"][1:].tolist() == [1, 1, 1]
    assert leaf["first"].tolist() == [0, 0, 1, 3]
    assert leaf["svar"][1:].tolist() == [1, 2, -1]                                         # column 7: X does not have it
    assert leaf["sgroup"][1:].tolist() == [-1, 0, -1] and leaf["xbar"][1:].tolist() == [0.125, 0.5, 0.0]
    want = []
    for g, path in host.leaves(pool, 1):
        for j, members in host.groups_of(path):
            for k, mb in enumerate(members):
                want.append((mb[0], mb[1], mb[2], (host.HEAD if k == 0 else 0) | (host.TAIL if k == len(members) - 1 else 0), mb[3], mb[4]))
    assert member.tolist() == want
    assert member["frac"].tolist() == [3 / 12, 9 / 12, 0 / 9, 9 / 12, 9 / 9]
    assert member["side"].tolist() == [0, 1, 0, 1, 1] and member["rule"].tolist() == [0, 0, 1, 0, 1]
    # groups in order of first appearance, path order inside a group
    root = Split(1, 0.0, Split(0, 1.0, Split(1, -1.0, Leaf([1.0, 1.0], count=0), Leaf([2.0, 2.0], count=0)), Leaf([0.0, 0.0])), Leaf([0.0, 0.0]))
    leaf, member, off = host.records(ex.build_pool([root], 2), 2)
    assert leaf["n_groups"].tolist() == [2, 2, 2, 1] and member["var"][:3].tolist() == [1, 1, 0]
    assert member["flags"][:3].tolist() == [host.HEAD, host.TAIL, host.HEAD | host.TAIL]
    assert member["split"][:3].tolist() == [0.0, -1.0, 1.0] and member["frac"][:3].tolist() == [0.5, 0.0, 0.5]   # a pair of counts 0, 0


# ------------------------------------------------------------------ 4. refusals, the binding, the library
@pytest.fixture(scope="module")
def hand(oracle):
    name, pool, fidx, X = host.pools()[1]
    return PosteriorSampler(pool, fidx, fidx.shape[1], 1, backend=oracle), X


def test_refusals_of_the_python_layer(hand, oracle):
    s, X = hand
    with pytest.raises(ValueError, match="X must be a matrix"):
        s.shap(np.zeros((0, 4)), [0])
    with pytest.raises(ValueError, match="X must be a matrix"):
        s.shap(np.zeros((2, 3, 4)), [0])
    with pytest.raises(ValueError, match="picks must be a vector"):
        s.shap(X, [[0, 1]])
    with pytest.raises(ValueError, match="no draws to attribute"):
        s.shap(X, [])
    for bad in ([0, 3], [-1]):
        with pytest.raises(ValueError, match="picks must index the 3 stored draws"):
            s.shap(X, bad)
    with pytest.raises(ValueError, match="not both"):
        shap_values(s, X, draws=[0], samples=2)
    with pytest.raises(ValueError, match="samples must be >= 1"):
        shap_values(s, X, samples=0)
    with pytest.raises(ValueError, match="draws must be a vector"):
        shap_values(s, X, draws=[[0]])
    with pytest.raises(ValueError, match="at least 2 draws"):
        shap_summary(s, X, draws=[1])
    with pytest.raises(ValueError, match="quantiles must be in"):
        shap_summary(s, X, quantiles=[1.5])
    with pytest.raises(TypeError, match="sampler must be"):
        shap_values(object(), X)
    # a backend without the symbol (the oracle) says which one it lacks
    for call in (lambda: s.shap(X, [0, 1]), lambda: shap_values(s, X), lambda: shap_summary(s, X),
                 lambda: _MultiChainSampler([s, s]).shap(X, [0, 5]), lambda: oracle.lib.shap_entry_point()):
        with pytest.raises(NotImplementedError, match="pgb_predict_shap"):
            call()


def test_blocks_are_multiples_of_64_under_the_limit(monkeypatch):
    monkeypatch.setenv("PGB_SHAP_BLOCK_BYTES", "65536")
    assert shap_mod.blocks(2 * 1 * 4, 300) == [(0, 300)]                     # 64 rows x 64 B = 4 KiB: 1024 rows fit
    assert shap_mod.blocks(4 * 3 * 5, 300) == [(0, 128), (128, 256), (256, 300)]
    assert shap_mod.blocks(64 * 16 * 100, 130) == [(0, 64), (64, 128), (128, 130)]   # never fewer than 64 rows
    monkeypatch.delenv("PGB_SHAP_BLOCK_BYTES")
    assert shap_mod.blocks(50 * 1 * 50, 100000) == [(0, 53632), (53632, 100000)]      # 1 GiB: 20 000 B per row


@pytest.mark.parametrize("so", ["libpgbart_hip.so", "libpgbart_hip_p128.so"])
def test_both_library_builds_export_the_entry_point(so):
    path = os.path.join(ROOT, "pymc_bart_amd", "csrc", so)
    syms = subprocess.check_output([os.path.join(compiled.LLVM, "llvm-readelf"), "--dyn-syms", path], text=True)
    assert " pgb_predict_shap\n" in syms and " pgb_shap_kernel_ms\n" in syms and "pgb_predict_shap" not in _abi.SYMBOLS


def test_the_library_validates_before_it_touches_a_device():
    """Every check of ``pgb_predict_shap`` precedes its first HIP call, so the library answers them without a GPU."""
    lib = _abi.load_hip_library()
    call = lib.shap_entry_point()
    name, pool, fidx, X = host.pools()[1]
    fidx = np.ascontiguousarray(fidx, np.int32)
    carr = pool.as_c()
    buf = np.zeros(64)                                            # stands in for device memory: never dereferenced
    picks = np.zeros(3, np.int32)

    def run(**kw):
        a = dict(trees=C.byref(carr), fidx=fidx.ctypes.data, n_forests=3, m=5, X=buf.ctypes.data, n_rows=8, p=4, ldx=4,
                 picks=picks.ctypes.data, n_picks=3, out=buf.ctypes.data, base=buf.ctypes.data)
        a.update(kw)
        rc = call(a["trees"], a["fidx"], a["n_forests"], a["m"], a["X"], a["n_rows"], a["p"], a["ldx"], a["picks"],
                  a["n_picks"], a["out"], a["base"], None)
        return rc, lib.lib.pgb_last_error().decode()

    for name, arg in (("trees", "trees"), ("fidx", "forest_tree_idx"), ("X", "X_dev"), ("picks", "picks_host"),
                      ("out", "out_dev"), ("base", "base_host_out")):
        rc, msg = run(**{name: None})
        assert rc == E_INVALID and f"pgb_predict_shap: {arg} is null" in msg, (name, msg)
    for name in ("n_picks", "n_rows", "n_forests", "m", "p"):
        for bad in (0, -1):
            rc, msg = run(**{name: bad})
            assert rc == E_INVALID and name in msg, (name, msg)
    rc, msg = run(ldx=3)
    assert rc == E_INVALID and "ldx must be >= p" in msg, msg
    for bad in (3, -1):
        picks[1] = bad
        rc, msg = run()
        assert rc == E_INVALID and "picks_host[1]" in msg and "outside [0, n_forests = 3)" in msg, msg
    picks[1] = 0
    rc, msg = run(p=2 ** 31 - 1, ldx=2 ** 31, n_rows=2 ** 36)
    assert rc == E_INVALID and "out_dev" in msg and "overflows" in msg, msg
    rc, msg = run(n_rows=2 ** 38)
    assert rc == E_INVALID and "n_rows exceeds" in msg, msg
    broken = fidx.copy()
    broken[2, 1] = 7                                              # the history, through pred_validate
    rc, msg = run(fidx=broken.ctypes.data)
    assert rc == E_INVALID and "forest_tree_idx entry outside" in msg, msg
    rc, msg = run(p=2)
    assert rc == E_INVALID and "column X does not have" in msg, msg
    pool.left[0] = 0                                              # a node that is its own child
    rc, msg = run()
    assert rc == E_INVALID and "do not form a tree" in msg, msg


def test_the_binding_mirrors_the_header():
    text = open(os.path.join(ROOT, "include", "pgbart_shap.h")).read()
    assert int(re.search(r"#define PGB_SHAP_FAST_U (\d+)", text).group(1)) == _abi.SHAP_FAST_U
    assert "#define PGB_SHAP_MAX_U (PGB_MAX_DEPTH + 1)" in text
    budget = json.load(open(os.path.join(ROOT, "profiles", "occupancy_budget.json")))["kernels"]
    assert sum(k.startswith("k_shap<") for k in budget) == 8
    guard = open(os.path.join(ROOT, "tools", "occupancy_guard.py")).read()
    assert '"k_shap<"' in guard                                   # one wave per workgroup: 64 threads, not 256
