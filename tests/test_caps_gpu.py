"""The sampler at its tree-size limits -- GPU half: the HIP library at 255 nodes per tree and at depth 64.

The cap cases (tests/_cases.py: ALL_CAPS) put accepted trees on both limits of include/pgbart.h within 8 steps: the
two `f_nodes + 2 <= MAXN` guards and the `depth < PGB_MAX_DEPTH` reads of the control kernel, the 256-entry
label-to-value tables of the row passes filled for 128 leaves (next to the label of dropped rows, 255), the
[2][MAXP][MAXN] particle tables copied whole at resampling, the export and the chain image with `parents[255]` in use.
Every comparison with the oracle is exact; what each case reaches, and the oracle's own arithmetic at the limits, is
pinned in tests/test_caps.py."""
import ctypes as C

import numpy as np
import pytest

import _predict_exact as E
from _cases import ALL_CAPS, CAP_MAX_NODES, cap_prefix, cap_reach, digest, random_cap_case, run_case
from pymc_bart_amd import _abi
from pymc_bart_amd.image import ChainImage, differing_fields
from pymc_bart_amd.sampler import Backend, PyBartSettings, PySampler
from pymc_bart_amd.trees import PosteriorSampler, TreeArrays
from test_caps import CAP_GOLD, CAP_IDS, complete_rows, oracle_run
from test_parity_gpu import _assert_same
from test_wide_gpu import _same_forest

pytestmark = pytest.mark.gpu

ONE_PER_KIND = [("chain", "linear"), ("bushy", "categorical_k3"), ("both", "normal")]
ONE_IDS = [f"{k}-{v}" for k, v in ONE_PER_KIND]


def _same_image(a, b):
    """The chain images of two samplers: equal field for field, up to who wrote them and the launch counter."""
    ia, ib = ChainImage.parse(a.checkpoint()), ChainImage.parse(b.checkpoint())
    assert differing_fields(ia, ib) == []
    return ia


def _p128(hip):
    big = Backend(lib=_abi.load_hip_library(128), mem=hip.mem)
    assert big.lib.max_particles == 128 and hip.lib.max_particles == 64
    return big


@pytest.mark.parametrize("kind,variant", ALL_CAPS, ids=CAP_IDS)
def test_cap_hip_equals_oracle_and_golden(hip, kind, variant):
    c, o, _ = oracle_run(kind, variant)
    g = run_case(c, hip)
    lib = g["sampler"].backend.lib
    assert lib.backend_name == "hip-gfx950" and lib.max_particles == (128 if c["P"] > 64 else 64)
    _assert_same(g, o)
    _same_forest(g, o)
    for f in ("slope", "xbar", "svar", "rule"):
        assert np.array_equal(getattr(g["forest"], f), getattr(o["forest"], f)), f
    assert digest(g) == CAP_GOLD[c["name"]]
    assert g["counters"]["saturations"] == 0
    _same_image(g["sampler"], o["sampler"])


@pytest.mark.parametrize("kind,variant", ONE_PER_KIND, ids=ONE_IDS)
def test_cap_two_particles_per_lane_build_gives_the_same_chain(hip, kind, variant):
    c, o, _ = oracle_run(kind, variant)
    assert c["P"] <= 64
    g = run_case(c, _p128(hip))
    assert g["sampler"].backend.lib.max_particles == 128
    _assert_same(g, o)
    assert digest(g) == CAP_GOLD[c["name"]]
    _same_image(g["sampler"], o["sampler"])


KNOBS = {
    # the 16-bit order keys / float32 shadow of the split columns, forced on at test sizes
    "order keys and float32 shadow forced": {"PGB_X32_MIN_MB": "0"},
    "odd launch geometry": {"PGB_ROWS_GRID": "7", "PGB_ROWS_TARGET": "3", "PGB_ROWS_TARGET_INIT": "5", "PGB_LL_GRID": "5",
                            "PGB_LL_TARGET": "2"},
    "wide launch geometry": {"PGB_ROWS_GRID": "333", "PGB_ROWS_TARGET": "100000", "PGB_ROWS_TARGET_INIT": "1",
                             "PGB_LL_GRID": "1000", "PGB_LL_TARGET": "99999"},
}


@pytest.mark.parametrize("knob", list(KNOBS))
@pytest.mark.parametrize("kind,variant", ONE_PER_KIND + [("both", "probit"), ("bushy", "normal")],
                         ids=ONE_IDS + ["both-probit", "bushy-normal"])
def test_cap_chain_does_not_depend_on_the_knobs(hip, monkeypatch, kind, variant, knob):
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)
    c, o, _ = oracle_run(kind, variant)
    g = run_case(c, hip)
    assert g["sampler"].backend.lib.backend_name == "hip-gfx950"
    _assert_same(g, o)
    assert digest(g) == CAP_GOLD[c["name"]]


def _pair(c, backend_a, backend_b):
    X, Y = c["X"], c["Y"]
    st = PyBartSettings.from_data(X, c.get("bart_Y", Y), m=c["m"], num_particles=c["P"], seed=c["seed"],
                                  family=c.get("family", "normal"), n_outputs=c.get("K", 1),
                                  response=c.get("response", "constant"), batch=c["batch"], alpha=c["alpha"], beta=c["beta"],
                                  compat=c.get("compat", 0))
    return st, [PySampler(st, X, Y, c["rules"], c["prior"], backend=b) for b in (backend_a, backend_b)]


@pytest.mark.parametrize("kind,variant", ONE_PER_KIND, ids=ONE_IDS)
def test_cap_host_output_step_equals_the_device_output_step(hip, kind, variant):
    """pgb_step_host against pgb_step on the case's own chain (run_case's key and moving sigma): the step output and
    the tree record served from the mapped block hold full trees."""
    c, o, r = oracle_run(kind, variant)
    st, (a, b) = _pair(c, hip, hip)
    K, n = st.n_outputs, st.n
    sig_rng = np.random.default_rng(99)
    for it in range(c["steps"]):
        sig = float(0.5 + sig_rng.random())
        for s in (a, b):
            s.set_likelihood([sig] if st.family == "normal" else [])
        sa, va = a.step(it < c["steps"] // 2)                    # host path
        _, vb = b.step(it < c["steps"] // 2, fetch=False)        # device path
        sb = hip.mem.to_host(b.sum_trees_device())
        sb = sb.reshape(K, n) if K > 1 else sb
        assert np.array_equal(sa, sb) and np.array_equal(va, vb)
        assert np.array_equal(sa, o["sum_trees"][it])            # (the chain whose reach is pinned)
        ta, tb = a.export_trees(0), b.export_trees(0)
        for f in ("tree_id", "node_off", "var", "left", "right", "count", "split", "value", "slope", "xbar", "svar"):
            assert np.array_equal(getattr(ta, f), getattr(tb, f)), f
        assert a.counters.as_dict() == b.counters.as_dict()


@pytest.mark.parametrize("kind,variant", ONE_PER_KIND, ids=ONE_IDS)
def test_cap_chain_migrates_at_the_cut_where_a_full_tree_is_stored(hip, oracle, kind, variant):
    """HIP -> oracle right after the first step that stores a tree at a limit -> the two-particles-per-lane build two
    steps later: the image carries the full node table and its labels across."""
    c, o, r = oracle_run(kind, variant)
    cut = r["first_full"] + 1
    g = run_case(c, hip, checkpoint_at={cut: oracle, cut + 2: _p128(hip)})
    assert g["sampler"].backend.lib.max_particles == 128
    _assert_same(g, o)
    assert digest(g) == CAP_GOLD[c["name"]]
    _same_image(g["sampler"], o["sampler"])
    # the images at the cut itself, written by the two backends
    stopped = cap_prefix(c, cut)
    ia = _same_image(run_case(stopped, hip)["sampler"], run_case(stopped, oracle)["sampler"])
    assert np.diff(ia.node_off).max() == CAP_MAX_NODES or ia.depth.max() == 64


@pytest.mark.parametrize("kind,variant", [("bushy", "normal"), ("both", "categorical_k3"), ("both", "linear")])
def test_cap_packed_tree_record_equals_the_array_export(hip, oracle, kind, variant):
    """As test_packed_tree_record_on_gpu_equals_the_array_export, on batches that contain 255-node trees: the record
    served from the mapped block (host-output step) and the one fetched from the device."""
    c, o, r = oracle_run(kind, variant)
    st, (g, q) = _pair(c, hip, oracle)

    def arrays(s_, which):
        lib = s_.backend.lib
        cc = _abi.TreeArraysC()
        lib.check(lib.lib.pgb_export_trees(s_._h, which, C.byref(cc)), "size")
        ta = TreeArrays.empty(cc.n_trees, cc.total_nodes, cc.n_outputs)
        c2 = ta.as_c()
        lib.check(lib.lib.pgb_export_trees(s_._h, which, C.byref(c2)), "fill")
        return ta

    sig_rng = np.random.default_rng(99)
    full = 0
    for it in range(c["steps"]):
        sig = float(0.5 + sig_rng.random())
        for s_ in (g, q):
            s_.set_likelihood([sig] if st.family == "normal" else [])
            s_.step(it < c["steps"] // 2, fetch=it % 2 == 0)
        for which in (0, 1):
            pg, po, ag = g.export_trees(which), q.export_trees(which), arrays(g, which)
            assert pg.raw == po.raw
            for f in ("tree_id", "node_off", "var", "split", "left", "right", "count", "value"):
                assert np.array_equal(getattr(pg, f), getattr(ag, f)), (it, which, f)
            full += int(np.diff(ag.node_off).max() == CAP_MAX_NODES)
    assert full >= 2


# ------------------------------------------------------------------ device consumers of the grown forest
@pytest.fixture(scope="module", params=[("chain", "linear"), ("both", "normal"), ("both", "mix")], ids=lambda kv: "-".join(kv))
def grown(request, hip):
    """(case, forest at a limit, its PosteriorSampler on the device, 65 rows): the forest right after the first step
    that stores a tree at a limit, grown by the HIP library; two "draws" -- the trees in both orders."""
    kind, variant = request.param
    c, o, r = oracle_run(kind, variant)
    g = run_case(cap_prefix(c, r["first_full"] + 1), hip)
    forest = g["forest"]
    assert forest.n_trees == 2
    sizes = np.diff(forest.node_off)
    depth = max(E.tree_depth(forest, t) for t in range(2))
    assert sizes.max() == CAP_MAX_NODES or depth == 64
    fidx = np.array([[0, 1], [1, 0]], np.int32)
    X = c["X"][:65].copy()
    return c, forest, PosteriorSampler(forest, fidx, 2, 1, backend=hip), X, g


def test_cap_predict_equals_the_exact_walk(grown):
    c, forest, ps, X, g = grown
    rows = complete_rows(c["X"])
    got = ps.sample_posterior(c["X"][rows], [0, 1])
    exact = E.walk(forest, ps.forest_idx, c["X"][rows])
    ratio = exact.bound_ratio(got)
    print(f"{c['name']}: |device - exact| / bound = {ratio:.3f} over {rows.size} training rows")
    assert ratio <= 1.0
    # ... which is the sampler's own sum_trees on those rows
    np.testing.assert_allclose(got[0, 0], g["sum_trees"][-1][rows], rtol=0, atol=1e-9)
    # rows with a missing value: both subtrees, weighted by the counts
    part = ps.sample_posterior(X, [0, 1])
    assert E.walk(forest, ps.forest_idx, X).bound_ratio(part) <= 1.0


def test_cap_pointwise_log_likelihood_equals_the_host(grown):
    from pymc_bart_amd import NormalLikelihood
    from pymc_bart_amd.pointwise import pointwise_log_likelihood
    from test_pointwise_gpu import _host_matrix

    c, forest, ps, X, g = grown
    lik, y = NormalLikelihood("sigma"), c["Y"][:65]
    pts = {"sigma": np.array([0.7, 1.3])}
    got, nc = pointwise_log_likelihood(ps, X, y, lik, points=pts, return_clamped=True)
    want, nc_host = _host_matrix(ps, lik, X, y, [0, 1], pts)
    assert got.shape == (2, 65) and np.array_equal(got, want) and nc == nc_host == 0


def test_cap_pdp_sweep_equals_the_host(grown, oracle):
    from test_pdp_gpu import _check

    c, forest, ps, X, g = grown
    cols = list(range(X.shape[1]))
    _check(ps, np.nan_to_num(X), cols, np.array([[0, 1]] * len(cols)), oracle)


def test_cap_ice_equals_the_host(grown):
    from test_ice_gpu import _check

    c, forest, ps, X, g = grown
    cols = list(range(X.shape[1]))
    inst = X[[3, 40]].copy()
    _check(ps, X, inst, cols, np.tile(np.array([0, 1, 1]), (len(cols), 2, 1)))


def test_cap_shap_values_equal_the_host(grown):
    from test_shap_gpu import _check

    c, forest, ps, X, g = grown
    got, base = _check(ps, X, [0, 1, 0])
    assert np.count_nonzero(got) > 0 and np.all(got[:, :, np.isnan(X)] == 0.0)


# ------------------------------------------------------------------ fuzz at the limits
FUZZ_SEEDS = range(9002, 9026)


def test_cap_fuzz_parity_at_the_limits(hip, oracle):
    """24 random configurations around the limits (tests/_cases.py: random_cap_case), HIP == oracle on every one.  The
    window draws every particle count, every row count, every kind and every compat value of the generator; at least
    18 of the 24 oracle runs are stopped by a limit -- a 255-node tree with leaves that would still split, or rows
    held in a leaf at depth 64 (measured on the oracle: 22)."""
    reached, drawn = [], []
    for seed in FUZZ_SEEDS:
        c = random_cap_case(seed)
        drawn.append((c["P"], c["X"].shape[0], c["kind"], c["compat"]))
        o = run_case(c, oracle)
        g = run_case(c, hip)
        assert g["sampler"].backend.lib.max_particles == (128 if c["P"] > 64 else 64)
        assert digest(g) == digest(o), (seed, c["kind"], c["family"], c["X"].shape, c["m"], c["P"], c["K"], c["compat"])
        _same_image(g["sampler"], o["sampler"])
        r = cap_reach(c, o)
        reached.append(r["full_open"] > 0 or r["depth_cap"] > 0)
    P, n, kinds, compat = (set(col) for col in zip(*drawn))
    assert P == {2, 10, 64, 65, 128} and n == {128, 129, 255, 257, 1025, 2049}
    assert kinds == {"chain", "bushy", "both"} and compat == {0, 1, 2, 3}
    print(f"cap fuzz: {sum(reached)} of {len(reached)} oracle runs reach a limit")
    assert sum(reached) >= 18
