"""The sampler at its tree-size limits -- CPU half: the oracle at 255 nodes per tree and at depth 64.

include/pgbart.h bounds a tree at PGB_MAX_NODES = 255 nodes (node tables of 255 entries; a row's label is a byte, the
ordinal of its leaf -- 0 .. 127 in a full tree -- or 255 for a dropped row) and at PGB_MAX_DEPTH = 64 (prior_leaf[64]; a node at depth 64 is a
leaf with probability 1).  Every other sampler test stays far inside both (at most 73 nodes, depth 9).  The cap cases
of tests/_cases.py (alpha = 0.9999, beta = 0: a node splits whenever it can) drive the accepted trees into both within
8 steps.  The GPU half (tests/test_caps_gpu.py) holds the HIP library to the oracle's chains there; here the oracle's
side is pinned, and checked against arithmetic that shares no code with it:

* every (kind, variant) reaches what it is for (`check_cap_reach`) and reproduces its committed fingerprint
  (tests/golden/cap_runs.json, written by tests/golden/make_oracle_golden.py);
* the limits hold in every exported tree of every step: an odd node count <= 255, no node deeper than 64, children
  stored side by side after their parent, counts that partition;
* `sum_trees` of the last step equals the exact walk (tests/_predict_exact.py: Fraction arithmetic) of the training
  rows through the final forest, and every node's count equals a NumPy recount of the rows routed by the split rules:
  a label-table entry or a leaf value that goes wrong only in a full tree shows here;
* a chain image taken right after a full tree is stored resumes bit for bit on a fresh handle;
* the prediction validators (the oracle's and the HIP library's host check) and the SHAP packer accept the depth-64
  forests the sampler made;
* a stand-alone host program runs the oracle through a depth-64 chain under AddressSanitizer and
  UndefinedBehaviorSanitizer with strict bounds: the read `prior_leaf[depth]` never leaves its 64 entries (an
  off-by-one in the depth guard reads the field that follows the table, which today happens to be >= 1, so no chain
  shows it).
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import _predict_exact as E
from _cases import (ALL_CAPS, cap_prefix, CAP_MAX_DEPTH, CAP_MAX_NODES, cap_reach, cap_targets, check_cap_reach, digest, forest_trees,
                    make_cap, run_case, step_trees, tree_at_caps, tree_depths)
from _oracle import oracle_backend
from pymc_bart_amd import _abi
from pymc_bart_amd.image import ChainImage
from pymc_bart_amd.trees import PosteriorSampler

CAP_GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "cap_runs.json")))
CAP_IDS = [f"{k}-{v}" for k, v in ALL_CAPS]
SCALAR = [(k, v) for k, v in ALL_CAPS if v in ("normal", "linear", "mix")]
NAN_FREE = [(k, v) for k, v in ALL_CAPS if k != "both"]
DEEP = [(k, v) for k, v in ALL_CAPS if cap_targets(k, v)[1]]


@functools.lru_cache(maxsize=None)
def oracle_run(kind, variant):
    """The oracle's run of a cap case, computed once and shared (nobody changes it)."""
    c = make_cap(kind, variant)
    res = run_case(c, oracle_backend())
    return c, res, cap_reach(c, res)


def _ids(cases):
    return [f"{k}-{v}" for k, v in cases]


@pytest.mark.parametrize("kind,variant", ALL_CAPS, ids=CAP_IDS)
def test_cap_case_reaches_its_limits_and_reproduces_its_fingerprint(kind, variant):
    c, res, _ = oracle_run(kind, variant)
    check_cap_reach(c, res)
    assert digest(res) == CAP_GOLD[c["name"]]
    assert res["counters"]["saturations"] == 0


def _check_tree(c, tree, what):
    var, left, right, count = tree
    nn = len(var)
    assert nn % 2 == 1 and nn <= CAP_MAX_NODES, (what, nn)
    assert tree_depths(left, right, var).max() <= CAP_MAX_DEPTH, what
    inner = np.flatnonzero(var >= 0)
    assert np.all(right[inner] == left[inner] + 1) and np.all(left[inner] > inner) and np.all(right[inner] < nn), what
    # every node but the root is the child of exactly one split
    assert np.array_equal(np.sort(np.concatenate([left[inner], right[inner]])), np.arange(1, nn)), what
    kids = count[left[inner]] + count[right[inner]]
    assert np.all(kids <= count[inner]) and np.all(count >= 0), what
    if not np.isnan(c["X"]).any():
        assert np.array_equal(kids, count[inner]) and count[0] == c["X"].shape[0], what


@pytest.mark.parametrize("kind,variant", ALL_CAPS, ids=CAP_IDS)
def test_limits_hold_in_every_exported_tree(kind, variant):
    c, res, _ = oracle_run(kind, variant)
    assert len(res["trees"]) == c["steps"]
    for it, packed in enumerate(res["trees"]):
        for k, tree in enumerate(step_trees(c, packed)):
            _check_tree(c, tree, (c["name"], it, k))
    for k, tree in enumerate(forest_trees(res["forest"])):
        _check_tree(c, tree, (c["name"], "forest", k))


def complete_rows(X):
    return np.flatnonzero(~np.isnan(X).any(axis=1))


@pytest.mark.parametrize("kind,variant", SCALAR, ids=_ids(SCALAR))
def test_sum_trees_is_the_exact_walk_of_the_final_forest(kind, variant):
    """The tolerance of test_sum_trees_equals_sum_of_tree_predictions: atol = 1e-9, rtol = 0; rows without a missing
    value (a dropped row keeps what its tree gave it before)."""
    c, res, r = oracle_run(kind, variant)
    forest = res["forest"]
    assert max(len(t[0]) for t in forest_trees(forest)) >= 129   # (the final forest itself is at a limit)
    rows = complete_rows(c["X"])
    fidx = np.arange(c["m"], dtype=np.int32)[None, :]
    exact = E.walk(forest, fidx, c["X"][rows])
    want = np.array([float(v) for v in exact.R[0, 0]])
    np.testing.assert_allclose(res["sum_trees"][-1][rows], want, rtol=0, atol=1e-9)
    assert exact.L.max() == 0 and np.all(exact.T == c["m"])      # one leaf per tree: nothing marginalised


def numpy_counts(forest, X, rules):
    """Rows per node, by routing the training rows through the splits (the rule contract of _predict_exact.py:
    continuous left when x <= v, one-hot left when x == v); a row whose split value is missing is in neither child."""
    off = np.asarray(forest.node_off)
    out = np.zeros(forest.total_nodes, np.int64)
    for a, b in zip(off[:-1], off[1:]):
        at = {0: np.arange(X.shape[0])}
        for k in range(b - a):   # children come after their parent
            idx = at.pop(k)
            out[a + k] = idx.size
            j = int(forest.var[a + k])
            if j < 0:
                continue
            x, v = X[idx, j], forest.split[a + k]
            go_left = (x == v) if rules[j] == _abi.RULE_ONEHOT else (x <= v)
            at[int(forest.left[a + k])] = idx[go_left]
            at[int(forest.right[a + k])] = idx[~go_left & ~np.isnan(x)]
    return out


@pytest.mark.parametrize("kind,variant", NAN_FREE, ids=_ids(NAN_FREE))
def test_counts_of_the_final_forest_are_a_recount_of_the_rows(kind, variant):
    c, res, _ = oracle_run(kind, variant)
    assert not np.isnan(c["X"]).any()
    forest = res["forest"]
    assert np.array_equal(numpy_counts(forest, c["X"], c["rules"]), forest.count)
    assert np.array_equal(forest.rule[forest.var >= 0], c["rules"][forest.var[forest.var >= 0]])


@pytest.mark.parametrize("kind,variant", ALL_CAPS, ids=CAP_IDS)
def test_chain_image_with_a_full_tree_resumes_bit_for_bit(oracle, kind, variant):
    """One cut right after the first step that stores a tree at a limit: the image holds a 255-node tree (or one with
    a node at depth 64), and the fresh handle that loads it continues the chain."""
    c, res, r = oracle_run(kind, variant)
    cut = r["first_full"] + 1
    assert 1 <= cut < c["steps"]
    got = run_case(c, oracle, checkpoint_at=(cut,))
    assert digest(got) == CAP_GOLD[c["name"]]
    # the image at the cut does hold the tree at its limit, with its labels: a run stopped there says so
    stopped = run_case(cap_prefix(c, cut), oracle)
    assert np.array_equal(stopped["sum_trees"], res["sum_trees"][:cut])
    img = ChainImage.parse(stopped["sampler"].checkpoint())
    n, off = c["X"].shape[0], np.asarray(img.node_off)
    found = 0
    for t, (a, b) in enumerate(zip(off[:-1], off[1:])):
        s = tree_at_caps((img.var[a:b], img.left[a:b], img.right[a:b], img.count[a:b]), n)
        assert np.array_equal(img.depth[a:b], tree_depths(img.left[a:b], img.right[a:b], img.var[a:b]))
        if not (s["full_open"] or s["depth_cap"]):
            continue
        found += 1
        leaves = np.flatnonzero(img.var[a:b] < 0)
        assert np.array_equal(np.sort(img.label[a:b][leaves]), np.arange(leaves.size))
        # the rows' labels: every leaf of the full tree with its count, label 255 for the dropped rows
        assert np.array_equal(np.bincount(img.lid[t], minlength=256)[img.label[a:b][leaves]], img.count[a:b][leaves])
        assert (img.lid[t] == 255).sum() == n - img.count[a:b][leaves].sum()
        if s["full_open"]:
            # (a label is the leaf's ordinal, the left child keeping its parent's: 128 leaves use 0 .. 127)
            assert img.label[b - 1] == leaves.size - 1 == CAP_MAX_NODES // 2
            assert (img.lid[t] == leaves.size - 1).sum() == img.count[b - 1]
            assert img.count[b - 1] > 0 or not s["node_cap"]
    assert found > 0


@functools.lru_cache(maxsize=None)
def deep_forest(kind, variant):
    """The forest right after the first step that stores a tree with rows held at depth 64."""
    c, res, r = oracle_run(kind, variant)
    forest = run_case(cap_prefix(c, r["first_deep"] + 1), oracle_backend())["forest"]
    assert max(tree_depths(t[1], t[2], t[0]).max() for t in forest_trees(forest)) == CAP_MAX_DEPTH
    return c, forest


@pytest.mark.parametrize("kind,variant", DEEP, ids=_ids(DEEP))
def test_oracle_validator_and_shap_packer_accept_the_depth_64_forest(oracle, kind, variant):
    """pgb_pred_host.h says the prediction validators never refuse a sampler's own tree; here the sampler's deepest."""
    import _shap_host as H

    c, forest = deep_forest(kind, variant)
    X, (n, p) = c["X"], c["X"].shape
    fidx = np.arange(forest.n_trees, dtype=np.int32)[None, :].copy()
    # the oracle's pgb_predict validates, walks, and gives the exact walk on the rows without a missing value
    rows = complete_rows(X)[:40]
    ps = PosteriorSampler(forest, fidx, forest.n_trees, forest.n_outputs, backend=oracle)
    got = ps.sample_posterior(X[rows], [0])
    exact = E.walk(forest, fidx, X[rows])
    assert exact.bound_ratio(got) <= 1.0
    # the SHAP packer takes every leaf, the ones at depth 64 included
    leaf, member, off = H.records(forest, p)
    assert leaf.shape[0] == int((forest.var < 0).sum()) and off[-1] == leaf.shape[0]
    assert leaf["n_members"].max() == CAP_MAX_DEPTH


@pytest.mark.parametrize("kind,variant", DEEP, ids=_ids(DEEP))
def test_hip_library_host_check_accepts_the_depth_64_forest(kind, variant):
    """`pred_validate` of the HIP library lets the forest through: the refusal that FOLLOWS it answers (a compiled
    family without a code object), which needs no device and launches nothing.  The library must have been built."""
    from test_predict_validation import Calls

    assert os.path.exists(_abi.hip_library_path()), "libpgbart_hip.so has not been built (__graft_entry__.build())"
    c, forest = deep_forest(kind, variant)
    rc, msg = Calls(_abi.load_hip_library(), oracle_backend()).run(forest, compiled=True)["pgb_pointwise_loglik"]
    assert rc == -1 and msg == "the compiled family needs a code object", msg


# ------------------------------------------------------------------ the oracle under sanitizers, stand-alone
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZED_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "pgbart.h"
static void* slurp(const char* dir, const char* name, size_t bytes) {
  char path[4096];
  snprintf(path, sizeof path, "%s/%s", dir, name);
  FILE* f = fopen(path, "rb");
  void* buf = malloc(bytes ? bytes : 1);
  if (!f || fread(buf, 1, bytes, f) != bytes) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
  fclose(f);
  return buf;
}
#define OK(call) do { if ((call) != PGB_OK) { fprintf(stderr, "%s: %s\n", #call, pgb_last_error()); return 3; } } while (0)
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const char* dir = argv[1];
  const int steps = atoi(argv[2]);
  pgb_settings* s = slurp(dir, "settings.bin", sizeof(pgb_settings));
  const size_t n = (size_t)s->n, p = (size_t)s->p, K = (size_t)s->n_outputs;
  double* X = slurp(dir, "X.bin", 8 * n * p);
  double* y = slurp(dir, "y.bin", 8 * n);
  int32_t* rules = slurp(dir, "rules.bin", 4 * p);
  double* prior = slurp(dir, "prior.bin", 8 * p);
  double* sigma = slurp(dir, "sigma.bin", 8 * (size_t)steps);
  double* out = malloc(8 * K * n);
  int32_t* vi = malloc(4 * p);
  pgb_handle* h = NULL;
  pgb_counters ctr;
  OK(pgb_create(s, NULL, &h));
  OK(pgb_set_data(h, X, (int64_t)p, rules, prior));
  OK(pgb_set_response(h, y));
  for (int it = 0; it < steps; ++it) {
    OK(pgb_set_likelihood(h, sigma + it, 1));
    OK(pgb_step(h, it < steps / 2, out, vi, &ctr));
  }
  char path[4096];
  snprintf(path, sizeof path, "%s/sum_trees.bin", dir);
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(out, 8, K * n, f) != K * n) return 4;
  fclose(f);
  OK(pgb_destroy(h));
  free(s); free(X); free(y); free(rules); free(prior); free(sigma); free(out); free(vi);
  return 0;
}
"""


@pytest.fixture(scope="module")
def sanitized_oracle(tmp_path_factory):
    """oracle/pgbart_oracle.c and a main of its own, built with ASan + UBSan; bounds-strict also checks an array that
    is the last member of its struct, which `prior_leaf[64]` of pgb_settings is."""
    d = tmp_path_factory.mktemp("sanitized_oracle")
    (d / "main.c").write_text(SANITIZED_MAIN)
    prog = str(d / "oracle_main")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-w", "-DPGB_MAX_PARTICLES=128",
                           "-fsanitize=address,undefined,bounds-strict", "-fno-sanitize-recover=all",
                           f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "oracle", "pgbart_oracle.c"),
                           str(d / "main.c"), "-o", prog, "-lm"])
    return prog


@pytest.mark.parametrize("kind", ["chain", "both"])
def test_oracle_runs_a_depth_64_chain_clean_under_sanitizers(sanitized_oracle, tmp_path, kind):
    """The Normal case of the kind, as run_case drives it (its key, its moving sigma): no report, exit status 0, and
    the chain of the shared library -- so the program did pop nodes at depth 64."""
    from pymc_bart_amd.sampler import PyBartSettings

    c, res, r = oracle_run(kind, "normal")
    assert r["depth_cap"] > 0
    st = PyBartSettings.from_data(c["X"], c["Y"], m=c["m"], num_particles=c["P"], seed=c["seed"], batch=c["batch"],
                                  alpha=c["alpha"], beta=c["beta"])
    (tmp_path / "settings.bin").write_bytes(bytes(st.as_c()))
    np.ascontiguousarray(c["X"], np.float64).tofile(tmp_path / "X.bin")
    np.ascontiguousarray(c["Y"], np.float64).tofile(tmp_path / "y.bin")
    np.ascontiguousarray(c["rules"], np.int32).tofile(tmp_path / "rules.bin")
    np.ascontiguousarray(c["prior"], np.float64).tofile(tmp_path / "prior.bin")
    sig_rng = np.random.default_rng(99)
    np.array([0.5 + sig_rng.random() for _ in range(c["steps"])]).tofile(tmp_path / "sigma.bin")
    run = subprocess.run([sanitized_oracle, str(tmp_path), str(c["steps"])], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert np.array_equal(np.fromfile(tmp_path / "sum_trees.bin"), res["sum_trees"][-1])
