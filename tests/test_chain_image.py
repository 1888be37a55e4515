"""The chain image (include/pgbart_image.h, pgb_checkpoint_*): CPU half -- the oracle writes and reads the record
every backend shares; the layout is pinned from Python, and damaged records are errors.  The GPU half (the HIP
library writes the same bytes, chains migrate between backends, the oracle resumes a GPU chain after its burn-in)
is tests/test_steady_state_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from _cases import CASES, digest, make_case, run_case
from _image_edits import EDIT_CASES, image_edits
from pymc_bart_amd import _abi
from pymc_bart_amd.image import ChainImage, ImageHeader, differing_fields
from pymc_bart_amd.sampler import PyBartSettings, PySampler

ROUND_TRIP = ["nan_onehot_prior", "categorical_k4_cfg5_small", "linear_response", "categorical_k3_mix", "subset_rule",
              "probit_cfg4_small", "upstream/onehot_fail_nan", "one_tree_two_particles"]


@pytest.mark.parametrize("name", ROUND_TRIP)
def test_oracle_chain_resumed_from_its_image_is_the_uninterrupted_chain(oracle, name):
    c = make_case(name)
    cuts = (1, c["steps"] // 2 - 1, c["steps"] // 2 + 2)
    assert digest(run_case(c, oracle, checkpoint_at=cuts)) == digest(run_case(c, oracle))


def _sampler(c, backend, seed=None):
    X, Y = c["X"], c["Y"]
    p = X.shape[1]
    st = PyBartSettings.from_data(X, c.get("bart_Y", Y), m=c["m"], num_particles=c["P"], seed=c["seed"] if seed is None else seed,
                                  batch=c["batch"], family=c.get("family", "normal"), n_outputs=c.get("K", 1),
                                  response=c.get("response", "constant"), compat=c.get("compat", 0))
    rules = np.zeros(p, np.int32) if c["rules"] is None else c["rules"]
    prior = np.ones(p) if c["prior"] is None else c["prior"]
    s = PySampler(st, X, Y, rules, prior, backend=backend)
    s.set_likelihood([0.8] if c.get("family", "normal") == "normal" else c.get("lik_params", []))
    return s


def test_image_layout_as_documented(oracle):
    """The record parsed by an independent reader (pymc_bart_amd/image.py follows the header's text, not its code):
    header fields, section sizes, and the content against what the ABI's own getters report."""
    c = make_case("categorical_k3_mix")
    s = _sampler(c, oracle)
    for it in range(9):
        s.step(it < 6)
    blob = s.checkpoint()
    img = ChainImage.parse(blob)
    hd = img.header
    assert hd.header_bytes == C.sizeof(ImageHeader) and hd.total_bytes == len(blob) and img.writer == "oracle-cpu"
    assert bytes(hd.s) == bytes(s.settings.as_c())
    stt = s.state()
    assert hd.iter == stt["iter"] and hd.lower == stt["lower"] and np.array_equal(img.leaf_sd, stt["leaf_sd"])
    assert hd.rs_count == 6 * s.settings.batch_sizes()[0]
    n, K, m = s.settings.n, 3, s.settings.m
    assert img.sum_trees.shape == (K, n) and img.lid.shape == (m, n)
    forest = s.export_trees(1)
    assert np.array_equal(img.node_off, forest.node_off) and np.array_equal(img.var, forest.var)
    assert np.array_equal(img.count, forest.count) and np.array_equal(img.value, forest.value)
    assert np.array_equal(img.slope, forest.slope) and np.array_equal(img.svar, forest.svar)
    assert np.array_equal(img.left, forest.left) and np.array_equal(img.right, forest.right)
    # the labels say which leaf every row sits in: the row counts of the leaves, and sum_trees itself
    base = np.repeat(img.node_off[:-1], np.diff(img.node_off))
    for t in (0, m - 1):
        sl = slice(img.node_off[t], img.node_off[t + 1])
        leaves = np.flatnonzero(img.var[sl] < 0)
        for k in leaves:
            assert np.count_nonzero(img.lid[t] == img.label[sl][k]) == img.count[sl][k]
    assert base.size == hd.total_nodes
    # split weights: alpha in the units of the caller's prior
    w = s.split_weights()
    assert np.allclose(img.alpha / img.alpha.sum(), w / w.sum(), rtol=1e-12)
    assert np.array_equal(np.cumsum(img.alpha)[-1:] >= img.cdf[-1:], [True])  # the sampler's sums may lag the weights
    # a second image of the same state is the same bytes; one step later it is not the same chain state
    assert s.checkpoint() == blob
    s.step(False)
    assert "sum_trees" in differing_fields(ChainImage.parse(s.checkpoint()), img)


def test_loading_an_image_then_saving_gives_the_same_bytes(oracle):
    c = make_case("nan_onehot_prior")
    a = _sampler(c, oracle)
    for it in range(7):
        a.step(it < 4)
    blob = a.checkpoint()
    b = _sampler(c, oracle)
    b.restore(blob)
    assert b.checkpoint() == blob
    sa, va = a.step(False)
    sb, vb = b.step(False)
    assert np.array_equal(sa, sb) and np.array_equal(va, vb)
    assert a.counters.as_dict() == b.counters.as_dict()
    ta, tb = a.export_trees(0), b.export_trees(0)
    for f in ("tree_id", "node_off", "var", "count", "split", "value"):
        assert np.array_equal(getattr(ta, f), getattr(tb, f)), f


def test_export_of_the_last_batch_survives_the_image(oracle):
    c = make_case("subset_rule")
    a = _sampler(c, oracle)
    for it in range(5):
        a.step(it < 3)
    b = _sampler(c, oracle)
    b.restore(a.checkpoint())
    ta, tb = a.export_trees(0), b.export_trees(0)
    for f in ("tree_id", "node_off", "var", "left", "right", "count", "split", "value", "rule"):
        assert np.array_equal(getattr(ta, f), getattr(tb, f)), f


def test_damaged_or_foreign_images_are_refused_with_a_message(oracle):
    c = make_case("ragged_1025")
    a = _sampler(c, oracle)
    for it in range(4):
        a.step(True)
    blob = a.checkpoint()
    b = _sampler(c, oracle)

    def refused(bad, text):
        with pytest.raises(_abi.PGBError, match=text):
            b.restore(bytes(bad))

    refused(blob[:100], "truncated")
    refused(blob[:-8], "truncated")
    refused(b"XXXXXXXX" + blob[8:], "not a pgbart checkpoint")
    bad = bytearray(blob)
    bad[8] = 99  # version
    refused(bad, "layout version")
    other = _sampler(c, oracle, seed=1)  # another chain of the same model: settings differ in the seed
    with pytest.raises(_abi.PGBError, match="settings differ"):
        other.restore(blob)
    img = ChainImage.parse(blob)
    off = img.node_off.ctypes.data - np.frombuffer(blob, np.uint8).ctypes.data
    bad = bytearray(blob)
    bad[off + 4: off + 8] = (10_000).to_bytes(4, "little")  # node_off[1]
    refused(bad, "inconsistent")
    off = img.var.ctypes.data - np.frombuffer(blob, np.uint8).ctypes.data
    bad = bytearray(blob)
    bad[off: off + 4] = (77).to_bytes(4, "little")  # a split on a column X does not have
    refused(bad, "inconsistent")
    # the sampler that refused all of these is untouched: it still loads the good image and continues the chain
    b.restore(blob)
    sa, _ = a.step(False)
    sb, _ = b.step(False)
    assert np.array_equal(sa, sb)
    for name in EDIT_CASES:  # the same of records that are whole but could not have been written by any backend
        _edited_images_are_refused(oracle, name)


def end_of_run_image(name, oracle, steps=None):
    c = make_case(name)
    if steps is not None:
        c["steps"] = steps
    return c, run_case(c, oracle, record_every=10 ** 6)["sampler"].checkpoint()


def _fresh(c, blob, backend):
    """A new sampler with the image's own settings (alpha / beta of the case included)."""
    p = c["X"].shape[1]
    st = PyBartSettings.from_data(c["X"], c.get("bart_Y", c["Y"]), m=c["m"], num_particles=c["P"], seed=c["seed"],
                                  batch=c["batch"], alpha=c.get("alpha", 0.95), beta=c.get("beta", 2.0),
                                  family=c.get("family", "normal"), n_outputs=c.get("K", 1),
                                  response=c.get("response", "constant"), compat=c.get("compat", 0))
    assert bytes(st.as_c()) == bytes(ChainImage.parse(blob).header.s)
    return PySampler(st, c["X"], c["Y"], np.zeros(p, np.int32) if c["rules"] is None else c["rules"],
                     np.ones(p) if c["prior"] is None else c["prior"], backend=backend)


def _edited_images_are_refused(oracle, name):
    """The table of tests/_image_edits.py on the end-of-run image of one case: every single-field edit a writer never
    produces is refused by pgb_image_check with its own "checkpoint is inconsistent (...)" text; the sampler that
    refused them all still loads the good image and continues the chain."""
    c, blob = end_of_run_image(name, oracle)
    b = _sampler(c, oracle)
    edits, skipped = image_edits(blob)
    assert len(edits) >= 34 and {w for w, _ in skipped} <= {"an orphan row with a label no leaf has",
                                                           "a node with two parents, another with none"}, skipped
    if name == "nan_onehot_prior":
        assert not skipped, skipped  # (this image has orphan rows: every edit of the table applies)
    for what, bad, text in edits:
        with pytest.raises(_abi.PGBError, match=r"checkpoint is inconsistent \(.*(" + text + ")"):
            b.restore(bad)
            pytest.fail(f"{name}: accepted: {what}")
    a = _sampler(c, oracle)
    a.restore(blob)
    b.restore(blob)
    for tune in (True, False):
        sa, va = a.step(tune)
        sb, vb = b.step(tune)
        assert np.array_equal(sa, sb) and np.array_equal(va, vb)
    assert a.checkpoint() == b.checkpoint()


@pytest.mark.parametrize("name", CASES)
def test_no_image_a_writer_produces_is_refused(oracle, name):
    """The condition on every check of pgb_image_check: the end-of-run image of every parity case loads (NaN rows,
    empty leaves of the upstream-semantics switches, stumps that won every update, K-vector and linear leaves)."""
    c, blob = end_of_run_image(name, oracle)
    _fresh(c, blob, oracle).restore(blob)


def test_binding_refuses_a_library_of_another_abi_revision(tmp_path):
    """pymc_bart_amd/_abi.py checks pgb_abi_version() (include/pgbart.h: PGB_ABI_VERSION) before binding anything."""
    import subprocess

    src = tmp_path / "stale.c"
    src.write_text("int pgb_abi_version(void) { return 5; }\nconst char* pgb_backend_name(void) { return \"hip-gfx950\"; }\n")
    so = tmp_path / "libstale.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    with pytest.raises(_abi.PGBError, match="revision 5"):
        _abi.PGBLibrary(str(so))
    src.write_text("int pgb_create(void) { return 0; }\n")
    so2 = tmp_path / "libolder.so"  # (another name: the loader caches by path)
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so2)])
    with pytest.raises(_abi.PGBError, match="no pgb_abi_version"):
        _abi.PGBLibrary(str(so2))


def test_the_forest_of_an_image_predicts_like_the_sampler_it_came_from(oracle):
    """`ChainImage.forest()` = `export_trees(1)` of the chain: a checkpoint can be predicted from without a sampler,
    and its in-sample prediction is the image's own sum_trees (one-hot / subset splits included: the caller names the
    columns' rules, the image holds trees)."""
    from pymc_bart_amd.trees import PosteriorSampler

    c = make_case("subset_rule")
    s = _sampler(c, oracle)
    for it in range(8):
        s.step(it < 4)
    img = ChainImage.parse(s.checkpoint())
    f_img, f_smp = img.forest(rules=c["rules"]), s.export_trees(1)
    for name in ("tree_id", "node_off", "var", "left", "right", "count", "split", "value", "rule"):
        assert np.array_equal(getattr(f_img, name), getattr(f_smp, name)), name
    m = c["m"]
    ps = PosteriorSampler(f_img, np.arange(m, dtype=np.int32)[None, :], m, 1, backend=oracle)
    # rows without a missing value in a split column predict exactly what the chain holds for them
    X = c["X"]
    ok = ~np.isnan(X).any(axis=1)
    pred = ps.sample_posterior(X[ok], [0])[0, 0]
    np.testing.assert_allclose(pred, img.sum_trees[0][ok], rtol=0, atol=1e-9)


FUZZ_IMAGES = [("normal/linear", {"rules": "mixed"}, 11), ("categorical:3/mix", {"rules": "mixed"}, 12),
               ("poisson_log", {}, 13), ("normal_meanscale:2", {}, 14)]


def test_loader_safety_under_the_sanitizers(oracle, tmp_path):
    """tests/image_fuzz_main.c: the oracle and pgb_image_check compiled with AddressSanitizer and UBSan into a
    stand-alone program; 2 000 seeded random edits (single bytes, whole fields, truncations) of each of four images
    go to pgb_checkpoint_load, and whatever is accepted is stepped, exported and saved.  Passes when nothing is
    reported; the number of accepted edits is printed (most single-bit changes of a number are another valid chain)."""
    import os
    import subprocess

    from _cases import make_history_case, moving_inputs, run_schedule

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "image_fuzz"
    subprocess.check_call(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover", "-std=gnu11",
                           "-ffp-contract=off", "-DPGB_MAX_PARTICLES=128", "-w", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "image_fuzz_main.c"), "-o", str(exe), "-lm"])
    total = 0
    for i, (kind, kw, seed) in enumerate(FUZZ_IMAGES):
        c = make_history_case(kind, n=257, **kw)  # (small: most accepted edits are stepped under the sanitizers)
        sched = moving_inputs(c)
        s = run_schedule(c, sched, oracle)["sampler"]
        off = sched(c["steps"] - 1).get("offset")
        rules = np.zeros(8 * ((c["X"].shape[1] * 4 + 7) // 8) // 4, np.int32)
        rules[: c["X"].shape[1]] = c["rules"]
        st = bytes(s.settings.as_c())
        case = tmp_path / f"case{i}.bin"
        case.write_bytes(b"".join([np.int64(len(st)).tobytes(), st, np.ascontiguousarray(c["X"], np.float64).tobytes(),
                                   np.asarray(s.backend.mem.to_host(s._y), np.float64).tobytes(), rules.tobytes(),
                                   np.ascontiguousarray(c["prior"], np.float64).tobytes(),
                                   np.int64(off is not None).tobytes(),
                                   b"" if off is None else np.ascontiguousarray(off, np.float64).tobytes()]))
        image = tmp_path / f"image{i}.bin"
        image.write_bytes(s.checkpoint())
        r = subprocess.run([str(exe), str(case), str(image), "2000", str(seed)], capture_output=True, text=True,
                           env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
        print(f"{kind}: {r.stdout.strip()}")
        assert r.returncode == 0 and r.stderr == "", f"{kind}:\n{r.stdout}\n{r.stderr[-4000:]}"
        words = r.stdout.split()
        assert words[0] == "edits" and words[1] == "2000" and words[4] == "failed_after_accept" and words[5] == "0"
        total += int(words[3])
    assert 0 < total < 4 * 2000  # some edits are other valid chains, some are refused
    print(f"accepted edits: {total} of {4 * 2000}")
