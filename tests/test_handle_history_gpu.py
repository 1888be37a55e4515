"""A handle's history leaves no trace -- GPU half.

Every parity test elsewhere feeds a handle once and steps it; under PyMC the step method calls set_response /
set_offset / set_likelihood before EVERY astep.  Here the inputs move at every astep (tests/_cases.py:
moving_inputs) and
  (1) the HIP library equals the oracle on every step's outputs and on the final image,
  (2) at every cut a fresh HIP handle -- built with the inputs in force there, then restore(image) -- continues
      bit for bit to the end and ends with the same image bytes,
  (3) a step with set_offset(None) and a step with an all-zero offset can be exchanged without a trace
      (has_off 1 -> 0 -> 1 against adding 0.0).
Likewise for pgb_set_data called again, a refused call, and ldx > p.  Every comparison is exact.  The oracle's own
setters are pinned in tests/test_handle_history.py."""
import ctypes as C

import numpy as np
import pytest

from _cases import (apply_inputs, assert_same_run, check_schedule, history_sampler, make_history_case, moving_inputs,
                    run_schedule)
from pymc_bart_amd import _abi
from pymc_bart_amd.image import ChainImage
from test_handle_history import (CUTS, IDS, SCHEDULES, SEQ_NAMES, padded_matrix_chain, refused_set_data_leaves_no_data,
                                 run_set_data_sequence, set_data_sequences)

pytestmark = pytest.mark.gpu


def _both(c, hip, oracle, cuts=CUTS):
    sched = moving_inputs(c)
    full = check_schedule(c, sched, hip, cuts, reference=run_schedule(c, sched, oracle))
    assert full["sampler"].backend.lib.backend_name == "hip-gfx950"
    if c["family"] != "normal":
        assert_same_run(run_schedule(c, moving_inputs(c, swap=True), hip), full, f"{c['name']}: None <-> zeros")
    return full


@pytest.mark.parametrize("kind,kw", SCHEDULES, ids=IDS)
def test_moving_inputs_leave_no_trace(hip, oracle, kind, kw):
    _both(make_history_case(kind, **kw), hip, oracle)


@pytest.mark.parametrize("kind", ["normal", "bernoulli_probit", "categorical:3"])
def test_moving_inputs_with_order_keys(hip, oracle, monkeypatch, kind):
    """The F32 row pass and k_ctrl<KEYS> (forced on at test size), n = 2049: three chunks, one row in the last."""
    monkeypatch.setenv("PGB_X32_MIN_MB", "0")
    _both(make_history_case(kind, n=2049), hip, oracle, cuts=(5, 9))


@pytest.mark.parametrize("kind", ["bernoulli_probit", "categorical:4"])
def test_moving_inputs_with_two_particles_per_lane(hip, oracle, kind):
    """100 particles: libpgbart_hip_p128.so."""
    full = _both(make_history_case(kind, P=100), hip, oracle, cuts=(5, 9))
    assert full["sampler"].backend.lib.max_particles == 128


@pytest.mark.parametrize("kind", ["categorical:3", "categorical:5"])
def test_moving_inputs_in_the_unfactorised_softmax(hip, oracle, kind):
    """The test builds of both backends with PGB_CAT_DMAX tiny (build/variants/): every child of a softmax split is a
    "slow" one, so the likelihood pass takes its unfactorised fallback -- which adds the offset at a site of its own."""
    import os

    import __graft_entry__ as g
    from _oracle import NumpyMemory
    from pymc_bart_amd import _abi
    from pymc_bart_amd.sampler import Backend

    if not (os.path.exists(g.HIP_SO_CATSLOW) and os.path.exists(g.ORACLE_SO_CATSLOW)):
        pytest.skip("the PGB_CAT_DMAX test builds are missing (python -c 'import __graft_entry__ as g; g.build()')")
    hip_slow = Backend(lib=_abi.PGBLibrary(g.HIP_SO_CATSLOW), mem=hip.mem)
    orc_slow = Backend(lib=_abi.PGBLibrary(g.ORACLE_SO_CATSLOW), mem=NumpyMemory())
    assert hip_slow.lib.backend_name == "hip-gfx950" and orc_slow.lib.backend_name == "oracle-cpu"
    _both(make_history_case(kind), hip_slow, orc_slow, cuts=(5, 9))


# ------------------------------------------------------------------ compiled family: aux, code object, params, offset
CENSORED = "double z = (y - mu) / s;  return aux > 0.5 ? log_ndtr(-z) : -0.5 * z * z - log(s);"


def test_compiled_family_with_moving_aux_code_params_and_offset(hip, oracle, tmp_path_factory, monkeypatch):
    """The censored-Normal body of tests/test_compiled_family_gpu.py.  Through the run: the aux column is replaced by
    another one (pgb_set_loglik_aux), cleared, set again; the code object is replaced by a rebuild of the same body
    (pgb_set_loglik_code: "a new code object replaces the old one"); s and the offset move at every astep.  The
    oracle runs the body's host build as its callback family."""
    from pymc_bart_amd.compiled import CompiledLikelihood, compile_loglik

    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit"))
    c = make_history_case("normal")
    n = c["X"].shape[0]
    rng = np.random.default_rng(12)
    cens_time = rng.uniform(-1.0, 2.5, n)
    aux_a = (c["Y"] > cens_time).astype(float)
    aux_b = (c["Y"] > cens_time - 0.7).astype(float)
    c["Y"] = np.where(aux_a > 0, cens_time, c["Y"])
    c.update(family="compiled", name="history/compiled", lik=lambda r: [float(r.uniform(0.3, 0.6))])
    lik = CompiledLikelihood(CENSORED, params={"s": "sigma"}, aux=aux_a)
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.mktemp("jit_rebuild")))
    rebuilt = compile_loglik(CENSORED, ["s"], max_particles=64)
    assert not rebuilt.cached
    aux_at = {0: aux_a, 3: aux_b, 5: None, 7: aux_a, 10: aux_b}
    code_at = {4: rebuilt.code, 8: lik.compiled(64).code}

    def set_aux(s, aux):
        s._hist_aux = None if aux is None else np.ascontiguousarray(aux, np.float64)  # (kept alive with the sampler)
        if s.backend.lib.backend_name == "hip-gfx950":
            _, f = s.backend.lib.compiled_entry_points()
            dev = None if aux is None else s.backend.mem.from_host(s._hist_aux)
            s.backend.lib.check(f(s._h, None if dev is None else s.backend.mem.ptr(dev)), "pgb_set_loglik_aux")
        else:
            s._cl_ctx.aux = None if aux is None else s._hist_aux.ctypes.data

    def set_code(s, code):
        if s.backend.lib.backend_name == "hip-gfx950":
            f, _ = s.backend.lib.compiled_entry_points()
            s._hist_code = C.create_string_buffer(code, len(code))
            s.backend.lib.check(f(s._h, C.cast(s._hist_code, C.c_void_p), len(code), 1), "pgb_set_loglik_code")

    def setup(s, in_force):
        s.set_compiled_likelihood(lik)
        if "aux" in in_force:
            set_aux(s, in_force["aux"])
        if "code" in in_force:
            set_code(s, in_force["code"])

    def apply(s, inp):
        if "aux" in inp:
            set_aux(s, inp["aux"])
        if "code" in inp:
            set_code(s, inp["code"])

    c.update(setup=setup, apply=apply)
    base = moving_inputs(c)

    def sched(it):
        inp = base(it)
        if it in aux_at:
            inp["aux"] = aux_at[it]
        if it in code_at:
            inp["code"] = code_at[it]
        return inp

    # (a CPU backend runs the body as family "callback": the two images carry another family code in their settings,
    #  and nothing else of the settings may differ)
    ref = run_schedule(c, sched, oracle)
    full = check_schedule(c, sched, hip, (4, 6, 9), reference=ref, ignore=("settings",))
    assert full["sampler"].backend.lib.backend_name == "hip-gfx950"
    sg, so = full["sampler"].settings.as_c(), ref["sampler"].settings.as_c()
    assert sg.family == _abi.FAMILIES["compiled"] and bytes(sg) == bytes(so)  # (one PyBartSettings on both sides)
    ig, io = ChainImage.parse(full["end"]["image"]).header.s, ChainImage.parse(ref["end"]["image"]).header.s
    assert ig.family == _abi.FAMILIES["compiled"] and io.family == _abi.FAMILIES["callback"]
    io.family = ig.family
    assert bytes(ig) == bytes(io)
    # the aux column matters: the chain that kept the first column is another chain
    kept = run_schedule(c, lambda it: {k: v for k, v in sched(it).items() if k != "aux" or it == 0}, hip)
    assert kept["steps"][2] == full["steps"][2] and kept["steps"][-1]["sum_trees"] != full["steps"][-1]["sum_trees"]


# ------------------------------------------------------------------ pgb_set_data again
# (sequences a, b, c exercise the launch selection that pgb_set_data's `use_keys` flag decides: the KEYS instance of
#  k_ctrl and the F32 instance of the row pass are chosen together, for the data of the last call)
@pytest.mark.parametrize("seq", SEQ_NAMES)
@pytest.mark.parametrize("kind", ["normal", "categorical:3"])
def test_set_data_again_leaves_no_trace(hip, oracle, monkeypatch, kind, seq):
    c, seqs = set_data_sequences(kind)
    got = run_set_data_sequence(c, seqs[seq], hip, monkeypatch)
    want = run_set_data_sequence(c, seqs[seq][-1:], oracle, monkeypatch)
    assert_same_run(got, want, f"{kind} {seq}: HIP against the oracle")


def test_a_refused_set_data_leaves_the_handle_without_data(hip, monkeypatch):
    c, seqs = set_data_sequences("normal")
    s = refused_set_data_leaves_no_data(c, seqs["d_refused_then_good"][1], hip, monkeypatch)
    assert s.backend.lib.backend_name == "hip-gfx950"


@pytest.mark.parametrize("kind,kw", [("normal", {}), ("bernoulli_probit/linear", {"rules": "mixed"})], ids=["normal", "probit-linear-mixed"])
def test_a_padded_matrix_is_the_same_data(hip, oracle, kind, kw):
    """ldx = p + 3 with NaN and 1e300 in the pad columns: the chain, col_nan behaviour (X[:, 1] has missing values)
    and the column exponents of the linear leaves included, is the ldx = p chain -- and the oracle's."""
    c = make_history_case(kind, **kw)
    wide = padded_matrix_chain(c, hip, 3)
    assert_same_run(wide, padded_matrix_chain(c, hip, 0), f"{kind}: ldx = p + 3 against ldx = p")
    assert_same_run(wide, padded_matrix_chain(c, oracle, 3), f"{kind}: ldx = p + 3, HIP against the oracle")
