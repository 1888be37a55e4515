"""Family "compiled" on the MI355X: the body's code object runs inside the HIP library's own likelihood pass
(``pgb_set_loglik_code``), device-resident.  It must be the SAME sampler as the built-in family it spells out, and
the same as a CPU backend running the body's host build -- bit for bit."""
import json
import os

import numpy as np
import pytest

from _cases import digest, make_case, run_case
from pymc_bart_amd import _abi
from pymc_bart_amd.compiled import CompiledLikelihood, compile_loglik
from pymc_bart_amd.sampler import PyBartSettings, PySampler

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_runs.json")))
CHECK_LOSS = "double u = (y - mu) / b;  return -(u * (u < 0.0 ? q - 1.0 : q));"
CENSORED = "double z = (y - mu) / s;  return aux > 0.5 ? log_ndtr(-z) : -0.5 * z * z - log(s);"


@pytest.fixture(autouse=True)
def _jit_cache(tmp_path_factory, monkeypatch):
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit"))


def _with_compiled(lik):
    """Patch PySampler so that run_case's samplers take the compiled likelihood."""
    orig = PySampler.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        if self.settings.family == "compiled":
            self.set_compiled_likelihood(lik)

    return orig, init


def _run(c, backend, lik, **kw):
    orig, init = _with_compiled(lik)
    PySampler.__init__ = init
    try:
        return run_case(c, backend, **kw)
    finally:
        PySampler.__init__ = orig


def test_check_loss_on_hip_reproduces_the_builtin_fingerprint(hip):
    c = dict(make_case("quantile_asymlaplace"))
    c["family"] = "compiled"
    lik = CompiledLikelihood(CHECK_LOSS, params={"b": 0.25, "q": 0.9})
    res = _run(c, hip, lik)
    assert res["sampler"].backend.lib.backend_name == "hip-gfx950"
    assert digest(res) == GOLD["quantile_asymlaplace"]


def _cfg2_quantile(seed=3415, n=100_000, p=50):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (n, p))
    f = 10 * np.sin(np.pi * X[:, 0] * X[:, 1]) + 20 * (X[:, 2] - 0.5) ** 2 + 10 * X[:, 3] + 5 * X[:, 4]
    Y = f + rng.normal(0, 1.0 + X[:, 0], n)
    return X, Y


def _chain(X, Y, family, backend, lik=None, params=(), m=200, P=40, tune=10, draws=10, offset=None, aux_moves=None,
           seed=7, checkpoint_at=None):
    st = PyBartSettings.from_data(X, Y, m=m, num_particles=P, seed=seed, family=family)
    p = X.shape[1]
    s = PySampler(st, X, Y, np.zeros(p, np.int32), np.ones(p), backend=backend)
    if lik is not None:
        s.set_compiled_likelihood(lik)
    if offset is not None:
        s.set_offset(offset)
    out = []
    for it in range(tune + draws):
        if checkpoint_at is not None and it == checkpoint_at:
            blob = s.checkpoint()
            s = PySampler(st, X, Y, np.zeros(p, np.int32), np.ones(p), backend=backend)
            if lik is not None:
                s.set_compiled_likelihood(lik)
            if offset is not None:
                s.set_offset(offset)
            s.restore(blob)
        s.set_likelihood(aux_moves(it) if aux_moves is not None else list(params))
        st_, vi = s.step(it < tune)
        ta = s.export_trees(0)
        out.append((st_.copy(), vi.copy(), np.concatenate([ta.var, ta.left, ta.right, ta.count,
                                                           ta.split.view(np.int64), ta.value.ravel().view(np.int64)])))
    return out, s


def test_compiled_check_loss_equals_the_builtin_at_cfg2_size(hip):
    X, Y = _cfg2_quantile()
    lik = CompiledLikelihood(CHECK_LOSS, params={"b": 0.25, "q": 0.9})
    a, _ = _chain(X, Y, "asymmetric_laplace", hip, params=[0.25, 0.9])
    b, s = _chain(X, Y, "compiled", hip, lik=lik, params=[0.25, 0.9])
    assert s._cl_build.resources["scratch_bytes"] == 0
    for (sa, va, ta), (sb, vb, tb) in zip(a, b):
        assert np.array_equal(sa, sb) and np.array_equal(va, vb) and np.array_equal(ta, tb)


def _censored_data(n=100_000, p=20, seed=11):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (n, p))
    f = np.sin(2 * X[:, 0]) + 0.7 * X[:, 1]
    t = f + 0.4 * rng.standard_normal(n)
    c = rng.uniform(-1.0, 2.0, n)                    # right-censoring times
    cens = (t > c).astype(float)
    Y = np.where(cens > 0, c, t)
    off = 0.1 * np.round(X[:, 2] * 8) / 8            # an offset of the linear predictor
    return X, Y, cens, off


@pytest.mark.parametrize("P", [40, 100])
def test_censored_normal_on_hip_equals_the_oracle_running_the_host_build(hip, oracle, P):
    """A model outside the closed family: aux column, exp / log / log_ndtr, an offset, s moving every astep;
    P = 100 runs through libpgbart_hip_p128.so and its own code object."""
    X, Y, cens, off = _censored_data()
    lik = CompiledLikelihood(CENSORED, params={"s": "sigma"}, aux=cens)
    sig = np.random.default_rng(5).uniform(0.3, 0.6, 20)
    moves = lambda it: [float(sig[it])]  # noqa: E731
    a, sa = _chain(X, Y, "compiled", hip, lik=lik, m=50, P=P, tune=10, draws=10, offset=off, aux_moves=moves)
    b, sb = _chain(X, Y, "compiled", oracle, lik=lik, m=50, P=P, tune=10, draws=10, offset=off, aux_moves=moves)
    assert sa.backend.lib.backend_name == "hip-gfx950" and sa.backend.lib.max_particles == (128 if P > 64 else 64)
    assert sb.backend.lib.backend_name != "hip-gfx950"
    for (x1, v1, t1), (x2, v2, t2) in zip(a, b):
        assert np.array_equal(x1, x2) and np.array_equal(v1, v2) and np.array_equal(t1, t2)
    ca, cb = sa.counters.as_dict(), sb.counters.as_dict()
    for k in ("particle_steps", "tree_updates", "rows_touched", "rounds", "saturations"):
        assert ca[k] == cb[k], k


def test_refused_code_objects_are_never_launched_and_the_handle_stays_usable(hip, oracle):
    X, Y, cens, off = _censored_data(n=4000, p=4)
    lik = CompiledLikelihood(CENSORED, params={"s": 0.5}, aux=cens)
    st = PyBartSettings.from_data(X, Y, m=8, num_particles=10, seed=3, family="compiled")
    s = PySampler(st, X, Y, np.zeros(4, np.int32), np.ones(4), backend=hip)
    set_code, _ = s.backend.lib.compiled_entry_points()
    with pytest.raises(_abi.PGBError, match="pgb_set_loglik_code first"):
        s.step(True)
    wrong = compile_loglik(CENSORED, ["s"], max_particles=128).code      # the other particle build
    garbage = bytes(np.random.default_rng(1).integers(0, 256, 4096, dtype=np.uint8))
    for blob, msg in ((wrong, "particle build"), (garbage, "not a gfx950 code object")):
        rc = set_code(s._h, blob, len(blob), 1)
        assert rc == -1, rc                                               # PGB_E_INVALID
        assert msg in s.backend.lib.lib.pgb_last_error().decode()
    with pytest.raises(_abi.PGBError, match="pgb_set_loglik_code first"):
        s.step(True)                                                      # nothing was installed
    s.set_compiled_likelihood(lik)
    twin = PySampler(st, X, Y, np.zeros(4, np.int32), np.ones(4), backend=oracle)
    twin.set_compiled_likelihood(lik)
    for it in range(6):
        for q in (s, twin):
            q.set_likelihood([0.5])
        a, _ = s.step(it < 3)
        b, _ = twin.step(it < 3)
        assert np.array_equal(a, b)


def test_checkpoint_round_trip_and_two_chains_on_one_gpu(hip):
    X, Y, cens, off = _censored_data(n=20_000, p=6)
    lik = CompiledLikelihood(CENSORED, params={"s": "sigma"}, aux=cens)
    moves = lambda it: [0.4 + 0.01 * it]  # noqa: E731
    a, _ = _chain(X, Y, "compiled", hip, lik=lik, m=20, P=20, tune=5, draws=5, aux_moves=moves)
    b, _ = _chain(X, Y, "compiled", hip, lik=lik, m=20, P=20, tune=5, draws=5, aux_moves=moves, checkpoint_at=4)
    for (x1, v1, t1), (x2, v2, t2) in zip(a, b):
        assert np.array_equal(x1, x2) and np.array_equal(v1, v2) and np.array_equal(t1, t2)

    from pymc_bart_amd.chains import sample_chains
    from pymc_bart_amd.pgbart import BARTOp

    op = BARTOp(X, Y, m=20)
    res = sample_chains(op, chains=2, tune=4, draws=4, num_particles=20, random_seed=3, sigma=0.5,
                        likelihood=lik, keep_draws=True)
    assert len(res) == 2
    mods = set()
    for r in res:
        smp = r["step"].sampler
        assert smp.backend.lib.backend_name == "hip-gfx950" and smp.settings.family == "compiled"
        assert np.all(np.isfinite(r["mu"]))
        mods.add(id(smp._cl_code))
    assert len(mods) == 2                                                 # one module per handle
    assert not np.array_equal(res[0]["mu"], res[1]["mu"])                 # independent chains
