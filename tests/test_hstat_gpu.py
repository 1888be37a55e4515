"""Friedman's H-statistic on the MI355X: ``pgb_hstat_background``, ``pgb_hstat_rows`` and ``pgb_hstat_finish``
(``k_hstat_bg``, ``k_hstat_moments``, ``k_hstat_rows``) against the host reference of ``tests/_hstat_host.py`` -- the
header the kernels compile, built for the host, with the walk's sums by the oracle's ``pgb_predict`` -- bit for bit: every
word of the workspace (the moments, ``B0`` and ``B1``, the row partials), the per-row ``J``, ``T`` and ``I`` and the
outputs, over the row counts, list lengths, widths, outputs, leaf kinds, split rules and NaN / infinity patterns at which
the kernels take another path; every refusal; then ``friedman_h`` end to end on a two-chain fit.

Everything is ``np.array_equal`` on the bits; the end-to-end fit adds two ordering conditions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _hstat_host as host
import _ice_host as ice_host
import _permimp_host as permimp
from pymc_bart_amd import BARTOp, _abi, friedman_h
from pymc_bart_amd import hstat as hstat_mod
from pymc_bart_amd.chains import attach_history, sample_chain
from pymc_bart_amd.sampler import Backend
from pymc_bart_amd.utils import _get_posterior_sampler

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAXP = int(re.search(r"#define PRED_LDS_MAXP (\d+)", open(os.path.join(ROOT, "pymc_bart_amd", "csrc", "pgb_pred_walk.h")).read()).group(1))
ONEHOT, SUBSET = _abi.RULE_ONEHOT, _abi.RULE_SUBSET
GUARD = -7.75e300    # every buffer before a call and behind it after: no refused call may touch it
POISON = 7.0e77      # the padding of ldx > p: no result may show it
E_INVALID = -1


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


class Device:
    """One whole call on the device, block by block, with guards behind every buffer."""

    def __init__(self, hip, jobs: host.Jobs, pad=3):
        self.hip, self.jobs, self.pad = hip, jobs, pad
        self.ws_bytes_, self.background_, self.rows_, self.finish_ = hip.lib.hstat_entry_points()
        j = jobs
        self.history = (C.byref(j.carr), j.fidx.ctypes.data, j.fidx.shape[0], j.fidx.shape[1])
        self.job_args = (j.cols.ctypes.data, j.q, j.pairs.ctypes.data if j.n_pairs else None, j.n_pairs, j.picks.ctypes.data,
                         j.n_picks)
        got = C.c_int64(-1)
        self.n_common = np.full((j.n_picks, j.n_pairs), -1, np.int32)
        rc = self.ws_bytes_(*self.history, j.p, *self.job_args, C.byref(got), self.n_common.ctypes.data if j.n_pairs else None)
        hip.lib.check(rc, "pgb_hstat_workspace_bytes")
        self.words = got.value // 8
        self.ws = hip.mem.from_host(np.full(self.words + 64, GUARD))
        self.J, self.T, self.I = [], [], []  # noqa: E741

    def _wide(self, X):
        wide = np.full((X.shape[0], X.shape[1] + self.pad), POISON)
        wide[:, :X.shape[1]] = X
        return self.hip.mem.from_host(wide)

    def background(self, X, v, r0=0, init=True, change=None):
        mem = self.hip.mem
        xd, vd = self._wide(X), mem.from_host(np.ascontiguousarray(v))
        a = dict(X=mem.ptr(xd), nb=X.shape[0], p=X.shape[1], ldx=X.shape[1] + self.pad, w=mem.ptr(vd), r0=r0, ws=mem.ptr(self.ws))
        a.update(change or {})
        return self.background_(*self.history, a["X"], a["nb"], a["p"], a["ldx"], a["w"], a["r0"], int(init), *self.job_args, a["ws"],
                                mem.stream_ptr)

    def rows(self, X, w, r0=0, init=True, change=None, per_row=True):
        mem, j = self.hip.mem, self.jobs
        nb = X.shape[0]
        xd, wd = self._wide(X), mem.from_host(np.ascontiguousarray(w))
        nc, npr = j.n_picks * j.q * j.K * nb, j.n_picks * j.n_pairs * j.K * nb
        jd, td, idv = (mem.from_host(np.full(n + 64, GUARD)) for n in (nc, nc, npr))
        a = dict(X=mem.ptr(xd), nb=nb, p=X.shape[1], ldx=X.shape[1] + self.pad, w=mem.ptr(wd), r0=r0, ws=mem.ptr(self.ws),
                 jscr=mem.ptr(jd), job_args=self.job_args, history=self.history)
        a.update(change or {})
        rc = self.rows_(*a["history"], a["X"], a["nb"], a["p"], a["ldx"], a["w"], a["r0"], int(init), *a["job_args"], a["ws"],
                        a["jscr"], mem.ptr(td) if per_row else None, mem.ptr(idv) if per_row and j.n_pairs else None, mem.stream_ptr)
        got = [mem.to_host(b) for b in (jd, td, idv)]
        self.last = got
        if rc == 0:
            assert all(np.all(g[n:] == GUARD) for g, n in zip(got, (nc, nc, npr)))
            self.J.append(got[0][:nc].reshape(j.n_picks, j.q, j.K, nb))
            self.T.append(got[1][:nc].reshape(j.n_picks, j.q, j.K, nb))
            self.I.append(got[2][:npr].reshape(j.n_picks, j.n_pairs, j.K, nb))
        return rc

    def workspace(self):
        got = self.hip.mem.to_host(self.ws)
        assert np.all(got[self.words:] == GUARD)
        return got[:self.words]

    def finish(self, var_fit):
        j = self.jobs
        var_fit = np.ascontiguousarray(var_fit, np.float64).reshape(j.n_picks, j.K)
        out = {k: np.full((j.n_picks, j.q, j.K), GUARD) for k in ("main_var", "total_var", "h2_total")}
        out.update({k: np.full((j.n_picks, max(j.n_pairs, 1), j.K), GUARD) for k in ("inter_var", "h2")})
        bad = C.c_int64(-1)
        rc = self.finish_(self.hip.mem.ptr(self.ws), j.n_picks, j.q, j.n_pairs, j.K, var_fit.ctypes.data,
                          *(out[k].ctypes.data for k in ("main_var", "total_var", "h2_total", "inter_var", "h2")), C.byref(bad),
                          self.hip.mem.stream_ptr)
        self.hip.lib.check(rc, "pgb_hstat_finish")
        for k in ("inter_var", "h2"):
            out[k] = out[k][:, :j.n_pairs]
        out["n_nonfinite"] = int(bad.value)
        return out


def _check(hip, oracle, pool, table, cols, pairs, picks, Xb, v, Xe, w, cuts=(None, None), pad=3, var_fit=None):
    """The device against the host reference, bit for bit; the background is cut at ``cuts[0]`` and the evaluation rows at
    ``cuts[1]`` (a multiple of 64; ``None``: one block).  -> ``(the device's object, its outputs)``."""
    jobs = host.Jobs(pool, table, Xe.shape[1], cols, pairs, picks)
    ref, dev = host.Reference(oracle, jobs), Device(hip, jobs, pad)
    assert dev.words == ref.sizes["words"] and np.array_equal(dev.n_common, ref.n_common)
    for X, wt, cut, fr, fd in ((Xb, v, cuts[0], ref.background, dev.background), (Xe, w, cuts[1], ref.rows, dev.rows)):
        edges = [0, X.shape[0]] if cut is None or cut >= X.shape[0] else [0, cut, X.shape[0]]
        for r0, r1 in zip(edges[:-1], edges[1:]):
            fr(X[r0:r1], wt[r0:r1], r0, r0 == 0)
            hip.lib.check(fd(X[r0:r1], wt[r0:r1], r0, r0 == 0), "pgb_hstat_*")
    got, want = dev.workspace(), ref.ws
    assert np.array_equal(bits(got), bits(want)), (int((bits(got) != bits(want)).sum()), got.size, ref.sizes)
    for name in ("J", "T", "I"):
        a, b = np.concatenate(getattr(dev, name), axis=-1), getattr(ref, name)
        assert np.array_equal(bits(a), bits(b)), (name, int((bits(a) != bits(b)).sum()), a.size)
    var_fit = np.full((jobs.n_picks, jobs.K), 1.5) if var_fit is None else var_fit
    out, wout = dev.finish(var_fit), ref.finish(var_fit)
    for key in ("main_var", "total_var", "h2_total", "inter_var", "h2"):
        assert np.array_equal(bits(out[key]), bits(wout[key])), key
    assert out["n_nonfinite"] == wout["n_nonfinite"]
    return dev, out


def _rows(rng, n, p, rules=None, nan_rate=0.05):
    X = rng.normal(size=(n, p))
    for j, r in enumerate([] if rules is None else rules):
        if r == ONEHOT:
            X[:, j] = rng.integers(0, 4, n)
        elif r == SUBSET:
            X[:, j] = rng.integers(0, 8, n)
    X[rng.random((n, p)) < nan_rate] = np.nan
    return X


def _forests(rng, n_trees, m, D):
    return np.stack([rng.permutation(n_trees)[:m] for _ in range(D)]).astype(np.int32)


def _weights(rng, n):
    return rng.uniform(0.5, 2.0, n)


# ------------------------------------------------------------------ 1. row counts, list lengths, picks
@pytest.fixture(scope="module")
def lengths():
    """Use lists of 1, 3, 4, 8, 9 and 0 trees (``_permimp_host.lengths_pool``): both sides of PRED_WALKS and of its
    prefetch for the walk's sum; common lists of 0, 1, 3, 4 and 8 trees; K = 1."""
    rng = np.random.default_rng(101)
    pool = permimp.lengths_pool(rng, 1)
    table = _forests(rng, 12, 12, 3)
    return pool, table, _rows(rng, 130, 6), _rows(rng, 130, 6), _weights(rng, 130), _weights(rng, 130)


PAIRS6 = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5), (4, 0)]        # common lists of 1, 3, 4, 8, 0, 0 and 1 trees


@pytest.mark.parametrize("n_b,n_e", [(1, 130), (63, 64), (64, 63), (65, 1), (130, 65)])
def test_row_counts_and_list_lengths(hip, oracle, lengths, n_b, n_e):
    pool, table, Xb, Xe, v, w = lengths
    dev, out = _check(hip, oracle, pool, table, list(range(6)), PAIRS6, [0, 2, 0], Xb[:n_b], v[:n_b], Xe[:n_e], w[:n_e])
    assert dev.n_common[0].tolist() == [1, 3, 4, 8, 0, 0, 1]
    for key in ("h2", "inter_var", "h2_total", "main_var"):
        assert np.array_equal(bits(out[key][0]), bits(out[key][2])), key  # the repeated pick
    assert np.all(bits(out["h2"][:, 4:6]) == 0) and np.all(bits(np.concatenate(dev.I, -1)[:, 4:6]) == 0)   # no common tree
    assert np.all(bits(out["main_var"][:, 5]) == 0)                     # the unused column
    if n_e > 1 and n_b > 1:
        assert np.all(out["h2"][:, :4] > 0.0)


def test_blocks_continue_where_the_last_one_ended(hip, oracle, lengths):
    pool, table, Xb, Xe, v, w = lengths
    _, cut = _check(hip, oracle, pool, table, [4, 0, 3], [(0, 1), (2, 0)], [1, 2], Xb, v, Xe, w, cuts=(64, 128), pad=0)
    _, one = _check(hip, oracle, pool, table, [4, 0, 3], [(0, 1), (2, 0)], [1, 2], Xb, v, Xe, w)
    for key in ("main_var", "total_var", "h2_total", "inter_var", "h2"):
        assert np.array_equal(bits(cut[key]), bits(one[key])), key


def test_clean_rows_take_the_fixed_length_walk_too_and_no_per_row_output_is_needed(hip, oracle, lengths):
    pool, table, Xb, Xe, v, w = lengths
    clean = np.nan_to_num(Xe, nan=0.25)
    dev, out = _check(hip, oracle, pool, table, [4, 0, 3, 5], [(0, 2), (1, 0)], [1], Xb, v, clean, w)
    jobs = dev.jobs
    quiet = Device(hip, jobs)
    hip.lib.check(quiet.background(Xb, v), "pgb_hstat_background")
    hip.lib.check(quiet.rows(clean, w, per_row=False), "pgb_hstat_rows")
    assert np.all(quiet.last[1] == GUARD) and np.all(quiet.last[2] == GUARD)      # nothing per-row leaves the kernel
    assert np.array_equal(bits(quiet.workspace()), bits(dev.workspace()))
    assert np.array_equal(bits(quiet.finish(np.full((1, 1), 1.5))["h2"]), bits(out["h2"]))


# ------------------------------------------------------------------ 2. widths, outputs, leaves, rules
@pytest.mark.parametrize("p,K,linear", [(3, 1, False), (3, 3, True), (LDS_MAXP, 1, True), (LDS_MAXP + 1, 3, True),
                                        (LDS_MAXP + 1, 1, False)])
def test_widths_outputs_and_leaf_kinds(hip, oracle, p, K, linear):
    """p = 126 is the widest tile staged in LDS, p = 127 the first width read from global memory; constant, linear and
    mixed leaves (a third of a linear pool's leaves stay constant); ``ldx > p`` with poison in the padding."""
    rng = np.random.default_rng(200 + p + K)
    pool = ice_host.random_pool(rng, 14, p, K=K, depth=4, linear=[0, 1, p - 1] if linear else None,
                                split_cols=[0, 1, 2, p - 1] if p > 3 else None)
    table = _forests(rng, 14, 8, 3)
    cols = [p - 1, 0, 1] if p == 3 else [p - 1, 0, 2, 1, 64]
    pairs = [(0, 1), (2, 1), (0, 2)] if p == 3 else [(0, 1), (2, 1), (3, 0), (4, 1)]
    dev, out = _check(hip, oracle, pool, table, cols, pairs, [2, 0], _rows(rng, 70, p), _weights(rng, 70), _rows(rng, 67, p),
                      _weights(rng, 67), cuts=(64, 64))
    assert dev.n_common.max() > 0 and np.any(out["h2"] > 0.0) and out["n_nonfinite"] == 0


@pytest.mark.parametrize("p,K", [(5, 1), (5, 3), (LDS_MAXP + 1, 1)])
def test_one_hot_and_subset_rules(hip, oracle, p, K):
    rng = np.random.default_rng(300 + p + K)
    rules = [0, ONEHOT, 0, SUBSET, 0] + [0] * (p - 5)
    pool = ice_host.random_pool(rng, 16, p, K=K, depth=4, rules=rules, linear=[2, 4], split_cols=[0, 1, 2, 3, 4])
    table = _forests(rng, 16, 8, 2)
    dev, out = _check(hip, oracle, pool, table, [1, 3, 0, 4], [(0, 1), (1, 2), (3, 0)], [0, 1], _rows(rng, 90, p, rules),
                      _weights(rng, 90), _rows(rng, 130, p, rules), _weights(rng, 130))
    assert dev.n_common.max() > 0 and np.any(out["h2"] > 0.0)


def test_the_128_particle_build(hip, oracle, lengths):
    pool, table, Xb, Xe, v, w = lengths
    big = Backend(lib=_abi.load_hip_library(128), mem=hip.mem)
    _check(big, oracle, pool, table, [1, 2, 4], [(0, 1), (2, 1)], [0, 1], Xb[:70], v[:70], Xe[:66], w[:66])


# ------------------------------------------------------------------ 3. NaN, the infinities, -0.0
def test_rows_of_all_nan_infinities_and_minus_zero_on_a_split_value(hip, oracle):
    rng = np.random.default_rng(41)
    import _predict_exact as ex

    roots = [ex.Split(0, 0.0, ex.Split(1, -0.0, ex.Leaf([1.0], 3), ex.Leaf([-2.0], 5), count=8), ex.Leaf([0.5], 7), count=15),
             ex.Split(1, 0.0, ex.Leaf([0.25], 2), ex.Split(0, np.inf, ex.Leaf([4.0], 6), ex.Leaf([-1.0], 1), count=7), count=9),
             ex.Split(2, -np.inf, ex.Leaf([3.0], 0), ex.Split(0, 1.0, ex.Leaf([1.5], 0), ex.Leaf([2.5], 0), count=0), count=0)]
    roots += [ex.dyadic_tree(rng, 1, 3, [0, 1, 2], lambda r, c: float(r.normal()), counts="free") for _ in range(5)]
    pool = ex.build_pool(roots, 1)
    table = np.array([[0, 1, 2, 3, 4, 5, 6, 7], [7, 2, 1, 0, 6, 5, 4, 3]], np.int32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0])
    Xe, Xb = rng.choice(special, size=(100, 3)), rng.choice(special, size=(80, 3))
    Xe[::9], Xb[::7] = np.nan, np.nan                                   # rows of all NaN
    dev, out = _check(hip, oracle, pool, table, [0, 1, 2], [(0, 1), (0, 2), (1, 2)], [0, 1], Xb, _weights(rng, 80), Xe,
                      _weights(rng, 100))
    assert np.all(np.isfinite(np.concatenate(dev.I, -1))) and np.all(dev.n_common[:, :2] > 0)


# ------------------------------------------------------------------ 4. refusals
def test_every_refusal_leaves_everything_untouched(hip, lengths):
    pool, table, Xb, Xe, v, w = lengths
    jobs = host.Jobs(pool, table, 6, [2, 0, 4], [(0, 1), (2, 0)], [0, 1])
    dev = Device(hip, jobs)
    i32 = lambda *a: np.array(a, np.int32)  # noqa: E731
    bad_cols, twice, bad_picks = i32(0, 9, 1), i32(2, 0, 2), i32(0, 3)
    same, out_of, again, many = i32(0, 1, 2, 2), i32(0, 1, 3, 0), i32(0, 1, 1, 0), np.zeros(2 * 4097, np.int32)
    lots = np.zeros(1 << 22, np.int32)
    table_bad = table.copy()
    table_bad[1, 3] = 12
    h, ja = dev.history, dev.job_args
    jobs_with = lambda **kw: tuple(kw.get(k, x) for k, x in zip(("cols", "q", "pairs", "n_pairs", "picks", "n_picks"), ja))  # noqa: E731
    cases = [
        (dict(X=None), "X_dev is null"), (dict(w=None), "w_dev is null"), (dict(ws=None), "ws_dev is null"),
        (dict(jscr=None), "jscr_dev is null"), (dict(nb=0), "nb must be >= 1"), (dict(ldx=5), "ldx must be >= p"),
        (dict(p=0), "n_forests, m and p must be >= 1"), (dict(r0=-64), "first_row = -64 must be a multiple of 64"),
        (dict(r0=32), "first_row = 32 must be a multiple of 64"),
        (dict(history=(None,) + h[1:]), "trees is null"), (dict(history=h[:1] + (None,) + h[2:]), "forest_tree_idx is null"),
        (dict(history=h[:2] + (0,) + h[3:]), "n_forests, m and p must be >= 1"), (dict(history=h[:3] + (0,)), "n_forests, m and p must be >= 1"),
        (dict(history=h[:1] + (table_bad.ctypes.data,) + h[2:]), "forest_tree_idx entry outside"),
        (dict(job_args=jobs_with(cols=None)), "cols_host is null"), (dict(job_args=jobs_with(q=0)), "q must be >= 1"),
        (dict(job_args=jobs_with(picks=None)), "picks_host is null"), (dict(job_args=jobs_with(n_picks=0)), "n_picks must be >= 1"),
        (dict(job_args=jobs_with(pairs=None)), "pairs_host is null"), (dict(job_args=jobs_with(n_pairs=-1)), "n_pairs must be >= 0"),
        (dict(job_args=jobs_with(cols=bad_cols.ctypes.data)), "cols_host[1] = 9 is outside [0, p = 6)"),
        (dict(job_args=jobs_with(cols=twice.ctypes.data)), "repeats cols_host"),
        (dict(job_args=jobs_with(picks=bad_picks.ctypes.data)), "picks_host[1] = 3 is outside [0, n_forests = 3)"),
        (dict(job_args=jobs_with(pairs=same.ctypes.data)), "pairs_host[1] names slot 2 twice"),
        (dict(job_args=jobs_with(pairs=out_of.ctypes.data)), "pairs_host[1] = (3, 0) names a slot outside [0, q = 3)"),
        (dict(job_args=jobs_with(pairs=again.ctypes.data)), "pairs_host[1] repeats pairs_host[0]"),
        (dict(job_args=jobs_with(pairs=many.ctypes.data, n_pairs=4097)), "at most PGB_HSTAT_MAX_PAIRS = 4096 pairs per call"),
        (dict(nb=(1 << 37) - 64, job_args=jobs_with(picks=lots.ctypes.data, n_picks=1 << 22)), "overflows a 64-bit size"),
    ]
    for change, msg in cases:
        rc = dev.rows(Xe, w, change=change)
        text = hip.lib.lib.pgb_last_error().decode()
        if "entry outside" not in msg:
            assert text.startswith("pgb_hstat_rows: "), (change, text)
        assert rc == E_INVALID and msg in text, (change, rc, text)
        assert all(np.all(g == GUARD) for g in dev.last) and np.all(hip.mem.to_host(dev.ws) == GUARD), change
    for change, msg in [(dict(X=None), "X_dev is null"), (dict(w=None), "v_dev is null"), (dict(ws=None), "ws_dev is null"),
                        (dict(nb=0), "nb must be >= 1"), (dict(ldx=5), "ldx must be >= p"), (dict(r0=1), "first_row = 1 must be")]:
        rc = dev.background(Xb, v, change=change)
        text = hip.lib.lib.pgb_last_error().decode()
        assert rc == E_INVALID and msg in text and text.startswith("pgb_hstat_background: "), (change, rc, text)
        assert np.all(hip.mem.to_host(dev.ws) == GUARD), change
    got = C.c_int64(-5)
    common = np.full((2, 2), -9, np.int32)
    rc = dev.ws_bytes_(*h, 6, *jobs_with(pairs=again.ctypes.data), C.byref(got), common.ctypes.data)
    assert rc == E_INVALID and got.value == -5 and np.all(common == -9)
    assert "pgb_hstat_workspace_bytes: pairs_host[1] repeats" in hip.lib.lib.pgb_last_error().decode()
    out = np.full(8, GUARD)
    rc = dev.finish_(hip.mem.ptr(dev.ws), 2, 3, 2, 0, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                     out.ctypes.data, out.ctypes.data, C.byref(got), hip.mem.stream_ptr)
    assert rc == E_INVALID and "pgb_hstat_finish: K must lie in" in hip.lib.lib.pgb_last_error().decode() and np.all(out == GUARD)


# ------------------------------------------------------------------ 5. end to end
N_FIT, M_FIT = 1025, 20


@pytest.fixture(scope="module")
def fit(hip):
    """Two chains of 10 draws behind one sampler: ``y = x0 x1 + x2 + noise`` over five columns."""
    rng = np.random.default_rng(61)
    X = rng.uniform(-1, 1, size=(N_FIT, 5))
    y = 3.0 * X[:, 0] * X[:, 1] + X[:, 2] + rng.normal(0, 0.1, N_FIT)
    op = BARTOp(X, y, m=M_FIT)
    attach_history(op, [sample_chain(op, 60, 10, random_seed=4, chain=c, backend=hip, keep_draws=False) for c in (0, 1)])
    Xm = X.copy()
    Xm[5::17, 1], Xm[3::29, 4] = np.nan, np.nan
    return Xm, rng.uniform(0.5, 2.0, N_FIT), _get_posterior_sampler(op, backend=hip)


def test_friedman_h_end_to_end_against_itself_under_blocking_and_the_planted_interaction(hip, fit, monkeypatch):
    X, w, s = fit
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES", raising=False)
    whole = friedman_h(s, X, weights=w, rows=True)
    assert whole["n_draws"] == 20 and whole["pairs"].shape == (10, 2) and whole["n_nonfinite"] == 0
    job = hstat_mod.HstatJob(s, X, None, None, None, w, None, None, 0.94, True, None)
    (one,) = job.chunks(hip)
    limits = (one.ws_bytes + 64 * job.row_bytes(one) + 8, 2 * one.ws_bytes // 3)      # blocks of 64 rows; chunks of pairs
    for limit in limits:
        monkeypatch.setenv("PGB_PW_BLOCK_BYTES", str(limit))
        again = friedman_h(s, X, weights=w, rows=True)
        for key in hstat_mod.PER_DRAW:
            for suffix in ("", "_mean", "_sd", "_hdi"):
                assert np.array_equal(bits(again[key + suffix]), bits(whole[key + suffix])), (limit, key + suffix)
        for part in ("total", "pair"):
            for key in ("mean", "sd", "hdi"):
                assert np.array_equal(bits(again["rows"][part][key]), bits(whole["rows"][part][key])), (limit, part, key)
        assert np.array_equal(again["n_common_trees"], whole["n_common_trees"])
    monkeypatch.delenv("PGB_PW_BLOCK_BYTES")
    some = friedman_h(s, X, cols=[1, 0, 2], pairs=[(1, 0)], weights=w, draws=[3, 15])
    assert np.array_equal(bits(some["h2"][:, 0]), bits(whole["h2"][[3, 15], 0]))
    assert np.array_equal(bits(some["h2_total"]), bits(whole["h2_total"][[3, 15]][:, [1, 0, 2]]))
    # the planted interaction: ordering conditions only
    print("h_mean:", dict(zip(map(tuple, whole["pairs"].tolist()), np.round(whole["h_mean"], 4).tolist())))
    print("h2_total_mean:", np.round(whole["h2_total_mean"], 4).tolist())
    assert whole["pairs"][0].tolist() == [0, 1] and int(np.argmax(whole["h_mean"])) == 0
    assert int(np.argmin(whole["h2_total_mean"][:3])) == 2
