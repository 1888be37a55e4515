"""The stored-draw fuzz without a device (``tests/_stored_fuzz.py``): the generator is deterministic, draws only valid
calls and meets every limit exactly; ``SUITE_SEEDS`` -- what ``tests/test_stored_fuzz_gpu.py`` runs -- covers every
value of every dimension and the sixteen cells per entry point; and the host references the device is held to are
themselves held, on every suite case, to a restatement that shares neither their header nor its packer (the recounted
use lists, NumPy bins and curves, SciPy densities, the Python restatements of the SHAP headers, the NumPy profile route)
and to the identities that do not go through their headers (the exact walk, efficiency, the recount of the stop nodes,
``pgb_predict`` on the arm copies ...)."""
import numpy as np
import pytest

import _arms_host as arms_host
import _pdp_host as pdp_host
import _permimp_host as permimp
import _predict_exact as E
import _shap_host as shap_host
import _shap_interaction_host as hx
import _surv_host as surv_host
import _stored_fuzz as F

_CASES = {}


def case(seed):
    if seed not in _CASES:
        _CASES[seed] = F.random_walk_case(seed)
    return _CASES[seed]


# ------------------------------------------------------------------ the generator
def _same(a, b) -> bool:
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and len(a) and isinstance(a[0], np.ndarray):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    if hasattr(a, "node_off"):                                           # a pool
        return all(_same(np.asarray(getattr(a, k)), np.asarray(getattr(b, k)))
                   for k in ("node_off", "var", "split", "left", "right", "count", "value", "slope", "xbar", "svar", "rule"))
    return a == b


@pytest.mark.parametrize("seed", [0, 13, 31, 1000, 123456])
def test_the_generator_is_deterministic(seed):
    a, b = F.random_walk_case(seed), F.random_walk_case(seed)
    assert _same(a, b)
    assert not _same(a["X"], F.random_walk_case(seed + 1)["X"])


def test_an_unwalkable_history_does_not_pass_the_validation(oracle):
    c = F.random_walk_case(3)
    F.validate(oracle, c["pool"], c["table"], c["p"])
    pool = c["pool"]
    g = int(np.flatnonzero(np.asarray(pool.var) >= 0)[0])
    pool.left[g] = pool.right[g] = 0                                     # a split whose children are the root: a cycle
    with pytest.raises(Exception):
        F.validate(oracle, pool, c["table"], c["p"])


def test_limits_are_met_exactly_and_never_exceeded():
    """Over the suite seeds and a stretch of random ones: 255 nodes, depth 64, 65 slots of a SHAP term (32 for the
    interactions' pool), PGB_ALE_MAX_BINS, PGB_ARMS_MAX, PGB_ARMS_MAX_COLS and PGB_SURV_MAX_LEVELS are all reached, in
    the suite, and nothing lies beyond them."""
    most = dict(nodes=0, depth=0, slots=0, slots32=0, bins=0, arms=0, arm_cols=0, levels=0)
    for seed in list(F.SUITE_SEEDS) + list(range(5000, 5040)):
        c = case(seed) if seed in F.SUITE_SEEDS else F.random_walk_case(seed)
        pool, p = c["pool"], c["p"]
        here = dict(nodes=int(np.diff(pool.node_off).max()), depth=max(E.tree_depth(pool, t) for t in range(pool.n_trees)),
                    slots=hx.slots(pool, p), slots32=hx.slots(c["pool_u32"], p), bins=max(len(e) - 1 for e in c["edges"]),
                    arms=c["arm_values"].shape[0], arm_cols=len(c["arm_cols"]), levels=len(c["levels_u"]))
        limit = dict(nodes=255, depth=F.MAX_DEPTH, slots=F.SHAP_MAX_U, slots32=F.SHAPX_MAX_U, bins=F.ALE_MAX_BINS, arms=F.ARMS_MAX,
                     arm_cols=F.ARMS_MAX_COLS, levels=F.SURV_MAX_LEVELS)
        for k in most:
            assert here[k] <= limit[k], (seed, k, here[k])
            if seed in F.SUITE_SEEDS:
                most[k] = max(most[k], here[k])
        assert np.all(np.diff(pool.node_off) == np.diff(c["pool_u32"].node_off)) or c["wide_chains"]
        assert c["spare"] is None or c["spare"] not in c["every_used"]
        assert c["reg"] is None or np.all(np.isfinite(c["X"][:, c["reg"]]) | np.isnan(c["X"][:, c["reg"]]))
        assert len(c["picks"]) >= 1 and max(c["picks"]) < c["D"] and c["block"].shape == (c["nb"], p)
    assert most == dict(nodes=255, depth=F.MAX_DEPTH, slots=F.SHAP_MAX_U, slots32=F.SHAPX_MAX_U, bins=F.ALE_MAX_BINS,
                        arms=F.ARMS_MAX, arm_cols=F.ARMS_MAX_COLS, levels=F.SURV_MAX_LEVELS), most


# ------------------------------------------------------------------ coverage is a condition
def test_the_once_only_limits_occur_once_in_the_suite():
    assert sum(1 for s in F.SUITE_SEEDS if case(s)["took"]["bins"] == F.ALE_MAX_BINS) == 1
    assert sum(1 for s in F.SUITE_SEEDS if case(s)["took"]["arms"] == F.ARMS_MAX) == 1


@pytest.mark.parametrize("entry", sorted(F.ENTRIES))
def test_the_suite_seeds_cover_every_value_and_every_cell(entry):
    """Counted over what a case TOOK (a draw that another draw overrules does not count)."""
    took = [case(s)["took"] for s in F.SUITE_SEEDS]
    for dim in F.CONSUMES[entry]:
        seen = {t[dim] for t in took}
        missing = [v for v in F.TOOK_DIMS[dim] if v not in seen]
        assert not missing, (entry, dim, missing)
    cells = set()
    for s in F.SUITE_SEEDS:
        c = case(s)
        nan = bool(np.isnan(c["block"]).any())
        assert nan == (c["took"]["data"] in F.DATA_NAN), (s, c["took"]["data"])
        mixed = bool(np.any(np.asarray(c["pool"].rule)[np.asarray(c["pool"].var) >= 0] != E.CONT))
        assert mixed == (c["took"]["rules"] == "mixed"), s
        cells.add((c["p"] > F.LDS_MAXP, mixed, nan, c["K"] > 1))
    assert len(cells) == 16, sorted(cells)


def test_the_suite_holds_every_tree_shape_and_the_cases_the_issue_names():
    shapes = set()
    for s in F.SUITE_SEEDS:
        c = case(s)
        shapes |= {c["shapes"][t] for t in np.unique(c["table"])}
    assert shapes == set(F.SHAPES)
    assert any(case(s)["took"]["data"] == "unseen-codes" and case(s)["rules"] for s in F.SUITE_SEEDS)
    assert any(case(s)["wide_chains"] for s in F.SUITE_SEEDS)
    took = [case(s)["took"] for s in F.SUITE_SEEDS]
    assert sum(t["all_columns_paired"] for t in took) >= 4 and any(t["all_columns_paired"] and t["cols"] == "all" for t in took)
    assert sum(t["constant_leaves"] for t in took) >= 4                  # (the identities of the interactions and the arms run)
    for a, b in (("picks", "cols"), ("pad", "first_row"), ("excluded", "picks"), ("pairs", "cols_few"), ("bins", "cols")):
        assert len({(t[a], t[b]) for t in took}) >= 8, (a, b)            # (lists of one length do not move together)
    assert any(not case(s)["excluded"] for s in F.SUITE_SEEDS) and any(len(case(s)["excluded"]) == case(s)["p"] for s in F.SUITE_SEEDS)


# ------------------------------------------------------------------ the comparison
def test_the_comparison_sees_one_bit_a_guard_cell_and_the_padding():
    a = np.array([1.0, np.nan, -0.0, 3.0])
    b = a.copy()
    assert F.compare({"x": a, "i": np.arange(3)}, {"x": b, "i": np.arange(3)}, [("g", np.full(4, -7.0), -7.0)]) == []
    b[1] = -np.nan                                                       # (a NaN on both sides: equal whatever its bits)
    assert F.compare({"x": a}, {"x": b}, []) == []
    b[2] = 0.0
    assert len(F.compare({"x": a}, {"x": b}, [])) == 1                    # -0.0 against +0.0
    assert len(F.compare({"x": a}, {"x": np.nextafter(a, 9.0)}, [])) == 1
    assert len(F.compare({"x": a}, {"x": a[:3]}, [])) == 1
    assert len(F.compare({"i": np.arange(3)}, {"i": np.array([0, 1, 3])}, [])) == 1
    assert len(F.compare({"x": a}, {"x": a}, [("g", np.array([-7.0, 0.0]), -7.0)])) == 1
    assert len(F.compare({"x": np.array([F.POISON])}, {"x": np.array([F.POISON])}, [])) == 1


# ------------------------------------------------------------------ the references against their restatements
# Per entry point: the header-based reference of a suite case against a restatement that shares neither the header nor
# its packer -- `recount` from the definition of a use list, NumPy for bins and curves, SciPy for the densities, the
# Python restatements of the SHAP headers, the exact walk.  Bit for bit where the restatement is the same arithmetic.
_CHECKED = {}


def _same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | both))


def _count(entry, n=1):
    _CHECKED[entry] = _CHECKED.get(entry, 0) + n


def _listed(pool, lst, X, oracle):
    """The oracle's ``pgb_predict`` of the trees ``lst`` in that order, from +0.0 for an empty list: (K, n)."""
    return permimp.predict(oracle, pool, np.asarray(lst, np.int32)[None, :], X)[0] if len(lst) else \
        np.zeros((int(pool.n_outputs), X.shape[0]))


def _use_lists_are_the_recount(c, cols):
    args = (c["pool"], c["table"], c["p"], cols, c["picks"])
    off, lst = permimp.use_lists(*args)
    woff, wlst = permimp.recount(*args)
    assert np.array_equal(off, woff) and np.array_equal(lst, wlst), "the packer's use lists are not the recount's"
    return woff, wlst


def restate_predict(c, want, oracle):
    pass                                                                 # (ident_predict: the exact walk)


def restate_pointwise(c, want, oracle):
    """SciPy's densities as ``tests/test_pointwise.py`` writes them, with its tolerances on ``|got - want| / (1 + |want|)``,
    where the predictors lie in the ranges that module derives them for and nothing is near the clamp."""
    from scipy import special, stats

    mu = F.ref_predict(dict(c, excluded=[]), oracle)["out"]              # (D, K, n)
    y, fam = c["y"], c["family"]
    for d in range(mu.shape[0]):
        m, prm = mu[d], c["params"][d]
        tol = 1e-10
        with np.errstate(all="ignore"):
            if fam == "normal":
                ref = stats.norm.logpdf(y, m[0], prm[0])
            elif fam == "student_t":
                ref = stats.t.logpdf(y, prm[1], loc=m[0], scale=prm[0])
            elif fam == "asymmetric_laplace":
                b, q = prm
                ref = stats.laplace_asymmetric.logpdf(y, np.sqrt(q / (1 - q)), loc=m[0], scale=b / np.sqrt(q * (1 - q)))
            elif fam == "gamma_log":
                ref, tol = stats.gamma.logpdf(y, prm[0], scale=np.exp(m[0]) / prm[0]), 1e-9
            elif fam == "poisson_log":
                ref, tol = stats.poisson.logpmf(y, np.exp(m[0])), 1e-9
            elif fam == "negbin_log":
                ref, tol = stats.nbinom.logpmf(y, prm[0], prm[0] / (prm[0] + np.exp(m[0]))), 1e-9
            elif fam.startswith("bernoulli"):
                s = np.where(y > 0.5, m[0], -m[0])
                ref, tol = (special.log_ndtr(s) if fam.endswith("probit") else -np.logaddexp(0.0, -s)), 1e-12
            elif fam == "categorical":
                ref, tol = special.log_softmax(m, axis=0)[y.astype(int), np.arange(y.size)], 1e-12
            else:
                ref = stats.norm.logpdf(y, m[0], np.abs(m[1]))
        span = 8.0 if fam.startswith("bernoulli") else 3.0               # (the predictors test_pointwise.py draws)
        ok = np.all(np.abs(m) <= span, axis=0) & np.isfinite(ref) & (np.abs(ref) < 2000.0)
        if fam == "normal_meanscale":
            ok &= np.abs(m[1]) >= 0.3
        err = np.abs(want["ll"][d] - ref) / (1.0 + np.abs(ref))
        assert np.all(err[ok] <= tol), (fam, d, float(err[ok].max()))
        _count("pgb_pointwise_loglik:" + fam, int(ok.sum()))


def restate_ice(c, want, oracle):
    """Per (column, instance): the probe rows built here, every pick through the oracle's C entry point directly, summed
    in pick order and divided once -- the same bits; the predictions at the sampled rows within the exact walk's bound."""
    import test_predict_edges_gpu as T

    rows = F._sample_rows(c, 3)
    for ci, j in enumerate(c["cols"][:6] + c["cols"][-2:]):
        ci = c["cols"].index(j)
        for r in range(c["instances"].shape[0]):
            probe = np.tile(c["instances"][r], (c["nb"], 1))
            probe[:, j] = c["block"][:, j]
            fidx = c["table"][c["ice_picks"][ci, r]]
            mu = T.predict(oracle, c["pool"], fidx, probe)
            total = mu[0].copy()
            for s in range(1, mu.shape[0]):
                total = total + mu[s]
            assert _same_bits(want["out"][ci, r], total / float(mu.shape[0])), (j, r)
            if r == 0:
                assert E.walk(c["pool"], fidx, probe[rows]).bound_ratio(mu[:, :, rows]) <= 1.0, (j, r)
            _count("pgb_predict_ice")


def restate_pdp(c, want, oracle):
    """Eligible columns: the profile route restated in NumPy (``_pdp_host.profile_sweep``), the same bits.  The others:
    the sampled rows within the exact walk's bound with every other column excluded."""
    s = F._sampler(c, oracle)
    rows = F._sample_rows(c, 3)
    for ci, j in list(enumerate(c["cols"]))[:8]:
        picks = c["pdp_picks"][ci]
        if all(pdp_host.breakpoints(c["pool"], c["table"][d], j)[0] for d in picks.tolist()):
            got = pdp_host.profile_sweep(s, c["block"], [j], picks[None, :])
            assert _same_bits(want["out"][ci], got[0]), ("profile", j)
            _count("pgb_predict_pdp:profile")
        else:
            exact = E.walk(c["pool"], c["table"][picks], c["block"][rows], [v for v in range(c["p"]) if v != j])
            assert exact.bound_ratio(want["out"][ci][:, :, rows]) <= 1.0, ("direct", j)
            _count("pgb_predict_pdp:direct")


def restate_shap(c, want, oracle):
    """``_shap_host.restated`` (the header in Python floats) at one sampled row, two picks: the same bits."""
    rows = [F._sample_rows(c)[-1]]                                       # (a row with a NaN where the block has one)
    phi, base, _, _ = shap_host.restated(c["pool"], c["table"][c["picks"][:2]], c["block"][rows], float)
    assert _same_bits(want["values"][:2][..., rows], phi) and _same_bits(want["base"][:2], base)
    _count("pgb_predict_shap")


def restate_shapx(c, want, oracle):
    """``_shap_interaction_host.restated`` at one row, two picks (a term costs O(u^4) in Python): the same bits."""
    rows = [F._sample_rows(c)[-1]]
    Phi = hx.restated(c["pool_u32"], c["table"][c["picks"][:2]], c["block"][rows], float)
    cols = c["cols_few"]
    assert _same_bits(want["values"][:2][..., rows], Phi[:, :, cols][:, :, :, cols])
    _count("pgb_predict_shap_interactions")


def restate_permuted(c, want, oracle):
    """The use lists recounted from the definition; per (pick, column, repeat) the WHOLE matrix permuted
    (``permuted_matrix``) and the recounted list predicted at the block's rows of it and of the matrix as it is."""
    cols, q = c["cols"], len(c["cols"])
    off, lst = _use_lists_are_the_recount(c, cols)
    lo, hi = c["first_row"], c["first_row"] + c["nb"]
    f = want["f"]
    slots = list(range(q)) if q <= 8 else list(range(4)) + list(range(q - 4, q))
    for d in range(len(c["picks"])):
        for s in slots:
            mine = lst[off[d * q + s]:off[d * q + s + 1]]
            A = _listed(c["pool"], mine, c["block"], oracle)
            for r in range(c["R"]):
                Xp = permimp.permuted_matrix(c["X"], cols[s], c["perm_seed"], r)[lo:hi]
                delta = _listed(c["pool"], mine, Xp, oracle) - A
                assert _same_bits(want["delta"][d, s, r], delta) and _same_bits(want["pred"][d, s, r], f[d] + delta), (d, s, r)
                _count("pgb_predict_permuted")


def restate_ale(c, want, oracle):
    """The use lists recounted; the bins by ``np.searchsorted`` over the interior edges; the two edge copies predicted
    with the recounted list."""
    cols, q = c["cols"], len(c["cols"])
    off, lst = _use_lists_are_the_recount(c, cols)
    slots = list(range(q)) if q <= 8 else list(range(4)) + list(range(q - 4, q))
    for s in slots:
        e, x = np.asarray(c["edges"][s]), c["block"][:, cols[s]]
        B = e.size - 1
        b = np.where(np.isnan(x), B, np.searchsorted(e[1:B], x, side="left"))
        assert np.array_equal(want["bins"][s], b), s
        at = np.where(b == B, 0, b)
        hi, lo = c["block"].copy(), c["block"].copy()
        hi[:, cols[s]], lo[:, cols[s]] = e[at + 1], e[at]
        for d in range(len(c["picks"])):
            mine = lst[off[d * q + s]:off[d * q + s + 1]]
            delta = _listed(c["pool"], mine, hi, oracle) - _listed(c["pool"], mine, lo, oracle)
            delta[:, b == B] = 0.0
            assert _same_bits(want["out"][s, d], delta), (s, d)
            _count("pgb_predict_ale")


def restate_hstat(c, want, oracle):
    """The use lists recounted (the walk's sums come from them) and the common lists' lengths counted from the
    definition: the trees of the pick's forest that use both columns of a pair."""
    cols = c["cols_few"]
    _use_lists_are_the_recount(c, cols)
    uses = [permimp.tree_uses(c["pool"], t, c["p"]) for t in range(c["pool"].n_trees)]
    n_common = np.array([[sum(1 for t in c["table"][d] if cols[a] in uses[int(t)] and cols[b] in uses[int(t)])
                          for a, b in c["pairs"]] for d in c["picks"]], np.int32).reshape(len(c["picks"]), len(c["pairs"]))
    assert np.array_equal(want["n_common"], n_common)
    _count("pgb_hstat")


def restate_arms(c, want, oracle):
    """The union lists recounted from the definition (``ident_arms``: ``pgb_predict`` on the arm copies)."""
    args = (c["pool"], c["table"], c["p"], c["arm_cols"], c["picks"])
    off, lst = arms_host.union_lists(*args)
    woff, wlst = arms_host.recount(*args)
    assert np.array_equal(off, woff) and np.array_equal(lst, wlst) and np.array_equal(want["lens"], np.diff(woff))
    for d in range(len(c["picks"])):                                     # ... and the arms predicted with the recounted list
        mine = wlst[woff[d]:woff[d + 1]]
        f = permimp.predict(oracle, c["pool"], c["table"][c["picks"]], c["block"])[d]
        own = _listed(c["pool"], mine, c["block"], oracle)
        for a in range(min(c["arm_values"].shape[0], 3)):
            copy = arms_host.arm_copy(c["block"], c["arm_cols"], c["arm_values"][a])
            assert _same_bits(want["out"][a, d], f + (_listed(c["pool"], mine, copy, oracle) - own)), (a, d)
            _count("pgb_predict_arms")


def restate_surv(c, want, oracle):
    """``_surv_host.numpy_curves`` on ALL grid times at once (NumPy's sequential accumulates), against the chunks of the
    reference and the state it carried through them."""
    k = c["K"] - 1
    chunks = list(F._surv_chunks(c))
    f = np.concatenate([arms_host.reference_block(oracle, *a)[0] for _, a, _ in chunks])[:, :, k]    # (J, D, nb)
    t, dt = np.concatenate([r[0] for _, _, r in chunks]), np.concatenate([r[1] for _, _, r in chunks])
    _, _, u, beyond, link, off = chunks[0][2]
    S, R, T = surv_host.numpy_curves(f.copy(), t, dt, u, beyond, link, off)
    got_S = np.concatenate([want[f"f{c0}"][:, :, k] for c0, _, _ in chunks])
    assert _same_bits(got_S, S) and _same_bits(want["state"][0], S[-1]) and _same_bits(want["state"][1], R)
    assert _same_bits(want["state"][2:], T)
    _count("pgb_surv_curves")


def restate_leaf_codes(c, want, oracle):
    pass                                                                 # (ident_leaf_codes: the recount of the stop nodes)


RESTATED = {
    "pgb_predict": restate_predict, "pgb_pointwise_loglik": restate_pointwise, "pgb_predict_ice": restate_ice,
    "pgb_predict_pdp": restate_pdp, "pgb_predict_shap": restate_shap, "pgb_predict_shap_interactions": restate_shapx,
    "pgb_predict_permuted": restate_permuted, "pgb_predict_ale": restate_ale, "pgb_hstat": restate_hstat,
    "pgb_predict_arms": restate_arms, "pgb_surv_curves": restate_surv, "pgb_predict_leaf_codes": restate_leaf_codes,
}


@pytest.mark.parametrize("entry", sorted(F.ENTRIES))
def test_the_references_against_the_oracle_and_their_identities(entry, oracle):
    """The reference of every suite case: no padding value and no unexpected non-finite value in it; it equals its
    restatement (above); and the entry point's identities hold on it with the oracle's ``pgb_predict`` as the
    prediction.  ``pgb_predict`` itself, which the oracle implements, goes through its runner whole."""
    _, reference, identities = F.ENTRIES[entry]
    _CHECKED.clear()
    for s in F.SUITE_SEEDS:
        c = case(s)
        want = reference(c, oracle)
        try:
            RESTATED[entry](c, want, oracle)
        except AssertionError as exc:
            raise AssertionError(f"{entry} against its restatement: {exc}\n{F.describe(c)}") from exc
        for name, v in want.items():
            v = np.asarray(v)
            assert not np.any(v == F.POISON), (entry, name, F.describe(c))
            if v.dtype.kind == "f" and entry not in ("pgb_hstat", "pgb_surv_curves", "pgb_pointwise_loglik"):
                assert np.all(np.isfinite(v)), (entry, name, F.describe(c))
        try:
            identities(c, want, oracle)
        except AssertionError as exc:
            raise AssertionError(f"{entry}: {exc}\n{F.describe(c)}") from exc
        if entry == "pgb_predict":
            assert F.check(entry, c, oracle, oracle) == [], F.describe(c)
    if entry == "pgb_pointwise_loglik":                                  # every family met SciPy on some entries
        assert all(_CHECKED.get(entry + ":" + fam, 0) > 0 for fam in F.FAMILIES), _CHECKED
    elif entry == "pgb_predict_pdp":
        assert _CHECKED.get(entry + ":profile", 0) > 0 and _CHECKED.get(entry + ":direct", 0) > 0, _CHECKED
    elif RESTATED[entry] not in (restate_predict, restate_leaf_codes):
        assert _CHECKED.get(entry, 0) >= len(F.SUITE_SEEDS), _CHECKED
