"""The eleven timing tools of ``tools/`` still write what their committed files hold: one run of each, in this process,
at its smallest documented shape with ``--reps 1``, and the key paths of the file it writes compared with the key paths
of ``profiles/<tool>.json`` -- for the shape timed, under ``kernels`` and at the top level.  Nothing is asserted about
the times.  (``diag_timing`` takes about 6 s here, most of them its NumPy route on 2000 columns; the others about 1 s
each.)

``rowsummary_timing`` and ``ppc_timing`` have no committed file under ``profiles/``: their reference is the file each
wrote for this very command before the tools shared ``tools/_timing.py``, kept under ``tests/golden/timing_tools/``.
"""
import importlib
import json
import os
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tool -> (its arguments, the shape of the file that the run fills: a key of "shapes", an index into it, or None when
# the file is one flat record).  psis / psis_expect: a tenth of the rows and pointwise's draw count, which keeps the
# Pareto tail at 20 draws; fewer make PSIS warn about its own fit.
RUNS = {
    "diag_timing": (["--shapes", "small"], "small"),
    "ice_timing": (["--shapes", "plot"], "plot"),
    "pdp_timing": (["--shapes", "plot"], "plot"),
    "pointwise_timing": (["--shapes", "cfg2", "--small"], 0),
    "ppc_timing": (["--shapes", "plot"], "plot"),
    "psis_expect_timing": (["--small", "--draws", "100"], None),
    "psis_timing": (["--small", "--draws", "100"], None),
    "rowreduce_timing": (["--shapes", "plot"], "plot"),
    "rowsummary_timing": (["--shapes", "plot"], "plot"),
    "shap_interaction_timing": (["--shapes", "plot"], "plot"),
    "shap_timing": (["--shapes", "plot"], "plot"),
}
# what only a --baseline-root run writes (pointwise_timing: only an --ab-lib run), a path and everything below it
NOT_WRITTEN_HERE = {
    "ice_timing": ["baseline", "baseline_spread_ms", "speedup", "required/below_the_baseline_by_more_than_its_spread"],
    "pdp_timing": ["baseline", "baseline_spread_ms", "speedup", "required/plot_not_slower_than_the_baseline_beyond_its_spread"],
    "rowsummary_timing": ["baseline", "baseline_spread_ms", "speedup", "below_the_baseline_by_more_than_its_spread"],
    "psis_timing": ["baseline/package", "baseline/has_loo", "baseline/chain_seconds"],
    "psis_expect_timing": ["baseline/package", "baseline/has_loo_pit", "baseline/chain_seconds"],
    "pointwise_timing": ["median_ms/ab_fused_matrix", "median_ms/ab_fused_summary", "min_ms/ab_fused_matrix",
                         "min_ms/ab_fused_summary"],
}


def paths(obj, prefix=""):
    """The nested dict keys of ``obj`` as ``a/b/c``; a list stands for its first element."""
    if isinstance(obj, list):
        obj = obj[0] if obj else None
    out = set()
    if isinstance(obj, dict):
        for k, v in obj.items():
            out.add(prefix + k)
            out |= paths(v, prefix + k + "/")
    return out


def sections(doc, shape, drop):
    """``{section: key paths}`` of a tool's file: the shape timed, ``kernels`` and the rest of the top level."""
    def kept(ps):
        return {p for p in ps if not any(p == d or p.startswith(d + "/") for d in drop)}

    top = {k: v for k, v in doc.items() if k != "kernels" and (shape is None or k != "shapes")}
    out = {"top": kept(paths(top)), "kernels": paths(doc["kernels"])}
    if shape is not None:
        out["shape"] = kept(paths(doc["shapes"][shape]))
    return out


def reference(tool):
    for where in (os.path.join(ROOT, "profiles"), os.path.join(ROOT, "tests", "golden", "timing_tools")):
        if os.path.exists(os.path.join(where, tool + ".json")):
            with open(os.path.join(where, tool + ".json")) as fh:
                return json.load(fh)
    raise AssertionError(f"no committed file of {tool}")


@pytest.mark.gpu
def test_every_timing_tool_writes_the_key_paths_of_its_committed_file(tmp_path, monkeypatch):
    monkeypatch.setattr(sys, "path", [os.path.join(ROOT, "tools")] + list(sys.path))
    monkeypatch.setenv("PGB_JIT_CACHE", str(tmp_path / "jit"))        # (three tools set a default of their own)
    for tool, (argv, shape) in RUNS.items():
        out = tmp_path / (tool + ".json")
        t0 = time.perf_counter()
        rc = importlib.import_module(tool).main(argv + ["--reps", "1", "--out", str(out)])
        print(f"{tool}: {time.perf_counter() - t0:.1f} s, exit status {rc}")
        assert rc in (0, 1), tool                                     # (1: a tool's own verdict on its times)
        text = out.read_text()
        assert text.endswith("}\n"), tool
        got = sections(json.loads(text), shape, NOT_WRITTEN_HERE.get(tool, []))
        want = sections(reference(tool), shape, NOT_WRITTEN_HERE.get(tool, []))
        for section in want:
            assert got[section] == want[section], (tool, section, sorted(got[section] ^ want[section]))
