"""The timing tools of ``tools/`` without a GPU: every one imports and answers ``--help``, and the pieces of
``tools/_timing.py`` that need no device -- the spread of a baseline, the shapes a run keeps, the file it writes and
the baseline's child process -- do what the tools' own copies of them did."""
import glob
import importlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (image_timing.py is a script without a main(): importing it runs it, on a GPU)
TOOLS = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(ROOT, "tools", "*_timing.py"))
               if os.path.basename(p) not in ("_timing.py", "image_timing.py"))


def test_the_eleven_tools_and_the_compiled_family_one_are_found():
    assert len(TOOLS) == 12 and "rowsummary_timing" in TOOLS and "_timing" not in TOOLS


@pytest.mark.parametrize("tool", TOOLS)
def test_a_tool_imports_and_answers_help_without_a_device(tool, capsys):
    with pytest.raises(SystemExit) as e:
        importlib.import_module(tool).main(["--help"])
    assert e.value.code == 0 and capsys.readouterr().out.startswith("usage:")


def test_spread_is_the_larger_of_the_legs_difference_and_either_legs_range():
    import _timing

    legs = ("host", "host_again")
    b = {"median_ms": {"host": 10.0, "host_again": 13.0}, "min_ms": {"host": 9.5, "host_again": 12.0},
         "max_ms": {"host": 10.5, "host_again": 14.0}, "chain_seconds": 0.3}
    assert _timing.spread(b, legs) == 3.0                       # |10 - 13| over the ranges 1.0 and 2.0
    b = {"median_ms": {"host": 10.0, "host_again": 10.0}, "min_ms": {"host": 9.0, "host_again": 9.75},
         "max_ms": {"host": 10.25, "host_again": 16.0}}
    assert _timing.spread(b, legs) == 6.25                      # the medians agree: host_again's max - min
    b["max_ms"]["host"] = 17.0
    assert _timing.spread(b, legs) == 8.0                       # ... and the other leg's, when it is the larger


def test_by_statistic_turns_time_legs_layout_round():
    import _timing

    t = {"a": {"median_ms": 1.0, "min_ms": 0.5, "max_ms": 2.0}, "b": {"median_ms": 3.0, "min_ms": 2.5, "max_ms": 4.0}}
    assert _timing.by_statistic(t) == {"median_ms": {"a": 1.0, "b": 3.0}, "min_ms": {"a": 0.5, "b": 2.5},
                                       "max_ms": {"a": 2.0, "b": 4.0}}
    assert _timing.by_statistic(t, ["b"])["max_ms"] == {"b": 4.0}


def test_a_run_keeps_the_shapes_it_does_not_time_and_ends_the_file_with_a_newline(tmp_path, capsys):
    import _timing

    out = tmp_path / "x_timing.json"
    assert _timing.kept_shapes(str(out), ["plot"]) == {}        # no file yet
    _timing.write(str(out), {"shapes": {"plot": {"median_ms": 1.0}, "large": {"median_ms": 2.0}}, "kernels": []})
    line = {"reps": 1, "shapes": _timing.kept_shapes(str(out), ["plot"])}
    assert line["shapes"] == {"large": {"median_ms": 2.0}}
    line["shapes"]["plot"] = {"median_ms": 3.0}
    capsys.readouterr()
    _timing.write(str(out), line)
    text = out.read_text()
    assert text.endswith("}\n") and not text.endswith("\n\n")
    assert json.loads(text) == {"reps": 1, "shapes": {"large": {"median_ms": 2.0}, "plot": {"median_ms": 3.0}}}
    assert json.loads(capsys.readouterr().out) == json.loads(text)          # the one JSON line on stdout
    _timing.write(str(out), line, echo=False)
    assert capsys.readouterr().out == "" and out.read_text() == text


def test_the_baseline_is_the_last_baseline_line_of_a_child_given_the_leg_and_the_absolute_root(tmp_path, monkeypatch):
    import _timing

    script = tmp_path / "child.py"
    script.write_text("import json, sys\n"
                      "print('noise before')\n"
                      "print('BASELINE ' + json.dumps({'first': True}))\n"
                      "print('BASELINE-ish noise between')\n"
                      "print('BASELINE ' + json.dumps({'argv': sys.argv[1:]}), flush=True)\n"
                      "print('noise after')\n"
                      "print('to stderr', file=sys.stderr)\n")
    (tmp_path / "parent").mkdir()
    monkeypatch.chdir(tmp_path)
    got = _timing.run_baseline(str(script), "parent", ["--reps", "2", "--shapes", "plot"])
    assert got == {"argv": ["--baseline-leg", "--root", str(tmp_path / "parent"), "--reps", "2", "--shapes", "plot"]}
    assert _timing.BASELINE_SECONDS == 1100


def test_print_baseline_is_what_run_baseline_reads(capsys):
    import _timing

    _timing.print_baseline({"plot": {"chain_seconds": 0.3}})
    assert capsys.readouterr().out == 'BASELINE {"plot": {"chain_seconds": 0.3}}\n'


def test_walk_timing_puts_the_variable_back_also_after_an_exception(monkeypatch):
    import _timing

    monkeypatch.delenv("PGB_WALK_TIMING", raising=False)
    with pytest.raises(RuntimeError):
        with _timing.walk_timing():
            assert os.environ["PGB_WALK_TIMING"] == "1"
            raise RuntimeError
    assert "PGB_WALK_TIMING" not in os.environ
    monkeypatch.setenv("PGB_WALK_TIMING", "0")
    with _timing.walk_timing():
        assert os.environ["PGB_WALK_TIMING"] == "1"
    assert os.environ["PGB_WALK_TIMING"] == "0"
