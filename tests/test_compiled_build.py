"""The one build path of the compiled likelihood family (pymc_bart_amd/compiled.py): what the headers hash covers is what
the compilers read, ``__graft_entry__.build`` rebuilds the library from that same list, and the three kinds of build
of one text never share a cache entry.  CPU only."""

import importlib.util
import os
import re
import subprocess

import pytest

from pymc_bart_amd import compiled
from pymc_bart_amd.compiled import compile_loglik, compile_sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = "return mu + aux;"  # (no y, no random call: valid as a density and as a sampler body)
KINDS = ("pass", "pointwise", "sampler")


def _compile(kind):
    return compile_sampler(BOTH) if kind == "sampler" else compile_loglik(BOTH, pointwise=kind == "pointwise")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """BOTH built once as every kind into a fresh cache, with -H on every compiler line: the builds in the order
    of KINDS, the repository files the compilers opened, the cache directory."""
    cache = tmp_path_factory.mktemp("jit")
    opened, real = set(), subprocess.run

    def spy(cmd, **kw):
        if "-o" not in cmd:  # (not a compile: hipcc --version)
            return real(cmd, **kw)
        r = real([*cmd, "-H"], **kw)
        opened.update(a for a in cmd if a.endswith((".c", ".hip")))
        opened.update(m.group(1) for m in re.finditer(r"^\.+ (\S+)$", r.stderr, re.M))
        return r

    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PGB_JIT_CACHE", str(cache))
        mp.setattr(subprocess, "run", spy)
        builds = [_compile(kind) for kind in KINDS]
    mine = {os.path.realpath(f) for f in opened}
    here = tuple(os.path.realpath(d) + os.sep for d in (compiled.CSRC, compiled.INCLUDE))
    return builds, {f for f in mine if f.startswith(here)}, cache


def test_the_headers_hash_covers_every_file_a_run_time_build_reads(built):
    _, opened, _ = built
    listed = {os.path.realpath(f) for f in compiled._header_files()}
    assert opened <= listed, sorted(opened - listed)
    for f in ("include/pgbart_compiled_body.h", "include/pgbart_compiled.h", "pymc_bart_amd/csrc/k_loglik.h",
              "pymc_bart_amd/csrc/h_loglik_compiled.c", "pymc_bart_amd/csrc/h_ppc_compiled.c",
              "pymc_bart_amd/csrc/k_loglik_compiled.hip", "pymc_bart_amd/csrc/k_pointwise_compiled.hip",
              "pymc_bart_amd/csrc/k_ppc_compiled.hip"):
        assert os.path.realpath(os.path.join(ROOT, f)) in opened, f  # (the spy saw the compilers' reads)


def test_the_library_goes_stale_with_every_hashed_file(tmp_path, monkeypatch):
    """build() hands _stale the list of compiled._header_files(): a host unit newer than the library rebuilds it."""
    spec = importlib.util.spec_from_file_location("graft_entry_build", os.path.join(ROOT, "__graft_entry__.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    real = g._stale

    class Seen(Exception):
        pass

    def spy(target, sources):
        raise Seen(target, sources)

    monkeypatch.setattr(g, "_stale", spy)
    with pytest.raises(Seen) as e:  # (the first question build() asks; nothing is compiled)
        g.build(variants=False)
    target, sources = e.value.args
    assert target == g.HIP_SO and set(compiled._header_files()) <= set(sources)
    host_unit = os.path.join(compiled.CSRC, "h_loglik_compiled.c")
    assert host_unit in sources
    lib = tmp_path / "lib.so"
    lib.write_bytes(b"")
    newest = max(os.path.getmtime(s) for s in sources)
    os.utime(lib, (newest + 1, newest + 1))
    assert real(str(lib), sources) is False
    t = os.path.getmtime(host_unit)
    os.utime(lib, (t - 1, t - 1))  # (the host unit touched after the library was built)
    assert real(str(lib), [host_unit]) is True and real(str(lib), sources) is True


def test_the_three_kinds_of_one_text_never_share_a_cache_entry(built, monkeypatch):
    builds, _, cache = built
    keys = [compiled.cache_key(BOTH, []), compiled.cache_key(BOTH, [], pointwise=True),
            compiled.cache_key(BOTH, [], sampler=True)]
    assert len(set(keys)) == 3 and keys == [b.key for b in builds]
    assert [b.cached for b in builds] == [False] * 3  # (built in turn into one directory: no kind hit another's entry)
    assert sorted(os.listdir(cache)) == sorted(k + ext for k in keys for ext in (".co", ".json", ".so"))
    assert len({b.code for b in builds}) == 3

    def boom(*a, **k):
        raise AssertionError("a cache hit runs no subprocess")

    monkeypatch.setenv("PGB_JIT_CACHE", str(cache))
    monkeypatch.setattr(subprocess, "run", boom)
    for kind, b in zip(KINDS, builds):
        again = _compile(kind)
        assert again.cached and again.key == b.key and again.code == b.code and type(again) is type(b)
