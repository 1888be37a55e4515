"""The stored-draw fuzz on the MI355X: every entry point that walks a stored forest, on the suite seeds of
``tests/_stored_fuzz.py`` -- all dimensions of a call drawn at once -- against its host reference.  Bit for bit (a NaN on
both sides counts as equal), integers exactly, the guard cells behind every output untouched, the padding's value in no
result, and the identities the entry point's own module states.  A failure names the seed, the entry point and what the
case took: ``_stored_fuzz.random_walk_case(seed)`` alone reproduces it."""
import pytest

import _stored_fuzz as F

pytestmark = pytest.mark.gpu

GROUPS = [F.SUITE_SEEDS[i:i + 4] for i in range(0, len(F.SUITE_SEEDS), 4)]
_CASES = {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for name in ("PGB_PRED_WGS", "PGB_PW_WGS", "PGB_PW_BLOCK_BYTES"):
        monkeypatch.delenv(name, raising=False)


def _case(seed):
    if seed not in _CASES:
        _CASES[seed] = F.random_walk_case(seed)
    return _CASES[seed]


@pytest.mark.parametrize("seeds", GROUPS, ids=lambda g: f"seeds{g[0]}-{g[-1]}")
@pytest.mark.parametrize("entry", sorted(F.ENTRIES))
def test_the_device_equals_its_host_reference(entry, seeds, hip, oracle):
    for seed in seeds:
        case = _case(seed)
        bad = F.check(entry, case, hip, oracle)
        assert not bad, f"{entry}: " + "; ".join(bad) + "\n" + F.describe(case)
