#!/usr/bin/env python3
"""Generate tests/golden/sat_runs.json: exact fingerprints of the CPU oracle on the saturating cases of
tests/_cases.py (SAT_CASES) -- `digest` plus the saturation counter after every step, whether the step raised and the
count in the error's text.  A case is written only if its run reaches what it is for (check_sat_reach); the events
of every step are printed.  The oracle is regression-pinned against the file on CPU (tests/test_saturation.py) and
the HIP backend must reproduce it bit for bit (tests/test_saturation_gpu.py)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _cases import SAT_CASES, check_sat_reach, make_sat, run_sat_case, sat_digest  # noqa: E402
from _oracle import oracle_backend  # noqa: E402

out = {}
for name in SAT_CASES:
    c = make_sat(name)
    res = run_sat_case(c, oracle_backend())
    r = check_sat_reach(c, res)
    out[name] = sat_digest(res)
    print(name, out[name]["sha256"][:16], "events per step", r["events"],
          "of them beyond sum_trees" if "from_running_sd" in r else "", r.get("from_running_sd", ""))
json.dump(out, open(os.path.join(HERE, "sat_runs.json"), "w"), indent=1)
