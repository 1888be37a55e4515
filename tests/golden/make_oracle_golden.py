#!/usr/bin/env python3
"""Generate tests/golden/oracle_runs.json: exact fingerprints of the CPU oracle on the seeded
parity cases of tests/_cases.py.  The HIP backend must reproduce them bit for bit
(tests/test_parity_gpu.py), and the oracle itself is regression-pinned against them on CPU
(tests/test_oracle_golden.py).  Likewise tests/golden/wide_runs.json for the wide design matrices
(tests/test_wide.py, tests/test_wide_gpu.py): a case is written only if its run reaches the column
edges it exists for (check_wide_reach).  And tests/golden/cap_runs.json for the tree-size limits
(tests/test_caps.py, tests/test_caps_gpu.py): a case is written only if its run is stopped by the
limits it exists for (check_cap_reach); the reach table of every case is printed."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _cases import (ALL_CAPS, CASES, WIDE_P, WIDE_VARIANTS, check_cap_reach, check_wide_reach, digest,  # noqa: E402
                    make_cap, make_case, make_wide, run_case)
from _oracle import oracle_backend  # noqa: E402

out = {}
for name in CASES:
    res = run_case(make_case(name), oracle_backend())
    out[name] = digest(res)
    print(name, out[name]["sha256"][:16], out[name]["counters"])
json.dump(out, open(os.path.join(HERE, "oracle_runs.json"), "w"), indent=1)

wide = {}
for p in WIDE_P:
    for variant in WIDE_VARIANTS:
        c = make_wide(p, variant)
        res = run_case(c, oracle_backend())
        r = check_wide_reach(c, res)
        wide[c["name"]] = digest(res)
        print(c["name"], wide[c["name"]]["sha256"][:16], f"splits in blocks {r['blocks'][0]}..{r['blocks'][-1]} of {r['n_blocks']},",
              f"{r['last_column']} on column p - 1, {r['tuned_in_last_block']} weights of the last block tuned")
json.dump(wide, open(os.path.join(HERE, "wide_runs.json"), "w"), indent=1)

caps = {}
COLS = ("max_nodes", "max_depth", "node_cap", "depth_cap", "dropped", "open_leaves", "held_at_depth", "empty_leaves", "first_full")
print("| case | " + " | ".join(COLS) + " |")
print("|---|" + "---|" * len(COLS))
for kind, variant in ALL_CAPS:
    c = make_cap(kind, variant)
    res = run_case(c, oracle_backend())
    r = check_cap_reach(c, res)
    caps[c["name"]] = digest(res)
    print(f"| {c['name']} | " + " | ".join(str(r[k]) for k in COLS) + " |")
json.dump(caps, open(os.path.join(HERE, "cap_runs.json"), "w"), indent=1)
