#!/usr/bin/env python3
"""Parity hunt on a GPU box: random configurations (tests/_cases.random_case) through the HIP library and
the CPU oracle, bit-for-bit digests compared.
usage: python tools/fuzz_hunt.py FIRST_SEED COUNT [SECONDS] [large] [compat] [mk] [migrate] [--caps] [--extremes]
(--caps: the configurations of tests/_cases.random_cap_case instead -- trees driven into the limits of 255 nodes and
depth 64; the share of oracle runs that a limit stops (cap_reach) is printed; large and compat do not apply;
large: n = 50k .. 1M, few trees; compat: the upstream-semantics switches on, PGB_COMPAT_* = 1 + seed % 3;
mk: only the configurations with K-vector leaves -- the seeds of the others are skipped;
migrate: the GPU chain is moved to the oracle and back through the chain image -- pgb_checkpoint_save / _load,
include/pgbart_image.h -- at random steps, and must still be the chain the oracle runs alone;
--extremes: every continuous column of the configuration is recoded onto a random ladder of tests/_extreme_cases.py --
neighbouring doubles, beyond the float32 range, subnormals, -inf .. +inf -- by draws of their own, made after the
configuration's; the HIP chain on the recoded data must be the oracle's there AND, but for the split values, the HIP
chain on the data as drawn.  Constant leaves only: the seeds of linear / mix configurations are skipped.  Run it with
PGB_X32_MIN_MB=0 as well: the order keys of such columns)

usage: python tools/fuzz_hunt.py FIRST_SEED COUNT [SECONDS] --stored [ENTRY ...]
(--stored: the stored-draw entry points instead of the sampler -- tests/_stored_fuzz.random_walk_case draws a pool, a
forest table, rows and every argument of a call at once; each ENTRY of _stored_fuzz.RUNNERS, default all of them, lays
the device call out as its GPU module does and holds it to its host reference: bit for bit, guard cells, padding,
identities.  The same MISMATCH and summary lines and the same exit status; the counts are by (entry point, p at or
below / above PRED_LDS_MAXP, rules, K).  A GPU error ends the hunt: nothing is started after it.)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _cases import cap_reach, digest, random_cap_case, random_case, run_case  # noqa: E402
from _oracle import oracle_backend  # noqa: E402
from pymc_bart_amd.sampler import default_backend  # noqa: E402

first, count = int(sys.argv[1]), int(sys.argv[2])
budget = float(sys.argv[3]) if len(sys.argv) > 3 and not sys.argv[3].startswith("--") else 1e9


def hunt_stored(entries) -> int:
    import _stored_fuzz as F

    unknown = [e for e in entries if e not in F.RUNNERS]
    if unknown:
        sys.exit(f"no such entry point: {unknown}; the runners are {sorted(F.RUNNERS)}")
    entries = entries or sorted(F.RUNNERS)
    hip, orc = default_backend(0), oracle_backend()
    t0, bad, done, runs, by = time.time(), [], 0, 0, {}
    for seed in range(first, first + count):
        if time.time() - t0 > budget:
            break
        c = F.random_walk_case(seed, orc)
        for entry in entries:
            diff = F.check(entry, c, hip, orc)  # (a GPU error is no AssertionError: it ends the hunt here)
            key = (entry, "p > LDS" if c["p"] > F.LDS_MAXP else "p <= LDS", c["took"]["rules"], c["K"])
            by[key] = by.get(key, 0) + 1
            runs += 1
            if diff:
                bad.append((seed, entry))
                print("MISMATCH", seed, entry, "; ".join(diff), "|", F.describe(c), flush=True)
        done += 1
    dt = time.time() - t0
    print(f"fuzz: seeds {first}..{first + done - 1}: {done} configurations, {len(bad)} mismatches {bad}, {dt:.0f} s")
    print(f"stored: {runs} runs of {len(entries)} entry points, {runs / max(dt, 1e-9):.2f} per second")
    print("by (entry point, p, rules, K):", sorted(by.items(), key=lambda kv: -kv[1]))  # (every class: the rare ones matter)
    return 1 if bad else 0


if "--stored" in sys.argv[3:]:
    sys.exit(hunt_stored(sys.argv[sys.argv.index("--stored") + 1:]))
large = "large" in sys.argv[4:]
compat_on = "compat" in sys.argv[4:]
mk_only = "mk" in sys.argv[4:]
migrate = "migrate" in sys.argv[4:]
caps = "--caps" in sys.argv[3:]
extremes = "--extremes" in sys.argv[3:]
import numpy as np  # noqa: E402
hip, orc = default_backend(0), oracle_backend()
t0, bad, done, at_a_limit = time.time(), [], 0, 0
fam = {}
for seed in range(first, first + count):
    if time.time() - t0 > budget:
        break
    c = random_cap_case(seed) if caps else random_case(seed, large, compat=(1 + seed % 3) if compat_on else 0)
    if mk_only and int(c["K"]) < 2:
        continue
    if extremes and str(c.get("response", "constant")) != "constant":
        continue
    cuts, plain = (), None
    if extremes:
        from _extreme_cases import LADDERS, remap

        r = np.random.default_rng([seed, 0xE])
        plain = run_case(c, hip)
        c = dict(c, X=remap(c["X"], [str(r.choice(LADDERS)) if rule == 0 else None for rule in c["rules"]])[0])
    if migrate:  # 1..4 cuts, the chain alternating between the backends (the first move is to the oracle)
        r = np.random.default_rng(seed)
        at = sorted(set(int(x) for x in r.integers(1, max(2, c["steps"]), size=int(r.integers(1, 5)))))
        cuts = {a: (orc if i % 2 == 0 else hip) for i, a in enumerate(at)}
    ores = run_case(c, orc)
    g, o = digest(run_case(c, hip, checkpoint_at=cuts)), digest(ores)
    if caps:
        r = cap_reach(c, ores)
        at_a_limit += int(r["node_cap"] > 0 or r["depth_cap"] > 0)
    done += 1
    key = (c["family"], int(c["K"]), str(c.get("response", "constant")))
    fam[key] = fam.get(key, 0) + 1
    if plain is not None:  # rank invariance on the device: everything but the split values is where it was
        f0, f1 = plain["forest"], ores["forest"]
        same = (np.array_equal(plain["sum_trees"], ores["sum_trees"]) and np.array_equal(plain["vi"], ores["vi"])
                and plain["counters"] == ores["counters"] and np.array_equal(f0.var, f1.var)
                and np.array_equal(f0.count, f1.count) and np.array_equal(f0.value, f1.value))
        if not same:
            g = None
    if g != o:
        bad.append(seed)
        print("MISMATCH", seed, c["family"], c["X"].shape, c["m"], c["P"], c["K"], c["rules"].tolist(), flush=True)
print(f"fuzz: seeds {first}..{first + done - 1}: {done} configurations, {len(bad)} mismatches {bad}, {time.time() - t0:.0f} s")
if caps:
    print(f"oracle runs stopped by a limit (255 nodes or depth 64): {at_a_limit} of {done}")
print("by (family, K, response):", sorted(fam.items(), key=lambda kv: -kv[1])[:12])
sys.exit(1 if bad else 0)
