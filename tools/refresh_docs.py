#!/usr/bin/env python3
"""After `ROUND=rNN tools/final_profiles.sh` on the GPU box: copy gpurun_out/fin/rNN_* into profiles/ and regenerate
the parts of README.md / DESIGN.md that are generated from the bench line (between the `<!-- bench:begin -->` /
`<!-- bench:end -->` markers).  usage: python tools/refresh_docs.py [ROUND]"""
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RND = sys.argv[1] if len(sys.argv) > 1 else "r06"
fin = os.path.join(ROOT, "gpurun_out", "fin")
for f in sorted(os.listdir(fin)):
    if not f.startswith(RND + "_"):
        continue
    src, dst = os.path.join(fin, f), os.path.join(ROOT, "profiles", f)
    if f == f"{RND}_bench_rccl_world1.json":  # torch.distributed.run prints RCCL's banner first: keep the JSON line
        line = next(ln for ln in open(src) if ln.startswith("{"))
        open(dst, "w").write(line)
    else:
        shutil.copy(src, dst)
d = json.load(open(os.path.join(ROOT, "profiles", f"{RND}_bench.json")))
tab = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "show_bench.py"), "--table",
                               os.path.join(ROOT, "profiles", f"{RND}_bench.json")], text=True).strip()
w4, w5 = d["workloads"]["cfg4"], d["workloads"]["cfg5"]


def us(leg):
    return {k: round(v["avg_us"], 2) for k, v in leg["roofline_kernels"].items()}


rf, r4, r5, rr4, rr5 = d["roofline"], w4["roofline"], w5["roofline"], w4["roofline_rows"], w5["roofline_rows"]
design = f"""`python tools/show_bench.py --table profiles/{RND}_bench.json` (the line `python bench.py --full` printed on the last source state
of the round, `tools/final_profiles.sh`; BASELINE.md §3's table, every row from that ONE line):

{tab}

Per slot, by HIP events attached to every dispatch of the timed region (`roofline_kernels`; `profiles/{RND}_<cfg>_kernel_stats.txt`
is rocprofv3 of the same command): cfg2 `k_ctrl` {us(d)['k_ctrl']} µs (40 workgroups, latency-bound: no roofline) · `k_rows` {us(d)['k_rows']} µs
(1 024 workgroups); cfg4 `k_loglik` {us(w4)['k_loglik']} · `k_rows` {us(w4)['k_rows']} · `k_ctrl` {us(w4)['k_ctrl']} µs; cfg5 `k_loglik` {us(w5)['k_loglik']} ·
`k_rows_mk` {us(w5)['k_rows']} · `k_ctrl` {us(w5)['k_ctrl']} µs.  Kernels are those of round 5 but for the split-row selection of the large data
sets (`profiles/{RND}_experiments.md` §7: `k_ctrl` −0.25 µs at cfg4); the round's work was parity, the boundary and the bench:
differences to `profiles/r05_bench.json` (2.16 M / 559 k / 780 k) are mostly box-to-box spread.

How to read the roofline column.  **cfg2**: the dominant kernel by bytes is `k_rows`: {rf['algorithmic_bytes_per_launch']/1e6:.1f} MB algorithmic
per launch (§8d) ÷ {rf['avg_launch_us']:.2f} µs = {rf['achieved']/1e3:.2f} TB/s = **{rf['frac']:.2f}** of 8 TB/s — a cache work rate: the counters see
{rf['traffic']/1e6:.1f} MB per launch from HBM (`{RND}_pmc_cfg2.json`, FETCH × 2 + WRITE) = {rf['measured_hbm_frac']:.2f} of peak, the columns sit in the Infinity Cache.
Over the wall clock (§8d's own definition, `whole_step_frac`) the astep runs at **{rf['whole_step_frac']:.2f}**: half of it is the control
kernel, which is latency, not bytes; four chains on the one GPU fill those bubbles ({d['concurrent_chains']['value']/1e6:.2f} M aggregate).  **cfg4 / cfg5**: the
dominant kernel is `k_loglik`, bound by fp64-rate vector issue: {r4['valu_wave_insts_per_launch']/1e6:.2f} M / {r5['valu_wave_insts_per_launch']/1e6:.2f} M wave-instructions per launch
(`{RND}_pmc_cfg4.json` / `_cfg5.json`) ÷ its event time = **{r4['frac']:.2f}** / **{r5['frac']:.2f}** of 614 G/s; their row passes move {rr4['traffic']/1e6:.1f} /
{rr5['traffic']/1e6:.1f} MB per launch = {rr4['frac']:.2f} / {rr5['frac']:.2f} of HBM peak, measured.  `whole_step_frac` reads {r4['whole_step_frac']:.2f} / {r5['whole_step_frac']:.2f} there because §8d's
index-list byte model charges 2.5 / 1.7 × the bytes this layout moves for the same result (byte labels, 16-bit order
keys, a shared `pack`) — not because those runs are near the HBM roofline (`profiles/BENCH_NOTES.md`).
What bounds each configuration and what was tried against it: `profiles/{RND}_experiments.md` §3, §6, §7 (cfg4, the kernel
boundary once more), `r05_experiments.md` §3–§5 (cfg5, the heads of the kernels, the row pass), `r02`–`r04_experiments.md` (the
two-kernel slot, flags instead of kernel boundaries, graphs, grid barriers).  CPU rows: `oracle/` built `-O3 -march=native`
on the box ({d['cpu_baseline']['host']['cpu_model']}, {d['cpu_baseline']['host']['nproc']} cores visible), a restatement — the reference's sampler cannot run
here (§0)."""
readme = f"""Measured on one MI355X (round {int(RND[1:])}, steady state after 10 tuning sweeps, one chain per GPU; every row below comes
from the ONE line `python bench.py --full` prints — `profiles/{RND}_bench.json` — and the table itself is the output of
`python tools/show_bench.py --table profiles/{RND}_bench.json`, the form of BASELINE.md's results table):

{tab}"""


def splice(path, text):
    s = open(path).read()
    a, b = s.index("<!-- bench:begin -->"), s.index("<!-- bench:end -->")
    open(path, "w").write(s[:a] + "<!-- bench:begin -->\n" + text + "\n" + s[b:])


splice(os.path.join(ROOT, "DESIGN.md"), design)
splice(os.path.join(ROOT, "README.md"), readme)
print(tab)
