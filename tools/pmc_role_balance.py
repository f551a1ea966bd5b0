#!/usr/bin/env python3
"""Shader-sequencer counters of the one-launch step's kernel, one `rocprofv3 --pmc <counter> --kernel-trace` pass per counter (no
other tracing domain, the program behind `--`, as bench.py's own PMC leg runs it) on `bench.py --steps 40 --warmup 5 --num-envs N`:

    python tools/pmc_role_balance.py [--num-envs 4096,65536] [--out collect_out/pmc_role_balance.md]

Prints a markdown table: per counter and size the median over the kernel's launches, or `refused` with the profiler's last words when
it does not accept the counter.  A pass that ends on a signal or a time limit ends the tool: nothing else is started on the GPU."""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ["SQ_WAVES", "SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES", "SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_INSTS_SALU", "SQ_WAIT_INST_ANY"]
KERNEL = "post_ws_kernel_tick"


def one_pass(prof, counter, n, timeout_s):
    work = tempfile.mkdtemp(prefix="gf_pmc_", dir="/tmp")
    try:
        cmd = [prof, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", work, "-o", "pmc", "--", sys.executable,
               os.path.join(ROOT, "bench.py"), "--steps", "40", "--warmup", "5", "--num-envs", str(n), "--no-cpu-baseline", "--no-profile",
               "--no-sweep", "--no-hbm-point", "--no-pmc"]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s, cwd="/tmp")
        except subprocess.TimeoutExpired:
            return None, "timed out", True
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
            return None, f"ended with {p.returncode}", True
        files = glob.glob(os.path.join(work, "**", "*counter_collection.csv"), recursive=True)
        if p.returncode != 0 or not files:
            words = (p.stderr.strip().splitlines() or ["no counter_collection.csv"])[-1][-160:]
            return None, f"refused (exit {p.returncode}): {words}", False
        vals = [float(r["Counter_Value"]) for r in csv.DictReader(open(files[0])) if r.get("Counter_Name") == counter and KERNEL in r.get("Kernel_Name", "")]
        if not vals:
            return None, f"no launch of {KERNEL} in the pass", False
        return (statistics.median(vals), len(vals)), "ok", False
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", default="4096,65536")
    ap.add_argument("--out", default=os.path.join(ROOT, "collect_out", "pmc_role_balance.md"))
    ap.add_argument("--timeout", type=float, default=120.0)
    args = ap.parse_args()
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    sizes = [int(x) for x in args.num_envs.split(",")]
    rows, stop = [], False
    for counter in COUNTERS:
        cells = []
        for n in sizes:
            if stop:
                cells.append("not run")
                continue
            val, how, stop = one_pass(prof, counter, n, args.timeout)
            cells.append(f"{val[0]:.0f} ({val[1]} launches)" if val else how)
            print(counter, n, cells[-1], flush=True)
        rows.append((counter, cells))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"| counter (median over the launches of `{KERNEL}`) | " + " | ".join(f"{n} envs" for n in sizes) + " |\n")
        f.write("|---|" + "---|" * len(sizes) + "\n")
        for counter, cells in rows:
            f.write(f"| `{counter}` | " + " | ".join(cells) + " |\n")
    print(open(args.out).read())
    return 1 if stop else 0


if __name__ == "__main__":
    sys.exit(main())
