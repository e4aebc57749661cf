#!/usr/bin/env python3
"""The profiler driver: every rocprofv3 pass the records under profiles/ cite, one child process per pass.

    python3 scripts/profile_passes.py [--dry-run] [--limit SECONDS] [--out DIR] PRESET [TAG]     -> DIR/TAG_*
    (TAG: PRESET; DIR: build/profiles in the repository root, which git ignores)

    collect  kernel stats of the bench line, FETCH_SIZE / WRITE_SIZE / SQ_* / GRBM passes over prof_step.py, a bench.py --full
    wide     wide_bench.py, then per wide shape kernel stats, FETCH_SIZE, WRITE_SIZE and a clock + SQ pass over wide_one.py
    sq       two SQ_* passes and the GRBM pass over prof_step.py
    lds      the LDS-side SQ_* pass over prof_step.py
    ea       L2 <-> HBM interface counters (read side, write side) over the wide and the width-256 step

Each pass runs under `timeout -k 10 LIMIT` with its stderr in a file of its own.  The first pass that exits non-zero (124 /
137 from the limit, 134, 139, a signal, or an ordinary error) ends the run: nothing more is started on the card, the pass and
its status are named, and the driver exits non-zero.  The summaries are made only once every pass is done.  A counter pass
is --pmc with --kernel-trace and no other tracing.  --dry-run prints the command line of every pass and runs nothing.
No torch here: the driver itself never opens the GPU.

The file and directory names behind TAG_ are those of the shell scripts this replaces.  Those wrote into a directory named
after a tool outside the repository; nothing here names it, so give that directory with --out where the output has to land
there."""
import argparse
import os
import re
import shlex
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what a pass runs; a limit belongs to (workload, kind of pass), see LIMITS
WORKLOADS = {
    "bench": ["bench.py", "--full", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-formats"],
    "step2": ["scripts/prof_step.py", "2048", "2"],
    "step3": ["scripts/prof_step.py", "2048", "3"],
    "wide512": ["scripts/wide_one.py", "512", "8", "2048"],
    "wide1024": ["scripts/wide_one.py", "1024", "12", "1024"],
    # run plain, without the profiler, beside the passes of their preset
    "bench_full": ["bench.py", "--full"],
    "wide_bench": ["scripts/wide_bench.py"],
}

# what rocprofv3 collects beside --kernel-trace
COUNTERS = {
    "stats": ["--stats"],
    "fetch": ["--pmc", "FETCH_SIZE"],
    "write": ["--pmc", "WRITE_SIZE"],
    "grbm": ["--pmc", "GRBM_GUI_ACTIVE"],
    "sq_a": ["--pmc", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY",
             "SQ_ACTIVE_INST_ANY", "SQ_BUSY_CYCLES", "SQ_VALU_MFMA_BUSY_CYCLES"],
    "sq_b": ["--pmc", "SQ_WAIT_INST_LDS", "SQ_INSTS_LDS", "SQ_ACTIVE_INST_LDS", "SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU",
             "SQ_INSTS_SALU", "SQ_ACTIVE_INST_SCA", "SQ_INSTS_MFMA"],
    "wide_clk": ["--pmc", "GRBM_GUI_ACTIVE", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_WAVE_CYCLES", "SQ_LDS_BANK_CONFLICT",
                 "SQ_LDS_IDX_ACTIVE"],
    "lds": ["--pmc", "SQ_LDS_CMD_FIFO_FULL", "SQ_LDS_DATA_FIFO_FULL", "SQ_LDS_ADDR_CONFLICT", "SQ_INST_LEVEL_LDS",
            "SQ_INSTS_LDS", "SQ_VALU_MFMA_COEXEC_CYCLES", "SQ_LDS_UNALIGNED_STALL", "SQ_WAVE_CYCLES"],
    "ea_rd": ["--pmc", "TCC_EA0_RDREQ_sum", "TCC_EA0_RDREQ_LEVEL_sum", "TCC_EA0_RDREQ_DRAM_CREDIT_STALL_sum", "TCC_BUSY_sum"],
    "ea_wr": ["--pmc", "TCC_EA0_WRREQ_sum", "TCC_EA0_WRREQ_LEVEL_sum", "TCC_EA0_WRREQ_DRAM_CREDIT_STALL_sum",
              "TCC_EA0_WRREQ_64B_sum"],
}


def _wide(n, workload):
    return [("stats", workload, f"stats_{n}", f"stats_{n}.err", None), ("fetch", workload, f"FETCH_{n}", f"f_{n}.err", None),
            ("write", workload, f"WRITE_{n}", f"w_{n}.err", None), ("wide_clk", workload, f"clk_{n}", f"c_{n}.err", None)]


# preset -> its passes in order: (counter group, workload, output directory, stderr file, stdout file or None: dropped),
# every name behind DIR/TAG_
PRESETS = {
    "collect": [("stats", "bench", "stats", "stats.err", "stats_bench.json"), ("fetch", "step2", "FETCH_SIZE", "pmc1.err", None),
                ("write", "step2", "WRITE_SIZE", "pmc2.err", None), ("sq_a", "step2", "sq", "pmc3.err", None),
                ("grbm", "step3", "grbm", "pmc4.err", None), (None, "bench_full", None, "bench.err", "bench.json")],
    "wide": [(None, "wide_bench", None, "bench.err", "bench.jsonl")] + _wide("512x8", "wide512") + _wide("1024x12", "wide1024"),
    "sq": [("sq_a", "step2", "a", "a.err", None), ("sq_b", "step2", "b", "b.err", None), ("grbm", "step3", "g", "g.err", None)],
    "lds": [("lds", "step2", "c", "c.err", None)],
    "ea": [("ea_rd", "wide512", "rd_wide", "1.err", None), ("ea_wr", "wide512", "wr_wide", "2.err", None),
           ("ea_rd", "step2", "rd_256", "3.err", None), ("ea_wr", "step2", "wr_256", "4.err", None)],
}

# once all passes are done: pmc_summary.py over output directories -> a text file (with a heading line where several share
# one file), then the lines of a file to show (all of it, or those that match a pattern)
SUMMARIES = {
    "wide": [("summary.txt", "== 512x8", ["FETCH_512x8", "WRITE_512x8", "clk_512x8"]),
             ("summary.txt", "== 1024x12", ["FETCH_1024x12", "WRITE_1024x12", "clk_1024x12"])],
    "sq": [("summary.txt", None, ["a", "b", "g"])],
    "lds": [("summary.txt", None, ["c"])],
    "ea": [("wide.txt", None, ["rd_wide", "wr_wide"]), ("256.txt", None, ["rd_256", "wr_256"])],
}
SHOW = {"collect": ("bench.json", ""), "wide": ("bench.jsonl", ""), "sq": ("summary.txt", "k_bwd8h|k_fwd_pipe"),
        "lds": ("summary.txt", "k_bwd8h|k_fwd_pipe|k_bwd8<")}

# seconds per pass, by (workload, profiled?): three times the wall time measured on one MI355X, rounded up to 30 s, at
# least 60 s (the factor covers the first torch import on a fresh machine and a shared host); the measurements are in
# profiles/scripts_identity.txt.  The wide workloads were not measured: they take the limit of the most similar measured pass.
LIMITS = {("bench", True): 60, ("step2", True): 60, ("step3", True): 60, ("bench_full", False): 90,
          ("wide512", True): 60, ("wide1024", True): 60,      # as ("step2", True)
          ("wide_bench", False): 90}                          # as ("bench_full", False)


def run_passes(passes, dry_run=False):
    """Run `passes` in order, each a dict(name, argv, limit, and optionally cwd, env, stdout, stderr: paths; without them the
    child inherits this process's), as one child under `timeout -k 10 limit`.  The first one that exits non-zero ends the
    run: nothing more is started, a line on stderr names the pass and its status, and that status is returned (0: all
    passed).  dry_run: print each command line, run nothing."""
    for p in passes:
        argv = ["timeout", "-k", "10", str(p["limit"]), *p["argv"]]
        if dry_run:
            print(shlex.join(argv))
            continue
        t0 = time.monotonic()
        files = {k: open(p[k], "wb") if p.get(k) else None for k in ("stdout", "stderr")}
        try:
            status = subprocess.run(argv, cwd=p.get("cwd"), env=p.get("env"), stdin=subprocess.DEVNULL, **files).returncode
        finally:
            for f in files.values():
                if f:
                    f.close()
        print(f"pass {p['name']}: status {status} after {time.monotonic() - t0:.1f} s", file=sys.stderr, flush=True)
        if status != 0:
            print(f"pass {p['name']} ended with status {status} (limit {p['limit']} s"
                  + (f", stderr in {p['stderr']}" if p.get("stderr") else "") + "): nothing more is started",
                  file=sys.stderr, flush=True)
            return status
    return 0


def plan(preset, tag, out_dir, limit=None):
    """the passes of `preset` for run_passes; profiled ones run in /tmp with TMPDIR there, as rocprofv3 wants a writable
    working directory of its own"""
    out = os.path.join(out_dir, tag + "_")
    passes = []
    for group, workload, d, err, stdout in PRESETS[preset]:
        script, *args = WORKLOADS[workload]
        argv = ["python3", os.path.join(ROOT, script), *args]
        if group:
            argv = ["rocprofv3", "--kernel-trace", *COUNTERS[group], "--output-format", "csv", "-d", out + d, "--", *argv]
        passes.append(dict(name=f"{tag}_{d or workload}", argv=argv, limit=limit or LIMITS[workload, group is not None],
                           cwd="/tmp" if group else ROOT, env={**os.environ, "TMPDIR": "/tmp"} if group else None,
                           stdout=out + stdout if stdout else os.devnull, stderr=out + err))
    return passes


def summarise(preset, tag, out_dir):
    out = os.path.join(out_dir, tag + "_")
    # the per-dispatch traces are large: only the counters and stats stay (collect keeps those of its counter passes)
    for d in ["stats"] if preset == "collect" else [p[2] for p in PRESETS[preset] if p[2]]:
        for base, _, names in os.walk(out + d):
            for n in names:
                if n.endswith("kernel_trace.csv"):
                    os.remove(os.path.join(base, n))
    for name in {s[0] for s in SUMMARIES.get(preset, ())}:
        open(out + name, "w").close()
    for name, heading, dirs in SUMMARIES.get(preset, ()):
        with open(out + name, "a") as f:
            if heading:
                f.write(heading + "\n")
                f.flush()
            subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pmc_summary.py"), *(out + d for d in dirs)],
                           stdout=f, stderr=subprocess.STDOUT, check=False)
    if preset in SHOW:
        name, pattern = SHOW[preset]
        sys.stdout.writelines(line for line in open(out + name) if re.search(pattern, line))


def main(args):
    ap = argparse.ArgumentParser(usage=__doc__.split("\n\n")[1].strip())
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--limit", type=int, help="seconds for every pass, instead of the measured limits")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "profiles"))
    ap.add_argument("preset", choices=list(PRESETS))
    ap.add_argument("tag", nargs="?")
    a = ap.parse_args(args)
    preset, tag, dry_run, limit, out_dir = a.preset, a.tag or a.preset, a.dry_run, a.limit, os.path.abspath(a.out)
    if not dry_run:
        os.makedirs(out_dir, exist_ok=True)
    status = run_passes(plan(preset, tag, out_dir, limit), dry_run)
    if status == 0 and not dry_run:
        summarise(preset, tag, out_dir)
    return status


if __name__ == "__main__":
    sys.exit(min(abs(main(sys.argv[1:])), 255))      # (a child ended by a signal has a negative status)
