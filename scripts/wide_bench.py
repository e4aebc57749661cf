#!/usr/bin/env python3
"""Wide-path timing: per-kernel table of one fit step at hidden 512 / 1024 (BASELINE configs 3 and 5 shapes)."""
import json
import sys

from _common import kernel_table, timed_steps, timing_engine


def run(hidden, depth, size, steps=3, warm=1, fmt=0):
    eng = timing_engine(size, hidden, depth, fmt=fmt)
    dt = timed_steps(eng, steps, warm, profile=True)
    pw = 2 * hidden + (depth - 2) * hidden * hidden + 3 * hidden
    F = 6 * pw - 4 * hidden
    out = {"hidden": hidden, "depth": depth, "size": size, "scratch_format": eng.scratch_format, "ms_per_step": dt * 1e3,
           "Mpix_iters_per_s": size * size / dt / 1e6, "step_TFLOPs": size * size * F / dt / 1e12,
           "kernels": {k: {"ms_per_step": v["total_ms"], "launches": v["launches"],
                           "tflops": v["flops_per_launch"] * v["launches"] / max(v["total_ms"], 1e-9) / 1e9}
                       for k, v in kernel_table(eng, steps).items()}}
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    fmts = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [0]     # e.g. "16,12": both phase formats
    for hidden, depth, size in ((512, 8, 2048), (1024, 12, 1024)):
        for fmt in fmts:
            run(hidden, depth, size, fmt=fmt)
