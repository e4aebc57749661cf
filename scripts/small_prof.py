#!/usr/bin/env python3
"""Per-kernel times of one small fit step (config 1 shape) from the engine's HIP-event profiler.  Chosen for launch counts and
per-kernel microseconds of a launch-bound step, on small random weights (normal, sigma 0.01): such weights run at another
clock than the SIREN init (stream_probe.py measured it), so read step rates from small_bench.py."""
from _common import LR, kernel_table, timing_engine

for hidden, depth, size in ((64, 4, 256), (256, 8, 512)):
    eng = timing_engine(size, hidden, depth, init="randn0.01")
    eng.step([LR] * 3)
    eng.profile(True)
    eng.profile_reset()
    n = 20
    eng.step([LR] * n)
    rep = kernel_table(eng, n)
    print(hidden, depth, size, {k: (round(v["total_ms"] * 1e3, 1), int(v["launches"])) for k, v in rep.items()},
          "sum_us", round(sum(v["total_ms"] for v in rep.values()) * 1e3, 1), flush=True)
    eng.close()
