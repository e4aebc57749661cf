#!/usr/bin/env python3
"""Launch-bound regime: steps/s of small fits (BASELINE config 1: SIREN 64x4 on 256x256) through sf_step."""
from _common import timed_steps, timing_engine

for hidden, depth, size, n in ((64, 4, 256, 2000), (128, 8, 256, 2000), (256, 8, 512, 1000)):
    eng = timing_engine(size, hidden, depth)
    dt = timed_steps(eng, n, 50)
    print(f"{hidden}x{depth} @ {size}^2: {dt * 1e6:.1f} us/step, {size * size / dt / 1e6:.1f} Mpix-iters/s", flush=True)
    eng.close()
