#!/usr/bin/env python3
"""Probe: step rate of the same fit on the default (null) stream vs an explicitly created stream, and with
SIREN-initialised vs small random weights (clock / data effects)."""
import torch
from _common import timed_steps, timing_engine

size, steps = 4096, 5
img = torch.rand(size, size, 3, device="cuda")
for name, stream in (("null stream", torch.cuda.current_stream()), ("created stream", torch.cuda.Stream())):
    for wname, init in (("siren init", "siren"), ("uniform +-0.03", "uniform0.03")):
        with torch.cuda.stream(stream):
            e = timing_engine(size, 256, 8, init=init, target=img)
            dt = timed_steps(e, steps, 2)
            print(f"{name:15s} {wname:15s}: {dt * 1e3:.2f} ms/step, {size * size / dt / 1e6:.1f} Mpix-it/s", flush=True)
            e.close()
