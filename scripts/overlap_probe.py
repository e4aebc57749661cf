#!/usr/bin/env python3
"""Probe: do a forward-heavy and a backward-heavy phase overlap usefully on one GPU?  Two independent engines on
two streams step concurrently (their k_fwd / k_bwd phases drift against each other); compare the aggregate
Mpix-iters/s with one engine alone."""
import sys
import threading
import time

import torch
from _common import LR, timed_steps, timing_engine

size, steps = int(sys.argv[1]) if len(sys.argv) > 1 else 2896, 4


def make(stream):
    with torch.cuda.stream(stream):
        # (the SIREN init: small random weights overflow the backward and run at a higher clock)
        e = timing_engine(size, 256, 8)
    stream.synchronize()
    return e


s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
e1, e2 = make(s1), make(s2)
e2.step([LR])
print(f"one engine : {size * size / timed_steps(e1, steps, 1) / 1e6:.1f} Mpix-it/s")
ths = [threading.Thread(target=lambda e=e: e.step([LR] * steps)) for e in (e1, e2)]
t0 = time.perf_counter()
[t.start() for t in ths]; [t.join() for t in ths]; torch.cuda.synchronize()
t2 = time.perf_counter() - t0
print(f"two engines: {2 * size * size * steps / t2 / 1e6:.1f} Mpix-it/s aggregate")
