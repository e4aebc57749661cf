#!/usr/bin/env python3
"""Two steps of SIREN 1024x12 on 1024x1024 (one chunk), or of HIDDEN DEPTH SIZE, for rocprofv3 counter passes.  The weights
are small random ones (uniform in +-0.03): traffic and counters per launch do not depend on them, but they run at another
clock than the SIREN init (stream_probe.py measured it), so durations of these passes are not step times."""
import sys
import torch
from _common import LR, timing_engine

hidden, depth, size = (int(x) for x in (sys.argv[1:4] if len(sys.argv) > 3 else (1024, 12, 1024)))
eng = timing_engine(size, hidden, depth, init="uniform0.03")
eng.step([LR] * 2)
torch.cuda.synchronize()
eng.close()
