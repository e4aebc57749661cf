"""Tiny driver for rocprofv3 counter passes: a few fit steps of SIREN 256x8 at SIZE^2 (default 2048)."""
import sys
import torch
from _common import LR, timing_engine
size = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
eng = timing_engine(size, 256, 8)
eng.step([LR] * steps); torch.cuda.synchronize()
print("done")
