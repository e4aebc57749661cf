"""Per-kernel ms of forward_backward ONLY (no Adam: the weights stay the SIREN init, so a build of the library whose gradients
are garbage does not turn the operands into NaN and change the power state) at SIZE^2 (default 4096), library from
SIREN_FIT_LIB, scratch format from FMT (default 0).  usage: python scripts/fb_bench.py [SIZE] [REPS]"""
import os, sys, torch
from _common import kernel_table, lib_name, time_loop, timing_engine
H = W = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
fmt = int(os.environ.get("FMT", "0"))
eng = timing_engine(H, 256, 8, fmt=fmt)
for _ in range(3): eng.forward_backward()
torch.cuda.synchronize()
eng.profile(True); eng.profile_reset()
ms = time_loop(lambda: eng.forward_backward(sync=False), reps, "host")
print(lib_name(), f"fmt {fmt}: {ms:7.2f} ms/pass |", " ".join(f"{k[2:]}={v['total_ms']:.2f}" for k, v in kernel_table(eng, reps).items() if v['total_ms'] > 0.05))
