"""Per-kernel ms of one fit step at SIZE^2 (default 2048) of SIREN HIDDEN x DEPTH (default 256 x 8) at scratch format FMT
(default 0: the engine chooses) for the library selected by SIREN_FIT_LIB.  usage: python scripts/kbench.py [SIZE [HIDDEN DEPTH FMT]]"""
import sys
from _common import kernel_table, lib_name, timed_steps, timing_engine
if len(sys.argv) not in (1, 2, 5):
    sys.exit(__doc__)
size = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
hidden, depth, fmt = (int(x) for x in sys.argv[2:5]) if len(sys.argv) > 2 else (256, 8, 0)
eng = timing_engine(size, hidden, depth, fmt=fmt)
dt = timed_steps(eng, 5, 2, profile=True)
print(lib_name(), f"{dt*1e3:7.2f} ms/step {size*size/dt/1e6:6.1f} Mpix/s |", " ".join(f"{k[2:]}={v['total_ms']:.2f}" for k, v in kernel_table(eng, 5).items() if v['total_ms'] > 0.05))
