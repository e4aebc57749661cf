"""Wide path: step time of SIREN 512x8 on 2048^2 (format 12) against the pixel chunk size - do smaller inter-kernel tensors
(closer to the 256 MB Infinity Cache) pay for their extra launches?"""
import sys
from _common import timed_steps, timing_engine
hidden, depth, size = 512, 8, 2048
for chunk in [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "131072,262144,524288,1048576,2097152").split(",")]:
    eng = timing_engine(size, hidden, depth, fmt=12, chunk=chunk)
    dt = timed_steps(eng, 3, 1)
    print(f"chunk {chunk:8d} pixels: {dt*1e3:7.2f} ms/step  {size*size/dt/1e6:6.1f} Mpix/s")
    eng.close()
