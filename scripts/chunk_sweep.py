"""SIREN 256x8 at SIZE^2 (default 2048): step time and per-kernel ms against the pixel chunk size."""
import sys
from _common import kernel_table, timed_steps, timing_engine
H = W = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
for chunk in [16384, 32768, 65536, 131072, 262144, 1 << 20, 1 << 22]:
    if chunk > H * W: break
    eng = timing_engine(H, 256, 8, chunk=chunk)
    dt = timed_steps(eng, 4, 2, profile=True)
    print(f"chunk {chunk:8d}: {dt*1e3:8.2f} ms/step {H*W/dt/1e6:7.1f} Mpix/s | " + " ".join(f"{k[2:]}={v['total_ms']:.2f}" for k, v in kernel_table(eng, 4).items() if v['total_ms'] > 0.05), flush=True)
    eng.close()
