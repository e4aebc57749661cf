"""What the four render bench scripts (render_bench.py, wavelet_render_bench.py, fourier_render_bench.py,
feather_render_bench.py) share: the device note, HIP-event timing and its statistics, the alternating-block leg runner and
the fresh-process handle-memory probe."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "implicit-image-compression_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def device_note():
    note = {"device": torch.cuda.get_device_name(0)}
    # (both as torch reports them: SM clock in MHz, power_draw in the management library's own unit)
    for k, fn in (("clock_mhz", getattr(torch.cuda, "clock_rate", None)), ("power_draw", getattr(torch.cuda, "power_draw", None))):
        try:
            note[k] = fn(0)
        except Exception as e:   # (the management library is optional: say so rather than guess)
            note[k] = f"unavailable ({type(e).__name__})"
    return note


def timed(fn, n):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def stats(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1], "p10_ms": s[len(s) // 10],
            "p90_ms": s[(len(s) * 9) // 10], "calls": len(s)}


def alternate(legs, calls, warmup):
    """{leg: ms per call} of `legs` ({name: fn}): every leg warmed up, then two blocks of calls / 2 per leg in turn
    (a b c a b c), so that no leg owns the warm (or the throttled) end of the run"""
    for fn in legs.values():
        timed(fn, warmup)
    ms = {k: [] for k in legs}
    half = max(calls // 2, 1)
    for _ in range(2):
        for k, fn in legs.items():
            ms[k] += timed(fn, half)
    return ms


def print_handle_bytes(make):
    """the --mem-child side: print what torch.cuda.mem_get_info loses to the handle make() creates, as one JSON line"""
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    eng = make()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    eng.close()
    print(json.dumps({"bytes": int(free0 - free1)}))


def handle_memory(script, *args):
    """{train_handle_bytes, render_handle_bytes}: `script --mem-child KIND *args` in a fresh process per handle"""
    mem = {}
    for kind in ("train", "render"):
        out = subprocess.run([sys.executable, os.path.abspath(script), "--mem-child", kind, *map(str, args)],
                             stdout=subprocess.PIPE, timeout=180, check=True).stdout.decode().strip().splitlines()[-1]
        mem[f"{kind}_handle_bytes"] = json.loads(out)["bytes"]
    return mem
