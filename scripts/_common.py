"""What the scripts here share; each piece has at least two callers.  Importing this is all the path setup a script needs
(the repository root, the package and tests/, for tests/_gpu_fixtures.siren_engine: the oracle-initialised engine), and it
never touches the device.

    SIREN timing scripts:  siren_init_params, timing_engine, timed_steps, kernel_table, lib_name
    model benches:         time_loop
    render benches:        device_note, timed, stats, alternate, print_handle_bytes, handle_memory"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "implicit-image-compression_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

LR = 3e-4


def siren_init_params(hidden, depth):
    """the seed-0 Siren(depth, hidden, 50, 30) initialisation as the engine's flat vector, on the device"""
    from implicit_image.models import Siren
    torch.manual_seed(0)
    return torch.cat([q.detach().reshape(-1) for q in Siren(depth=depth, hidden_size=hidden, first_omega_0=50.0,
                                                              hidden_omega_0=30.0).parameters()]).cuda()


def timing_engine(size, hidden, depth, *, fmt=0, chunk=0, dtype="f16", init="siren", target=None):
    """a SirenEngine at size (an edge, or (H, W)) on the current stream, ready to step: parameters by `init`, the two linspace
    coordinate vectors, and `target` or a torch.rand image.
    init: "siren"       the seed-0 Siren(depth, hidden, 50, 30) initialisation, what a fit starts from
          "randn0.01"   normal, sigma 0.01   } small random weights: the step runs at another (higher) clock than from the
          "uniform0.03" uniform in +-0.03    } SIREN init (stream_probe.py); for launch counts and counter passes"""
    from implicit_image._engine import SirenEngine
    H, W = (size, size) if isinstance(size, int) else size
    eng = SirenEngine(H, W, hidden, depth, compute_dtype=dtype, scratch_format=fmt, chunk_pixels=chunk)
    torch.manual_seed(0)
    if init == "siren":
        params = siren_init_params(hidden, depth)
    else:
        params = {"randn0.01": lambda n: torch.randn(n, device="cuda") * 0.01,
                  "uniform0.03": lambda n: (torch.rand(n, device="cuda") * 2 - 1) * 0.03}[init](eng.num_params)
    eng.set_params(params)
    eng.set_coords(torch.linspace(0, 1, H).cuda(), torch.linspace(0, 1, W).cuda())
    eng.set_target(torch.rand(H, W, 3, device="cuda") if target is None else target)
    return eng


def timed_steps(eng, steps, warm, profile=False):
    """seconds per step: `warm` steps and a synchronise, then the host clock around one step([LR] * steps) and a synchronise;
    profile: the engine's per-kernel HIP events on, and reset, for the timed steps alone (read them with kernel_table)"""
    eng.step([LR] * warm)
    torch.cuda.synchronize()
    if profile:
        eng.profile(True)
        eng.profile_reset()
    return time_loop(lambda: eng.step([LR] * steps), 1, "host") * 1e-3 / steps


def kernel_table(eng, per):
    """{kernel: its profile_report() row} of the kernels that were launched, total_ms and launches divided by `per`"""
    return {k: {**v, "total_ms": v["total_ms"] / per, "launches": v["launches"] / per}
            for k, v in eng.profile_report().items() if v["launches"] > 0}


def lib_name():
    """basename of the library in use (the product's, or the one SIREN_FIT_LIB selects)"""
    from implicit_image._engine import _LIB_PATH
    return os.path.basename(_LIB_PATH)


def time_loop(fn, n, clock):
    """ms per call of n calls of fn() in a row, between two synchronises.  clock: "event" (HIP events on the current stream)
    or "host" (perf_counter, stopped after the closing synchronise)"""
    torch.cuda.synchronize()
    if clock == "event":
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    if clock == "event":
        e1.record()
    torch.cuda.synchronize()
    return (e0.elapsed_time(e1) if clock == "event" else (time.perf_counter() - t0) * 1e3) / n


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
