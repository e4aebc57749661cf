#!/usr/bin/env python3
"""Decode time and device memory of the wide render handle (sf_wide_render on an sf_wide_render_create handle) against the
decode path it replaces, on one MI355X.

    python scripts/wide_render_bench.py [--hidden 512 1024] [--sizes 2048 4096] [--chunks 65536 262144 1048576]
                                        [--calls 20] [--out profiles/wide_render_bench.json]

Model: SIREN hidden x 8 at its seed-0 initialisation.  Per (hidden, size), HIP-event time per call of
  (train)  sf_forward(pred) on a training handle of the default format and chunk + decode.to_u8 on the device - what
           decode.render_torch runs for these widths;
  (render) sf_wide_render to bytes on a render handle, once per --chunks value (chunk_pixels of the handle).
Every leg runs in worker processes of its own (a training handle at these sizes holds tens of GB): the legs alternate in two
rounds (train r r r train r r r), each worker warming up and then timing --calls / 2 calls, so that no leg owns the warm or
the throttled end of the run.  A worker also reports what torch.cuda.mem_get_info loses to its handle (measured before
anything else is allocated) and the sha256 of the bytes it produced; the render bytes must equal the training side's.
Reported per leg: median [min .. max] over its calls; per shape: whether the render median is above the training median by
more than that leg's own min-max spread (it stores less and converts nothing, so it should not be), and the fastest chunk
whose handle stays under 1 GiB.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import torch

from _common import ROOT, device_note, siren_init_params, stats, timed, timing_engine

DEPTH = 8
GIB = 1 << 30


def worker(kind, hidden, S, chunk, calls, warmup):
    """one leg in this process: handle memory, warm-up, `calls` timed calls, the sha256 of the bytes -> one JSON line"""
    from implicit_image._engine import WideRenderEngine
    from implicit_image.decode import to_u8
    torch.cuda.init()
    torch.zeros(1, device="cuda")                  # the runtime's own one-time allocations (its fill kernels) come first
    target = torch.rand(S, S, 3, device="cuda") if kind == "train" else None
    del_me = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")      # stays in torch's cache: the parameter vector and the
    del del_me                                                           # coordinates below come out of it, not out of free memory
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    if kind == "train":
        eng = timing_engine(S, hidden, DEPTH, target=target)
    else:
        eng = WideRenderEngine(S, S, hidden, DEPTH, chunk_pixels=chunk)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    if kind == "render":
        lin = torch.linspace(0, 1, S).cuda()
        eng.set_coords(lin, lin)
        eng.set_params(siren_init_params(hidden, DEPTH))
    u8 = torch.empty(S, S, 3, dtype=torch.uint8, device="cuda")
    pred = torch.empty(S, S, 3, device="cuda") if kind == "train" else None

    def call():
        if kind == "train":
            eng.lib.sf_forward(eng.h, pred.data_ptr(), None)
            u8.copy_(to_u8(pred))
        else:
            eng.lib.sf_wide_render(eng.h, u8.data_ptr(), None)

    timed(call, warmup)
    ms = timed(call, calls)
    torch.cuda.synchronize()
    digest = hashlib.sha256(u8.cpu().numpy().tobytes()).hexdigest()
    fmt = eng.scratch_format
    eng.close()
    print(json.dumps({"ms": ms, "handle_bytes": int(free0 - free1), "sha256": digest, "scratch_format": fmt}))


def run_worker(kind, hidden, S, chunk, calls, warmup, limit):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, str(hidden), str(S), str(chunk), str(calls),
                          str(warmup)], stdout=subprocess.PIPE, timeout=limit, check=True).stdout.decode().strip().splitlines()[-1]
    return json.loads(out)


def bench_shape(hidden, S, chunks, calls, warmup, limit):
    legs = [("train", 0)] + [("render", c) for c in chunks]
    got = {leg: {"ms": []} for leg in legs}
    for _ in range(2):
        for leg in legs:
            r = run_worker(leg[0], hidden, S, leg[1], max(calls // 2, 1), warmup, limit)
            got[leg]["ms"] += r.pop("ms")
            got[leg].update(r)
    tr = dict(stats(got[("train", 0)]["ms"]), **{k: v for k, v in got[("train", 0)].items() if k != "ms"})
    res = {"train": tr, "render": {}}
    for c in chunks:
        g = got[("render", c)]
        r = dict(stats(g["ms"]), **{k: v for k, v in g.items() if k != "ms"})
        r["bytes_identical"] = r["sha256"] == tr["sha256"]
        r["over_train"] = r["median_ms"] / tr["median_ms"]
        r["slower_than_train_beyond_its_spread"] = bool(r["median_ms"] - tr["median_ms"] > tr["max_ms"] - tr["min_ms"])
        res["render"][str(c)] = r
    small = {c: r for c, r in res["render"].items() if r["handle_bytes"] < GIB}
    res["fastest_chunk_under_1GiB"] = int(min(small, key=lambda c: small[c]["median_ms"])) if small else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--chunks", type=int, nargs="+", default=[1 << 16, 1 << 18, 1 << 20])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds one worker process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_render_bench.json"))
    ap.add_argument("--worker", nargs=6, metavar=("KIND", "HIDDEN", "SIZE", "CHUNK", "CALLS", "WARMUP"))
    args = ap.parse_args()
    if args.worker:
        kind, *nums = args.worker
        return worker(kind, *map(int, nums))
    res = {"what": f"SIREN hidden x {DEPTH}, seed-0 initialisation, HIP-event ms per call: (train) sf_forward(pred) on a training "
                   "handle + torch byte conversion, (render) sf_wide_render to bytes on a render handle per chunk_pixels; every "
                   "leg in worker processes of its own, two alternating rounds; median [min .. max]; handle memory from "
                   "torch.cuda.mem_get_info in the worker, before anything else is allocated",
           "before": device_note(), "shapes": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for hidden in args.hidden:
        for S in args.sizes:
            r = res["shapes"][f"{hidden}x{DEPTH}@{S}"] = bench_shape(hidden, S, args.chunks, args.calls, args.warmup, args.limit)
            line = {"train": "%.2f [%.2f .. %.2f] ms, %.0f MiB" % (r["train"]["median_ms"], r["train"]["min_ms"], r["train"]["max_ms"],
                                                                   r["train"]["handle_bytes"] / 2 ** 20)}
            for c, v in r["render"].items():
                line[f"render@{c}"] = "%.2f [%.2f .. %.2f] ms, %.0f MiB%s" % (
                    v["median_ms"], v["min_ms"], v["max_ms"], v["handle_bytes"] / 2 ** 20, "" if v["bytes_identical"] else " BYTES DIFFER")
            print(json.dumps({f"{hidden}x{DEPTH}@{S}": line}), flush=True)
            with open(args.out + ".partial", "w") as f:       # (a long run leaves what it has)
                json.dump(res, f, indent=1)
    res["after"] = device_note()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    os.remove(args.out + ".partial")


if __name__ == "__main__":
    main()
