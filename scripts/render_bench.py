#!/usr/bin/env python3
"""Render time and device memory of the inference-only path (sf_render on a render handle) against the training handle's
forward, on one MI355X.

    python scripts/render_bench.py [--sizes 2048 4096] [--calls 30] [--out profiles/render_bench.json]

Per model (SIREN 256x8, 128x8) and size, HIP-event time per call after warm-up, median and spread over --calls calls, of
  (a) sf_forward with pred on a training handle plus the torch byte conversion the host needs after it (the only way to
      render before sf_render existed), the forward alone also reported;
  (b) sf_render to bytes on a render handle;
and at 16 bits per sample (decode.bits=16), under keys of their own,
  (a16) sf_forward with pred plus the torch conversion decode.to_u16 - what a user had for 16 bits before sf_render16;
  (b16) sf_render16 to uint16 samples on the same render handle.
The legs alternate in blocks (a b a16 b16 a b a16 b16) inside one process, so both see the same device state; the spread of each leg
is reported next to its median.  Device memory held by each handle: torch.cuda.mem_get_info before / after creation in
a fresh child process per handle.
"""
import argparse
import json
import os

import torch

from _common import ROOT, alternate, device_note, handle_memory, print_handle_bytes, stats

MODELS = [(256, 8), (128, 8)]


def time_leg(hidden, depth, S, calls, warmup):
    from implicit_image._engine import RenderEngine, SirenEngine
    from implicit_image.decode import to_u8, to_u16
    from oracle import siren_oracle as so
    flat = torch.tensor(so.flatten(so.siren_init(hidden, depth, seed=0))).cuda()
    gh, gw = (v.cuda() for v in so.grid_vectors(S, S))
    tr, rn = SirenEngine(S, S, hidden, depth), RenderEngine(S, S, hidden, depth)
    for e in (tr, rn):
        e.set_coords(gh, gw)
        e.set_params(flat)
    pred = torch.empty(S, S, 3, device="cuda")
    u8 = torch.empty(S, S, 3, dtype=torch.uint8, device="cuda")
    u16 = torch.empty(S, S, 3, dtype=torch.int16, device="cuda")       # (uint16 samples; int16 is what every torch converts)

    def fwd_only():
        tr.lib.sf_forward(tr.h, pred.data_ptr(), None)

    def fwd_bytes():
        tr.lib.sf_forward(tr.h, pred.data_ptr(), None)
        return to_u8(pred)

    def render():
        rn.lib.sf_render(rn.h, u8.data_ptr(), None)

    def fwd_u16():
        tr.lib.sf_forward(tr.h, pred.data_ptr(), None)
        return to_u16(pred)

    def render16():
        rn.lib.sf_render16(rn.h, u16.data_ptr(), None)

    legs = {"forward_pred": fwd_only, "forward_pred_plus_torch_bytes": fwd_bytes, "render_bytes": render,
            "forward_pred_plus_torch_u16": fwd_u16, "render16_samples": render16}
    ms = alternate(legs, calls, warmup)
    same = bool(torch.equal(fwd_bytes(), u8))
    same16 = bool(torch.equal(fwd_u16(), u16.to(torch.int32) & 0xFFFF))
    tr.close()
    rn.close()
    del pred, u8, u16
    torch.cuda.empty_cache()
    r = {k: stats(v) for k, v in ms.items()}
    a, b = r["forward_pred_plus_torch_bytes"], r["render_bytes"]
    r["bytes_identical"] = same
    r["samples16_identical"] = same16
    r["render16_over_forward_plus_u16"] = r["render16_samples"]["median_ms"] / r["forward_pred_plus_torch_u16"]["median_ms"]
    r["render16_over_render_bytes"] = r["render16_samples"]["median_ms"] / b["median_ms"]
    r["render_over_forward_plus_bytes"] = b["median_ms"] / a["median_ms"]
    r["render_over_forward_alone"] = b["median_ms"] / r["forward_pred"]["median_ms"]
    r["render_not_slower_beyond_spread_of_a"] = bool(b["median_ms"] <= a["median_ms"] + (a["p90_ms"] - a["p10_ms"]))
    return r


def mem_child(kind, hidden, depth, S):
    from implicit_image._engine import RenderEngine, SirenEngine
    print_handle_bytes(lambda: (RenderEngine if kind == "render" else SirenEngine)(S, S, hidden, depth))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    ap.add_argument("--mem-child", nargs=4, metavar=("KIND", "HIDDEN", "DEPTH", "SIZE"))
    args = ap.parse_args()
    if args.mem_child:
        k, h, d, s = args.mem_child
        return mem_child(k, int(h), int(d), int(s))
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    res = {"what": "HIP-event ms per call; (a) sf_forward(pred) on a training handle + torch byte conversion, (b) sf_render to bytes "
                   "on a render handle; (a16) sf_forward(pred) + decode.to_u16, (b16) sf_render16 to uint16 samples on that render handle; "
                   "handle memory from torch.cuda.mem_get_info in a fresh process per handle",
           "before": device_note(), "models": {}}
    for hidden, depth in MODELS:
        for S in args.sizes:
            r = time_leg(hidden, depth, S, args.calls, args.warmup)
            mem = r["memory"] = handle_memory(__file__, hidden, depth, S)
            res["models"][f"{hidden}x{depth}@{S}"] = r
            print(json.dumps({f"{hidden}x{depth}@{S}": {"a_ms": r["forward_pred_plus_torch_bytes"]["median_ms"],
                                                        "fwd_ms": r["forward_pred"]["median_ms"],
                                                        "b_ms": r["render_bytes"]["median_ms"],
                                                        "a16_ms": r["forward_pred_plus_torch_u16"]["median_ms"],
                                                        "b16_ms": r["render16_samples"]["median_ms"], **mem}}), flush=True)
    res["after"] = device_note()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
