#!/usr/bin/env python3
"""Decode time and device memory of the FourierNet render path (sf_render on an sf_fourier_render_create handle) against the
decode path it replaces, on one MI355X.

    python scripts/fourier_render_bench.py [--sizes 2048 4096] [--calls 30] [--out profiles/fourier_render_bench.json]

Model: conf/mlp/fourier.yaml (hidden 128, depth 8 = 7 Linear layers, map_size 256, map_scale 16).  Per size, HIP-event time
per call after warm-up, median and p10..p90 over --calls calls, of
  (a) FourierNet.forward in eval mode (a training handle: sf_forward with pred) + decode.to_u8 on the device - what
      decode.render_torch runs for mlp=fourier;
  (b) sf_forward(pred) alone on that training handle, into a buffer allocated once;
  (c) sf_render to bytes on a render handle;
and at 16 bits per sample (decode.bits=16), under keys of their own,
  (a16) sf_forward(pred) on the training handle + decode.to_u16 - what a user had for 16 bits before sf_render16;
  (c16) sf_render16 to uint16 samples on the same render handle.
The legs alternate in blocks (a b c a16 c16 a b c a16 c16) inside one process, so all see the same device state.  Device memory held by
each kind of handle: torch.cuda.mem_get_info before / after creation in a fresh child process per handle.
"""
import argparse
import json
import os

import torch

from _common import ROOT, alternate, device_note, handle_memory, print_handle_bytes, stats

YAML = dict(depth=8, hidden_size=128, map_size=256, map_scale=16.0)
N_LINEAR = YAML["depth"] - 1


def time_leg(S, calls, warmup):
    from implicit_image._engine import FourierRenderEngine
    from implicit_image.data import get_grid
    from implicit_image.decode import to_u8, to_u16
    from implicit_image.models import registry
    torch.manual_seed(0)
    model = registry["fourier"](**YAML).cuda().eval()
    grid = get_grid(S, S).cuda()
    tr = model.engine(grid)
    flat = torch.cat([p.data.reshape(-1).float() for p in model._param_list()]).contiguous().cuda()
    rn = FourierRenderEngine(S, S, YAML["hidden_size"], N_LINEAR, YAML["map_size"])
    lin = torch.linspace(0, 1, S).cuda()
    rn.set_coords(lin, lin)
    rn.set_params(flat)
    rn.set_encoding(model.encoding.B.data.float())
    u8 = torch.empty(S, S, 3, dtype=torch.uint8, device="cuda")
    pred = torch.empty(S, S, 3, device="cuda")
    u16 = torch.empty(S, S, 3, dtype=torch.int16, device="cuda")       # (uint16 samples; int16 is what every torch converts)

    def model_bytes():
        with torch.no_grad():
            return to_u8(model(grid))

    def forward_pred():
        tr.lib.sf_forward(tr.h, pred.data_ptr(), None)

    def render():
        rn.lib.sf_render(rn.h, u8.data_ptr(), None)

    def forward_u16():
        tr.lib.sf_forward(tr.h, pred.data_ptr(), None)
        return to_u16(pred)

    def render16():
        rn.lib.sf_render16(rn.h, u16.data_ptr(), None)

    legs = {"model_forward_plus_torch_bytes": model_bytes, "sf_forward_pred": forward_pred, "sf_render_bytes": render,
            "sf_forward_pred_plus_torch_u16": forward_u16, "sf_render16_samples": render16}
    ms = alternate(legs, calls, warmup)
    same = bool(torch.equal(model_bytes(), u8))
    same16 = bool(torch.equal(forward_u16(), u16.to(torch.int32) & 0xFFFF))
    rn.profile(True)
    rn.profile_reset()
    for _ in range(calls):
        render()
    rep = rn.profile_report()
    rn.profile(False)
    rn.close()
    model._unbind()
    del u8, u16, pred, grid
    torch.cuda.empty_cache()
    r = {k: stats(v) for k, v in ms.items()}
    a, c = r["model_forward_plus_torch_bytes"], r["sf_render_bytes"]
    r["k_ff_render_ms"] = rep["k_ff_render"]["total_ms"] / max(rep["k_ff_render"]["launches"], 1)
    r["bytes_identical"] = same
    r["samples16_identical"] = same16
    r["render16_over_forward_plus_u16"] = r["sf_render16_samples"]["median_ms"] / r["sf_forward_pred_plus_torch_u16"]["median_ms"]
    r["render16_over_render_bytes"] = r["sf_render16_samples"]["median_ms"] / c["median_ms"]
    r["render_over_model_plus_bytes"] = c["median_ms"] / a["median_ms"]
    r["render_over_sf_forward"] = c["median_ms"] / r["sf_forward_pred"]["median_ms"]
    r["render_median_below_p10_of_a"] = bool(c["median_ms"] < a["p10_ms"])
    return r


def mem_child(kind, S):
    from implicit_image._engine import FourierEngine, FourierRenderEngine
    print_handle_bytes(lambda: (FourierRenderEngine if kind == "render" else FourierEngine)(
        S, S, YAML["hidden_size"], N_LINEAR, YAML["map_size"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fourier_render_bench.json"))
    ap.add_argument("--mem-child", nargs=2, metavar=("KIND", "SIZE"))
    args = ap.parse_args()
    if args.mem_child:
        return mem_child(args.mem_child[0], int(args.mem_child[1]))
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    res = {"what": "FourierNet 128 x 7 Linear, map 256, HIP-event ms per call; (a) FourierNet.forward (training handle) + torch "
                   "byte conversion, (b) sf_forward(pred) alone on that handle, (c) sf_render to bytes on a render handle; "
                   "(a16) sf_forward(pred) + decode.to_u16, (c16) sf_render16 to uint16 samples on that render handle; "
                   "k_ff_render from the render handle's profile; handle memory from torch.cuda.mem_get_info in a fresh "
                   "process per handle",
           "before": device_note(), "sizes": {}}
    for S in args.sizes:
        r = time_leg(S, args.calls, args.warmup)
        mem = r["memory"] = handle_memory(__file__, S)
        res["sizes"][str(S)] = r
        print(json.dumps({S: {"a_ms": r["model_forward_plus_torch_bytes"]["median_ms"],
                              "a_p90_ms": r["model_forward_plus_torch_bytes"]["p90_ms"],
                              "b_ms": r["sf_forward_pred"]["median_ms"], "c_ms": r["sf_render_bytes"]["median_ms"],
                              "a16_ms": r["sf_forward_pred_plus_torch_u16"]["median_ms"],
                              "c16_ms": r["sf_render16_samples"]["median_ms"],
                              "bytes_identical": r["bytes_identical"], **mem}}),
              flush=True)
    res["after"] = device_note()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
