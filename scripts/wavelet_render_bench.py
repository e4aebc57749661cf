#!/usr/bin/env python3
"""Decode time and device memory of the WaveletSiren render path (sf_wavelet_render on a render handle) against the decode
path it replaces, on one MI355X.

    python scripts/wavelet_render_bench.py [--sizes 2048 4096] [--calls 30] [--out profiles/wavelet_render_bench.json]

Model: conf/mlp/wavelet_siren.yaml (128x8).  Per size, HIP-event time per call after warm-up, median and p10..p90 over
--calls calls, of
  (a) WaveletSiren.forward in eval mode (a training handle: sf_forward with pred) + decode.to_u8 on the device - what
      decode.render_torch ran for mlp=wavelet_siren before sf_wavelet_render existed;
  (b) sf_wavelet_render to bytes, full window, on a render handle;
  (c) k_wv_render alone, from the handle's per-kernel profile (a separate profiled pass of (b));
and at 16 bits per sample (decode.bits=16), under keys of their own,
  (a16) WaveletSiren.forward (sf_forward with pred) + decode.to_u16 - what a user had for 16 bits before
        sf_wavelet_render16;
  (b16) sf_wavelet_render16 to uint16 samples, full window, on the same render handle.
The legs alternate in blocks (a b a16 b16 a b a16 b16) inside one process, so both see the same device state.  Device memory held by each
path's handle: torch.cuda.mem_get_info before / after creation in a fresh child process per handle.
"""
import argparse
import json
import os

import torch

from _common import ROOT, alternate, device_note, handle_memory, print_handle_bytes, stats

YAML = dict(depth=8, hidden_size=128, wavelet_levels=1, first_omega_0=50.0, hidden_omega_0=30.0, outermost_linear=True)


def time_leg(S, calls, warmup):
    from implicit_image._engine import WaveletRenderEngine
    from implicit_image.data import get_grid
    from implicit_image.decode import to_u8, to_u16
    from implicit_image.models import registry
    torch.manual_seed(0)
    model = registry["wavelet_siren"](**YAML).cuda().eval()
    grid = get_grid(S, S).cuda()
    flat = torch.cat([p.data.reshape(-1).float() for p in model._param_list()]).contiguous().cuda()
    rn = WaveletRenderEngine(S, YAML["hidden_size"], YAML["depth"], YAML["first_omega_0"], YAML["hidden_omega_0"], True)
    lin = torch.linspace(0, 1, rn.n).cuda()
    rn.set_coords(lin, lin)
    rn.set_params(flat)
    u8 = torch.empty(S, S, 3, dtype=torch.uint8, device="cuda")
    u16 = torch.empty(S, S, 3, dtype=torch.int16, device="cuda")       # (uint16 samples; int16 is what every torch converts)

    def model_bytes():
        with torch.no_grad():
            return to_u8(model(grid))

    def render():
        rn.lib.sf_wavelet_render(rn.h, 0, S, 0, S, u8.data_ptr(), None)

    def model_u16():
        with torch.no_grad():
            return to_u16(model(grid))

    def render16():
        rn.lib.sf_wavelet_render16(rn.h, 0, S, 0, S, u16.data_ptr(), None)

    legs = {"model_forward_plus_torch_bytes": model_bytes, "wavelet_render_bytes": render,
            "model_forward_plus_torch_u16": model_u16, "wavelet_render16_samples": render16}
    ms = alternate(legs, calls, warmup)
    same = bool(torch.equal(model_bytes(), u8))
    same16 = bool(torch.equal(model_u16(), u16.to(torch.int32) & 0xFFFF))
    rn.profile(True)
    rn.profile_reset()
    for _ in range(calls):
        render()
    rep = rn.profile_report()
    rn.profile(False)
    rn.close()
    model._unbind()
    del u8, u16, grid
    torch.cuda.empty_cache()
    r = {k: stats(v) for k, v in ms.items()}
    a, b = r["model_forward_plus_torch_bytes"], r["wavelet_render_bytes"]
    r["profiled_per_call_ms"] = {k: v["total_ms"] / calls for k, v in rep.items() if v["launches"]}
    r["k_wv_render_ms"] = rep["k_wv_render"]["total_ms"] / max(rep["k_wv_render"]["launches"], 1)
    r["bytes_identical"] = same
    r["samples16_identical"] = same16
    r["render16_over_model_plus_u16"] = r["wavelet_render16_samples"]["median_ms"] / r["model_forward_plus_torch_u16"]["median_ms"]
    r["render16_over_render_bytes"] = r["wavelet_render16_samples"]["median_ms"] / b["median_ms"]
    r["render_over_model_plus_bytes"] = b["median_ms"] / a["median_ms"]
    r["render_median_not_above_p90_of_a"] = bool(b["median_ms"] <= a["p90_ms"])
    return r


def mem_child(kind, S):
    from implicit_image._engine import WaveletEngine, WaveletRenderEngine
    print_handle_bytes(lambda: WaveletRenderEngine(S, 128, 8) if kind == "render" else WaveletEngine(S, S, 128, 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavelet_render_bench.json"))
    ap.add_argument("--mem-child", nargs=2, metavar=("KIND", "SIZE"))
    args = ap.parse_args()
    if args.mem_child:
        return mem_child(args.mem_child[0], int(args.mem_child[1]))
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    res = {"what": "WaveletSiren 128x8, HIP-event ms per call; (a) WaveletSiren.forward (training handle) + torch byte conversion, "
                   "(b) sf_wavelet_render to bytes on a render handle, full window, (c) k_wv_render from the handle's profile; "
                   "(a16) WaveletSiren.forward + decode.to_u16, (b16) sf_wavelet_render16 to uint16 samples on that render handle; "
                   "handle memory from torch.cuda.mem_get_info in a fresh process per handle",
           "before": device_note(), "sizes": {}}
    for S in args.sizes:
        r = time_leg(S, args.calls, args.warmup)
        mem = r["memory"] = handle_memory(__file__, S)
        res["sizes"][str(S)] = r
        print(json.dumps({S: {"a_ms": r["model_forward_plus_torch_bytes"]["median_ms"],
                              "a_p90_ms": r["model_forward_plus_torch_bytes"]["p90_ms"],
                              "b_ms": r["wavelet_render_bytes"]["median_ms"], "k_wv_render_ms": r["k_wv_render_ms"],
                              "a16_ms": r["model_forward_plus_torch_u16"]["median_ms"],
                              "b16_ms": r["wavelet_render16_samples"]["median_ms"], **mem}}),
              flush=True)
    res["after"] = device_note()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
