#!/usr/bin/env python3
"""Decode-to-bytes time and device memory of the inference-only Feathermap path (sf_feather_render_load + sf_render on a
feather render handle) against the only way there was before it - a FeatherNet training handle - on one MI355X.

    python scripts/feather_render_bench.py [--sizes 1024 4096] [--calls 30] [--out profiles/feather_render_bench.json]

SIREN 128x8 under Feathermap at density 0.2 (n 316, m 32: 20 240 stored floats for 99 843 weights and biases), seeded init.
Per size, HIP-event time per call after warm-up, median and spread over --calls calls, of
  (a) the training handle (sf_create + sf_feather_attach): the feather vector copied into its view, sf_feather_materialise,
      sf_forward with pred, and the torch byte conversion the host needs after it; the forward alone also reported;
  (b) the feather render handle: sf_feather_render_load of the same vector, then sf_render to bytes; sf_render alone (what
      every further band of a decode costs) also reported.
The legs alternate in blocks inside one process, so all see the same device state; the spread of each leg is reported next
to its median.  Device memory held by each handle: torch.cuda.mem_get_info before / after creation in a fresh child process
per handle.
"""
import argparse
import json
import os

import torch

from _common import ROOT, alternate, device_note, handle_memory, print_handle_bytes, stats

HIDDEN, DEPTH, DENSITY = 128, 8, 0.2
N, M = 316, 32
LOGICAL = ([HIDDEN] * (DEPTH - 1) + [3], [2] + [HIDDEN] * (DEPTH - 1))


def feather_vector():
    from implicit_image.models.siren import Siren
    from implicit_image.pipeline.feathermap import FeatherNet
    torch.manual_seed(0)
    net = FeatherNet(Siren(depth=DEPTH, hidden_size=HIDDEN, first_omega_0=50, hidden_omega_0=30), compress=DENSITY)
    assert (net._size_n, net._size_m) == (N, M)
    return torch.cat([p.detach().reshape(-1) for _, p in net.named_parameters()]).float().contiguous()


def train_handle(S):
    from implicit_image._engine import SirenEngine
    eng = SirenEngine(S, S, HIDDEN, DEPTH, scratch_format=16)       # what FeatherNet fits with
    eng.feather_attach(N, M, *LOGICAL)
    return eng


def render_handle(S):
    from implicit_image._engine import FeatherRenderEngine
    return FeatherRenderEngine(S, S, HIDDEN, DEPTH, N, M, *LOGICAL)


def time_leg(S, calls, warmup):
    from implicit_image.decode import to_u8
    from oracle import siren_oracle as so
    flat = feather_vector().cuda()
    gh, gw = (v.cuda() for v in so.grid_vectors(S, S))
    tr, rn = train_handle(S), render_handle(S)
    for e in (tr, rn):
        e.set_coords(gh, gw)
    fview = tr.feather_view("params")
    pred = torch.empty(S, S, 3, device="cuda")
    u8 = torch.empty(S, S, 3, dtype=torch.uint8, device="cuda")

    def fwd_only():
        tr.lib.sf_forward(tr.h, pred.data_ptr(), None)

    def train_decode():
        fview.copy_(flat)
        tr.lib.sf_feather_materialise(tr.h)
        tr.lib.sf_forward(tr.h, pred.data_ptr(), None)
        return to_u8(pred)

    def render_decode():
        rn.lib.sf_feather_render_load(rn.h, flat.data_ptr())
        rn.lib.sf_render(rn.h, u8.data_ptr(), None)

    def render_only():
        rn.lib.sf_render(rn.h, u8.data_ptr(), None)

    train_decode()                                                   # both handles hold weights before a leg runs alone
    render_decode()
    legs = {"forward_pred": fwd_only, "train_handle_decode_to_bytes": train_decode, "render_handle_decode_to_bytes": render_decode,
            "render_bytes": render_only}
    ms = alternate(legs, calls, warmup)
    same = bool(torch.equal(train_decode(), u8))
    same_w = bool(torch.equal(tr.get_params(), rn.get_params()))
    tr._views.clear()
    tr.close()
    rn.close()
    del pred, u8, fview
    torch.cuda.empty_cache()
    r = {k: stats(v) for k, v in ms.items()}
    a, b = r["train_handle_decode_to_bytes"], r["render_handle_decode_to_bytes"]
    r["bytes_identical"] = same
    r["weights_identical"] = same_w
    r["render_over_train_decode"] = b["median_ms"] / a["median_ms"]
    r["render_not_slower_beyond_spread_of_a"] = bool(b["median_ms"] <= a["median_ms"] + (a["p90_ms"] - a["p10_ms"]))
    return r


def mem_child(kind, S):
    print_handle_bytes(lambda: (render_handle if kind == "render" else train_handle)(S))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feather_render_bench.json"))
    ap.add_argument("--mem-child", nargs=2, metavar=("KIND", "SIZE"))
    args = ap.parse_args()
    if args.mem_child:
        return mem_child(args.mem_child[0], int(args.mem_child[1]))
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    res = {"what": "HIP-event ms per call; (a) feather vector -> sf_feather_materialise -> sf_forward(pred) on a training handle "
                   "with sf_feather_attach + torch byte conversion, (b) sf_feather_render_load + sf_render to bytes on a feather "
                   "render handle; handle memory from torch.cuda.mem_get_info in a fresh process per handle",
           "model": {"hidden": HIDDEN, "depth": DEPTH, "density": DENSITY, "n": N, "m": M, "stored": 2 * N * M + 2 * DEPTH},
           "before": device_note(), "sizes": {}}
    for S in args.sizes:
        r = time_leg(S, args.calls, args.warmup)
        mem = r["memory"] = handle_memory(__file__, S)
        res["sizes"][str(S)] = r
        print(json.dumps({f"{HIDDEN}x{DEPTH}@{S}": {"a_ms": r["train_handle_decode_to_bytes"]["median_ms"],
                                                    "fwd_ms": r["forward_pred"]["median_ms"],
                                                    "b_ms": r["render_handle_decode_to_bytes"]["median_ms"],
                                                    "render_ms": r["render_bytes"]["median_ms"],
                                                    "bytes_identical": r["bytes_identical"], **mem}}), flush=True)
    res["after"] = device_note()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
