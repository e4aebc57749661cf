#!/usr/bin/env python3
"""Time per training step of B small fits on one MI355X: the parent commit's route - sf_step per handle in turn, with graph
replay and (beside it) eagerly - against this tree's sf_step_many, which launches every kernel of a step once for all B.

    python scripts/step_many_bench.py --parent <tree of the parent commit, library built in place> [--out profiles/step_many_bench.json]
    python scripts/step_many_bench.py --parent <tree> --sweep      # and the wall time of an 8-seed `make fit` sweep, batch_jobs 1 / 8

Both libraries are loaded into this process (the parent's through ctypes beside the product's), each with its own B handles
in the same state at scratch format 16.  A round is 50 steps of all B fits between two synchronises on the host clock; the
legs alternate for --rounds rounds (a b c a b c ...) after one warm-up round each, so that no leg owns the warm or the
throttled end of the run.  Reported per leg: median, minimum and maximum microseconds per step and fit.
Acceptance (64x4 on 256^2, B = 8): the batched median lies below the sequential (replay) median by more than that leg's own
max - min spread.  Every ratio is written down as measured, whatever it is."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

from _common import LR, ROOT, device_note, siren_init_params

import torch

SHAPES = [("64x4@256", 64, 4, 256, 0.0), ("128x8@256", 128, 8, 256, 0.0), ("128x8@512 masked 0.5", 128, 8, 512, 0.5)]
BATCHES = (1, 2, 4, 8, 16, 32)
STEPS = 50


def parent_library(tree):
    """the parent tree's library beside the product's: the prototypes it has, declared as the binding declares them"""
    from implicit_image import _engine
    lib = C.CDLL(os.path.join(tree, "implicit-image-compression_amd", "csrc", "libsiren_fit.so"))
    for name, (_, args, restype) in _engine.PROTOTYPES.items():
        if hasattr(lib, name):
            getattr(lib, name).argtypes, getattr(lib, name).restype = args, restype
    return lib


def engines(lib, B, hidden, depth, size, density):
    """B handles of `lib` at format 16: the seed-0 SIREN initialisation, a torch.rand target each, a random mask at `density`"""
    from implicit_image import _engine
    head, _engine._lib = _engine._lib, lib                   # (SirenEngine keeps the library it was built with)
    try:
        out = []
        params = siren_init_params(hidden, depth)
        g = torch.Generator(device="cuda").manual_seed(1)
        for b in range(B):
            eng = _engine.SirenEngine(size, size, hidden, depth, scratch_format=16)
            eng.set_params(params)
            eng.set_coords(torch.linspace(0, 1, size).cuda(), torch.linspace(0, 1, size).cuda())
            eng.set_target(torch.rand(size, size, 3, device="cuda", generator=g))
            if density:
                eng.set_masks((torch.rand(eng.num_params, device="cuda", generator=g) < density).float())
            out.append(eng)
        return out
    finally:
        _engine._lib = head


def measure(parent, B, hidden, depth, size, density, rounds):
    from implicit_image import _engine
    seq, many = engines(parent, B, hidden, depth, size, density), engines(_engine.load_library(), B, hidden, depth, size, density)
    lrs, rows = [LR] * STEPS, [[LR] * B for _ in range(STEPS)]

    def sequential(replay):
        def run():
            for e in seq:
                e.set_graph_replay(replay)
                e.step(lrs)
        return run
    legs = {"sequential_replay": sequential(True), "sequential_eager": sequential(False),
            "batched": lambda: _engine.step_many(many, rows)}
    us = {k: [] for k in legs}
    for r in range(rounds + 1):                               # round 0 warms every leg up (graph capture, first launches)
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                us[k].append((time.perf_counter() - t0) * 1e6 / STEPS / B)
    for e in seq + many:
        e.close()
    res = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in us.items()}
    ref = res["sequential_replay"]
    res["replay_over_batched"] = ref["median_us"] / res["batched"]["median_us"]
    res["eager_over_batched"] = res["sequential_eager"]["median_us"] / res["batched"]["median_us"]
    res["sequential_spread_us"] = ref["max_us"] - ref["min_us"]
    res["gain_beyond_spread"] = bool(ref["median_us"] - res["batched"]["median_us"] > res["sequential_spread_us"])
    return res


def sweep_wall(tree, batch):
    """wall seconds of the 8-seed sweep of `make fit` at 64x4 on 256^2 (2000 steps, masking=RigL, quant=none) in `tree`"""
    argv = [sys.executable, "-m", "implicit_image.fit", "seed=0,1,2,3,4,5,6,7", "mlp.hidden_size=64", "mlp.depth=4", "img.height=256",
            "img.width=256", "train.num_steps=2000", "masking=RigL", "quant=none"] + ([f"train.batch_jobs={batch}"] if batch > 1 else [])
    env = dict(os.environ, PYTHONPATH=os.path.join(tree, "implicit-image-compression_amd"), IIC_CONF=os.path.join(tree, "conf"))
    with tempfile.TemporaryDirectory() as where:
        t0 = time.perf_counter()
        subprocess.run(argv, cwd=where, env=env, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built in place")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))), help="indices into SHAPES")
    ap.add_argument("--sweep", action="store_true", help="also time the 8-seed fit sweep with train.batch_jobs 1 and 8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not args.parent or not os.path.exists(os.path.join(args.parent, "implicit-image-compression_amd", "csrc", "libsiren_fit.so")):
        ap.error("--parent: a tree of the parent commit with libsiren_fit.so built in place")
    parent = parent_library(os.path.abspath(args.parent))
    res = {"what": "microseconds per training step and fit, B fits of one shape at scratch format 16: the parent's sf_step per "
                   "handle in turn (graph replay / eager) against sf_step_many; rounds of 50 steps, legs alternating",
           "rounds": args.rounds, "steps_per_round": STEPS, **device_note(), "shapes": {}}
    for idx in args.shapes:
        name, hidden, depth, size, density = SHAPES[idx]
        res["shapes"][name] = {}
        for B in args.batches:
            r = measure(parent, B, hidden, depth, size, density, args.rounds)
            res["shapes"][name][str(B)] = r
            print(json.dumps({"shape": name, "B": B, **{k: (round(v["median_us"], 2) if isinstance(v, dict) else v) for k, v in r.items()}}),
                  flush=True)
    at8 = res["shapes"].get(SHAPES[0][0], {}).get("8")
    if at8:
        res["accepted"] = at8["gain_beyond_spread"]
    if args.sweep:
        res["sweep_8_seeds_64x4_256_2000_steps"] = {"parent_s": sweep_wall(os.path.abspath(args.parent), 1),
                                                    "batch_jobs_1_s": sweep_wall(ROOT, 1), "batch_jobs_8_s": sweep_wall(ROOT, 8)}
        print(json.dumps(res["sweep_8_seeds_64x4_256_2000_steps"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
