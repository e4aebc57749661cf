#!/usr/bin/env python3
"""What leaving the bulk call costs per step: the step-by-step loop of a fit split by image rows (train.pixel_split) against
the ordinary bulk train_steps (sf_step), SIREN 256x8 on 1024^2 and 4096^2 on one MI355X.

    python scripts/pixel_split_bench.py [--runs 12] [--steps 20] [--out profiles/pixel_split_bench.json]

One process, two models of the same seed per shape: `split` carries a RowSplit of a world of one (every step is
forward_backward, Adam, one device copy of the SSE; no collective), `bulk` is the ordinary fit's train_steps.  A run is one
train_steps(n = --steps) between two synchronises by the host clock (the quantity is host-side launch cost, so the host
clock around work that ends in a synchronise is the instrument); the two sides alternate run by run, the order swapped every
round, --warmup runs dropped, the median, min and max of --runs reported as ms per step.

Then a REHEARSAL, labelled as such: two ranks over gloo sharing the one device at 1024^2 (each in a process of its own under
`timeout`, each owning half the rows).  gloo reduces on the host, and the two ranks' kernels share one GPU: the figure says
that the path runs and what it costs here, not what RCCL across devices would."""
import argparse
import json
import os
import statistics
import subprocess
import sys

from _common import LR, ROOT, device_note, time_loop

import torch

HIDDEN, DEPTH = 256, 8
SIDES = (1024, 4096)
REHEARSAL_SIDE = 1024
WORKER_LIMIT = 300                                                               # seconds


def setup(side, rank=0, world=1, split=True):
    """model, optimiser, grid and picture as fit_one makes them; split: this rank's rows under a RowSplit"""
    from implicit_image.data import get_grid, synthetic_image
    from implicit_image.models import registry
    from implicit_image.parallel import RowSplit
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler
    torch.manual_seed(0)
    model = registry["siren"](depth=DEPTH, hidden_size=HIDDEN, first_omega_0=50.0, hidden_omega_0=30.0)
    grid, img = get_grid(side, side), synthetic_image(side, side, seed=3)
    if split:
        rs = RowSplit(side, rank, world, row_coords=grid[:, 0, 0].contiguous())
        model.set_row_split(rs)
        grid, img = grid[rs.row_begin:rs.row_end], img[rs.row_begin:rs.row_end].contiguous()
    model = model.cuda()
    optim, _ = get_optimizer_lr_scheduler(model, {"name": "adam", "lr": LR})
    return model, optim, grid.cuda(), img.cuda()


def stats(ms):
    return {"median_ms_per_step": statistics.median(ms), "min_ms_per_step": min(ms), "max_ms_per_step": max(ms), "runs": len(ms)}


def one_process(side, runs, warmup, steps):
    from implicit_image.utils.train_helper import train_steps
    legs = {"split_world_of_one": setup(side, split=True), "bulk": setup(side, split=False)}
    ms, last = {k: [] for k in legs}, {}
    for u in range(warmup + runs):
        for name in (list(legs) if u % 2 == 0 else list(legs)[::-1]):
            model, optim, grid, img = legs[name]
            got = []
            t = time_loop(lambda: got.append(train_steps(model, optim, grid, img, steps)), 1, "host") / steps
            last[name] = got[0][-1]
            if u >= warmup:
                ms[name].append(t)
    res = {k: stats(v) for k, v in ms.items()}
    res["extra_ms_per_step"] = res["split_world_of_one"]["median_ms_per_step"] - res["bulk"]["median_ms_per_step"]
    res["split_over_bulk"] = res["split_world_of_one"]["median_ms_per_step"] / res["bulk"]["median_ms_per_step"]
    res["last_loss_equal"] = last["split_world_of_one"] == last["bulk"]          # (the two loops are bit-identical)
    for model, *_ in legs.values():
        model.bound_engine.close()
    return res


def rank_worker(side, runs, warmup, steps):
    """one rank of the rehearsal: RANK / WORLD_SIZE / MASTER_* from the environment; rank 0 prints the figures"""
    from implicit_image.parallel import init_split_group
    from implicit_image.utils.train_helper import train_steps
    import torch.distributed as dist
    rank, world, grouped = init_split_group("gloo")
    torch.cuda.set_device(0)
    try:
        model, optim, grid, img = setup(side, rank, world)
        ms = []
        for u in range(warmup + runs):
            dist.barrier()
            t = time_loop(lambda: train_steps(model, optim, grid, img, steps), 1, "host") / steps
            if u >= warmup:
                ms.append(t)
        dist.barrier()
    finally:
        if grouped:
            dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(stats(ms)), flush=True)


def rehearsal(side, runs, warmup, steps, world=2):
    port = 29600 + (os.getpid() % 1000)
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    argv = ["timeout", "-k", "10", str(WORKER_LIMIT), sys.executable, os.path.abspath(__file__), "--rank-worker", str(side),
            "--runs", str(runs), "--warmup", str(warmup), "--steps", str(steps)]
    procs = [subprocess.Popen(argv, env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, text=True) for r in range(world)]
    outs = [p.communicate(timeout=WORKER_LIMIT + 30)[0] for p in procs]
    if any(p.returncode for p in procs):
        raise RuntimeError(f"a rank of the rehearsal failed: exit status {[p.returncode for p in procs]}")
    return json.loads(outs[0].strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_split_bench.json"))
    ap.add_argument("--rank-worker", type=int, metavar="SIDE")
    args = ap.parse_args()
    if args.rank_worker:
        return rank_worker(args.rank_worker, args.runs, args.warmup, args.steps)
    res = {"what": f"ms per step of train_steps({args.steps}) by the host clock between two synchronises, SIREN {HIDDEN}x{DEPTH}: the "
                   "step-by-step loop of a world-of-one pixel-split fit against the ordinary bulk call (sf_step), one process, the "
                   "sides alternating run by run; then two gloo ranks sharing the device (a rehearsal)",
           "device": device_note(), "shapes": {}}
    for side in SIDES:
        r = res["shapes"][f"{HIDDEN}x{DEPTH}@{side}"] = one_process(side, args.runs, args.warmup, args.steps)
        print(json.dumps({side: {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items() if not isinstance(v, dict)},
                          "split": round(r["split_world_of_one"]["median_ms_per_step"], 4),
                          "bulk": round(r["bulk"]["median_ms_per_step"], 4)}), flush=True)
    r = rehearsal(REHEARSAL_SIDE, args.runs, args.warmup, args.steps)
    res["rehearsal_two_gloo_ranks_one_device"] = dict(r, shape=f"{HIDDEN}x{DEPTH}@{REHEARSAL_SIDE}", label=(
        "REHEARSAL: two ranks share one GPU and gloo reduces through the host; not a figure for RCCL across devices"))
    print(json.dumps({"rehearsal": round(r["median_ms_per_step"], 4)}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
