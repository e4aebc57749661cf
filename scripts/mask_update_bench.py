#!/usr/bin/env python3
"""Host time of one RigL topology update - Masking.update_connections() followed by a device synchronise - on one MI355X:
the parent commit's host path against sf_mask_update (csrc/siren_mask.hip), and the wall time of the default masked fit.

    python scripts/mask_update_bench.py --parent <tree of the parent commit, library built in place>
                                        [--updates 24] [--fit-runs 3] [--out profiles/mask_update_bench.json]

Three sides per shape, each in a worker process of its own (two trees cannot be imported into one interpreter), driven
in turn so that the sides alternate update by update and all see the same device state:
    parent       the parent tree's update_connections()
    head_device  this tree, the device route
    head_host    this tree with SIREN_FIT_DEVICE_MASK=0: a check that the untouched host path did not move
Every worker builds the model (RigL as conf/masking/RigL.yaml, density 0.5), trains `interval` = 20 steps before each update,
as the fit does, synchronises, and times update_connections() + torch.cuda.synchronize() with the host clock; the first
--warmup updates are dropped.  Reported: median, min and max per side.  The device route is accepted at a shape when its
median lies below the parent's by more than the parent's own min - max spread there.

Then `python -m implicit_image.fit masking=RigL quant=none train.num_steps=2000` at the first two shapes, parent against
head, alternating, --fit-runs runs each: the `seconds` of result.json (the fit loop's wall time).

    python scripts/mask_update_bench.py --config pruning --parent <tree> [--out profiles/prune_global_bench.json]

The same for masking=Pruning (conf/masking/Pruning.yaml: global-magnitude pruning, an update every 10 steps) and
sf_mask_prune_global: 10 training steps before each update, the trial count of every device update from its status row, the
fit at the first shape with PSNR compared to the last bit; the three sides run in every one of their six orders in turn.  In this mode every worker and every fit runs under a `timeout` of
its own, and the script stops at the first failure.

    python scripts/mask_update_bench.py --config snfs --parent <tree> [--out profiles/snfs_update_bench.json]

The same for masking=SNFS (conf/masking/SNFS.yaml: momentum growth, momentum redistribution, an update every 20 steps) and
sf_mask_update_snfs, with a fourth side, parent_again - a second worker on the parent tree: what two identical builds differ
by, the margin head_host is held to.  Per device update: the water-filling rounds from its status row; per side: how many
updates ran on the device (an update that finds adjusted_growth negative runs on the host).  The fit at the first shape for
--fit-runs model seeds (seed=0, 1, ...), parent against head: the routes are not bit-equal, so the PSNR of each seed is
recorded on both sides, with the parent's spread over the seeds.  Guarded like --config pruning.
"""
import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 4, 256), (256, 8, 512), (256, 8, 1024), (512, 8, 512)]       # hidden, depth, image side
INTERVAL = 20
PRUNE_SHAPES = [(64, 4, 256), (256, 8, 512), (512, 8, 512)]
PRUNE_INTERVAL = 10
WORKER_LIMIT, FIT_LIMIT = 900, 600                                            # seconds, the guarded configurations


class Cfg(dict):
    __getattr__ = dict.get


# What differs between the configurations.  masking: conf/masking/<name>.yaml as the workers build it; interval: training
# steps before each update; guarded: every worker and fit under a `timeout`, the sides in every order in turn, every update's
# time and the ratios to the parent kept; count: what word [1] of a device update's status row counts (None: nothing);
# read_stats: the statistics are read after every update; again: a second worker on the parent tree; seeds: the fit runs once per model seed and the PSNR is compared per seed.
CONFIGS = {
    "rigl": Cfg(masking="RigL", shapes=SHAPES, fit_shapes=SHAPES[:2], interval=INTERVAL, guarded=False, count=None, read_stats=True, again=False,
                seeds=False, out="mask_update_bench.json", text="RigL (conf/masking/RigL.yaml), density 0.5",
                mcfg=Cfg(name="RigL", density=0.5, sparse_init="erdos-renyi-kernel", dense_gradients=True,
                         growth_mode="absolute-gradient", prune_mode="magnitude", redistribution_mode="none", dense=False,
                         prune_rate=0.1, decay_schedule="cosine", end_when=1500, interval=INTERVAL)),
    "pruning": Cfg(masking="Pruning", shapes=PRUNE_SHAPES, fit_shapes=PRUNE_SHAPES[:1], interval=PRUNE_INTERVAL, guarded=True,
                   count="trials", read_stats=True, again=False, seeds=False, out="prune_global_bench.json",
                   text="Pruning (conf/masking/Pruning.yaml); trials: the threshold search's trial count per device update",
                   mcfg=Cfg(name="Pruning", density=1.0, sparse_init="random", final_density=0.5, dense_gradients=True,
                            growth_mode="none", prune_mode="global-magnitude", redistribution_mode="none", dense=False,
                            decay_schedule="magnitude-prune", start_when=5, end_when=1500, interval=PRUNE_INTERVAL)),
    "snfs": Cfg(masking="SNFS", shapes=PRUNE_SHAPES, fit_shapes=PRUNE_SHAPES[:1], interval=INTERVAL, guarded=True, count="rounds",
                read_stats=False, again=True, seeds=True, out="snfs_update_bench.json",
                text="SNFS (conf/masking/SNFS.yaml); rounds: the water-filling rounds per device update; parent_again: a second "
                     "worker on the parent tree",
                mcfg=Cfg(name="SNFS", density=0.05, sparse_init="erdos-renyi-kernel", dense_gradients=True, growth_mode="momentum",
                         prune_mode="magnitude", redistribution_mode="momentum", dense=False, prune_rate=0.1,
                         decay_schedule="cosine", end_when=1500, interval=INTERVAL)),
}


def tree_env(tree, knob=None):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(tree, "implicit-image-compression_amd"), tree]))
    env.pop("SIREN_FIT_DEVICE_MASK", None)
    if knob is not None:
        env["SIREN_FIT_DEVICE_MASK"] = knob
    return env


def worker(hidden, depth, side, config):
    """reads one line per update from stdin, answers with the milliseconds of that update"""
    import torch
    from implicit_image.data import get_grid
    from implicit_image.models import registry
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, setup_mask, train_steps
    from oracle import siren_oracle as so
    c = CONFIGS[config]
    mcfg, interval = c.mcfg, c.interval
    torch.manual_seed(0)
    model = registry["siren"](depth=depth, hidden_size=hidden, first_omega_0=50, hidden_omega_0=30).to("cuda")
    optim, sched = get_optimizer_lr_scheduler(model, Cfg(name="adam", lr=3e-4))
    mask = setup_mask(model, optim, mcfg)
    grid, img = get_grid(side, side).cuda(), so.synthetic_image(side, side, seed=3).cuda().contiguous()
    print("ready", flush=True)
    for _ in sys.stdin:
        train_steps(model, optim, grid, img, interval, lr_scheduler=sched, mask=mask)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mask.update_connections()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        pending = getattr(mask, "_pending", [])
        count = int(pending[-1][0][-1, 1]) if c.count and pending else None      # (the status row of the device update)
        pending = len(pending)
        # (outside the timed span: where the fit's log line reads it.  Not under SNFS: there the next update's argument step
        #  reads adjusted_growth and so pays the transfer of this update's rows inside its own timed span, as in a fit)
        density = mask.stats.total_density if c.read_stats else None
        print(json.dumps({"ms": ms, "device": pending, "density": density, "count": count}), flush=True)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def time_shape(trees, shape, updates, warmup, config="rigl"):
    c = CONFIGS[config]
    procs = {}
    for name, (tree, knob) in trees.items():
        limit = ["timeout", "-k", "10", str(WORKER_LIMIT)] if c.guarded else []
        mode = ["--config", config]
        procs[name] = subprocess.Popen(limit + [sys.executable, os.path.abspath(__file__), *mode, "--worker", *map(str, shape)],
                                       env=tree_env(tree, knob),
                                       cwd=tree, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        for name, p in procs.items():
            line = p.stdout.readline().strip()
            if line != "ready":
                raise RuntimeError(f"{name}: worker did not start ({line!r})")
        got = {name: [] for name in procs}
        for u in range(warmup + updates):
            order = list(procs)
            if c.guarded:                       # every order of the sides in turn, so that no side always follows the same one
                orders = list(itertools.permutations(order))
                order = orders[u % len(orders)]
            for name in order:
                p = procs[name]
                p.stdin.write("go\n")
                p.stdin.flush()
                line = p.stdout.readline()
                if not line:
                    raise RuntimeError(f"{name}: worker ended (exit status {p.poll()})")
                got[name].append(json.loads(line))
    finally:
        for p in procs.values():
            p.stdin.close()
        for p in procs.values():
            if p.wait(timeout=60):
                raise RuntimeError("a worker failed")
    res = {name: stats([r["ms"] for r in rs[warmup:]]) for name, rs in got.items()}
    for name, rs in got.items():
        res[name]["device_updates"] = sum(r["device"] for r in rs)
        res[name]["density_last"] = rs[-1]["density"]
        if c.count and any(r.get("count") is not None for r in rs):
            res[name][c.count] = [r["count"] for r in rs]
    if c.guarded:                               # update by update: under Pruning every side sees the same sequence of searches and
        for name, rs in got.items():            # the cost follows the trial count, so the sides are also compared pairwise (under
            #                                     SNFS the routes part at the all-ties first update: the ratios pair like with like
            #                                     only in the update's number)
            res[name]["ms"] = [round(r["ms"], 4) for r in rs[warmup:]]
        for name in [n for n in res if n != "parent"]:
            ratios = [a / b for a, b in zip(res[name]["ms"], res["parent"]["ms"])]
            res[name]["paired_ratio_to_parent"] = {"median": statistics.median(ratios), "min": min(ratios), "max": max(ratios)}
    par, dev = res["parent"], res["head_device"]
    res["parent_spread_ms"] = par["max_ms"] - par["min_ms"]
    res["accepted"] = bool(dev["median_ms"] < par["median_ms"] - res["parent_spread_ms"])
    res["parent_over_device"] = par["median_ms"] / dev["median_ms"]
    if "parent_again" in res:                   # the knob at 0 against the parent, held to what two identical builds differ by
        res["identical_builds_margin"] = abs(res["parent_again"]["median_ms"] - par["median_ms"]) / par["median_ms"]
        res["head_host_minus_parent"] = (res["head_host"]["median_ms"] - par["median_ms"]) / par["median_ms"]
        res["head_host_within_margin"] = bool(res["head_host_minus_parent"] <= res["identical_builds_margin"])
    return res


def time_fit(trees, shape, runs, config="rigl"):
    hidden, depth, side = shape
    c = CONFIGS[config]
    masking = c.masking
    limit = ["timeout", "-k", "10", str(FIT_LIMIT)] if c.guarded else []
    over = [f"masking={masking}", "quant=none", "train.num_steps=2000", f"img.height={side}", f"img.width={side}",
            f"mlp.hidden_size={hidden}", f"mlp.depth={depth}"]
    got = {name: [] for name in trees}
    for run in range(runs):
        seed = [f"seed={run}"] if c.seeds else []                 # (one model seed per run; otherwise the configured one)
        for name, (tree, knob) in trees.items():
            with tempfile.TemporaryDirectory() as tmp:
                env = dict(tree_env(tree, knob), IIC_CONF=os.path.join(tree, "conf"))
                subprocess.run(limit + [sys.executable, "-m", "implicit_image.fit"] + over + seed, cwd=tmp, env=env, check=True,
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
                found = [os.path.join(dp, "result.json") for dp, _, fs in os.walk(tmp) if "result.json" in fs]
                got[name].append(json.load(open(found[0])))
    return {name: dict(stats([r["seconds"] * 1e3 for r in rs]), PSNR=[r["PSNR"] for r in rs]) for name, rs in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built in place")
    ap.add_argument("--updates", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit-runs", type=int, default=3)
    ap.add_argument("--config", choices=("rigl", "pruning", "snfs"), default="rigl")
    ap.add_argument("--out")
    ap.add_argument("--worker", nargs=3, type=int, metavar=("HIDDEN", "DEPTH", "SIDE"))
    args = ap.parse_args()
    c = CONFIGS[args.config]
    if args.worker:
        return worker(*args.worker, config=args.config)
    if not args.out:
        args.out = os.path.join(ROOT, "profiles", c.out)
    if not args.parent or not os.path.exists(os.path.join(args.parent, "implicit-image-compression_amd", "csrc", "libsiren_fit.so")):
        ap.error("--parent: a tree of the parent commit with libsiren_fit.so built in place")
    if args.updates < 20:
        ap.error("--updates must be at least 20")
    parent = os.path.abspath(args.parent)
    trees = {"parent": (parent, None), "head_device": (ROOT, None), "head_host": (ROOT, "0")}
    if c.again:
        trees["parent_again"] = (parent, None)
    res = {"what": f"host ms of Masking.update_connections() + torch.cuda.synchronize(), {c.interval} training steps before each "
                   f"update, the {len(trees)} sides alternating update by update in worker processes of their own; then the fit "
                   "loop's seconds (as ms) of the default masked fit at 2000 steps, parent against head, alternating",
           "config": c.text, "shapes": {}, "fit": {}}
    for shape in c.shapes:
        tag = f"{shape[0]}x{shape[1]}@{shape[2]}"
        r = res["shapes"][tag] = time_shape(trees, shape, args.updates, args.warmup, args.config)
        print(json.dumps({tag: {k: (round(v["median_ms"], 3), round(v["min_ms"], 3), round(v["max_ms"], 3))
                                for k, v in r.items() if isinstance(v, dict)}, "accepted": r["accepted"]}), flush=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for shape in c.fit_shapes:
        tag = f"{shape[0]}x{shape[1]}@{shape[2]}"
        r = res["fit"][tag] = time_fit({k: trees[k] for k in ("parent", "head_device")}, shape, args.fit_runs, args.config)
        r["psnr_equal"] = len({p for side in ("parent", "head_device") for p in r[side]["PSNR"]}) == 1
        if c.seeds:                             # per seed: the device route's PSNR against the host route's spread over the seeds
            par, dev = r["parent"]["PSNR"], r["head_device"]["PSNR"]
            r["psnr_equal"] = par == dev
            r["parent_psnr_spread"] = max(par) - min(par)
            r["psnr_device_minus_parent"] = [d - p for d, p in zip(dev, par)]
        print(json.dumps({"fit " + tag: {k: round(v["median_ms"], 1) for k, v in r.items() if isinstance(v, dict)},
                          "psnr_equal": r["psnr_equal"]}), flush=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
