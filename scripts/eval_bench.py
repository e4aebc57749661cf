#!/usr/bin/env python3
"""Host time of one evaluation on one MI355X: the parent commit's eval_epoch - sf_forward with an fp32 prediction, about ten
torch ops on it, two reads - against eval_metrics (sf_eval: no prediction, no torch arithmetic, one read), torch's peak
allocation during the call on each side, and the wall time of the whole quantise phase of the default fit.

    python scripts/eval_bench.py --parent <tree of the parent commit, library built in place>
                                 [--repeats 24] [--out profiles/eval_bench.json]

Two sides per shape, each in a worker process of its own under a `timeout` (two trees cannot be imported into one
interpreter), driven in turn so that the sides alternate call by call, the order swapped every round:
    parent  the parent tree: eval_epoch(model, grid, img)
    head    this tree: eval_metrics(model, grid, img)
A worker takes the paths, the clock (time_loop) and nothing else from the scripts/_common.py of ITS tree, builds the registry
model as fit_one does, and per request runs one evaluation between two synchronises: ms by the host clock, and the growth of
torch.cuda.max_memory_allocated() over memory_allocated() before the call.  The first --warmup calls are dropped; the median
of --repeats is reported.  Acceptance is the project's rule: at no shape may the head's median exceed the parent's by more
than the parent's own max - min spread (`parent_spread_ms`, `accepted`); the ratios are written down whatever they are.
Then the whole quantise phase of the default fit (SIREN 128x8 on 512^2, quant=kmeans bits 8, 100 steps, an evaluation every
10, the conversion and the evaluation after it) per side in fresh processes.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# family, hidden, depth (Linear layers), image side
SHAPES = [("siren", 128, 8, 512), ("siren", 256, 8, 1024), ("siren", 256, 8, 4096), ("siren", 512, 8, 512),
          ("fourier", 128, 8, 2048), ("wavelet_siren", 128, 8, 2048)]
MAP_SIZE, MAP_SCALE = 256, 16
PHASE_SHAPE, LOG_STEPS, PHASE_STEPS = (128, 8, 512), 10, 100
WORKER_LIMIT = 600                                                               # seconds


def tree_env(tree):
    return dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(tree, "implicit-image-compression_amd"), tree]),
                EVAL_BENCH_TREE=tree)


def tree_common():
    """the scripts/_common.py of the tree this worker measures (its import is the worker's whole path setup)"""
    sys.path.insert(0, os.path.join(os.environ["EVAL_BENCH_TREE"], "scripts"))
    import _common
    assert os.path.dirname(os.path.abspath(_common.__file__)) == os.path.join(os.environ["EVAL_BENCH_TREE"], "scripts")
    return _common


def evaluation():
    """this tree's evaluation as its fit.py calls it: -> (name, fn(model, grid, img) -> (loss, PSNR, PSNR_8bit))"""
    from implicit_image.utils import train_helper
    if hasattr(train_helper, "eval_metrics"):
        return "eval_metrics", train_helper.eval_metrics
    return "eval_epoch", lambda model, grid, img: train_helper.eval_epoch(model, grid, img)[1:]


def worker(family, hidden, depth, side):
    """reads one line per call from stdin, answers with the ms of one evaluation plus synchronise and torch's peak growth"""
    common = tree_common()
    import torch
    from implicit_image.data import get_grid
    from implicit_image.models import registry
    from oracle import siren_oracle as so
    torch.manual_seed(0)
    kw = dict(map_size=MAP_SIZE, map_scale=MAP_SCALE) if family == "fourier" else dict(first_omega_0=50, hidden_omega_0=30)
    model = registry[family](depth=depth, hidden_size=hidden, **kw).to("cuda")
    grid, img = get_grid(side, side).cuda(), so.synthetic_image(side, side, seed=3).cuda().contiguous()
    name, fn = evaluation()
    fn(model, grid, img)                                                         # (the handle exists before the first timed call)
    print("ready", flush=True)
    for _ in sys.stdin:
        got = []
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        ms = common.time_loop(lambda: got.append(fn(model, grid, img)), 1, "host")
        grown = torch.cuda.max_memory_allocated() - before
        loss, psnr, psnr8 = got[0]
        print(json.dumps({"ms": ms, "torch_peak_growth_bytes": int(grown), "route": name, "loss": loss, "PSNR": psnr,
                          "PSNR_8bit": float(psnr8)}), flush=True)


def phase(hidden, depth, side):
    """the whole quantise phase as fit_one's loop runs it, once: its wall time in ms and the figures after the conversion"""
    tree_common()
    import torch
    import quant_phase_bench as qp                                               # (this tree's: the model and quantiser of fit_one)
    from implicit_image.pipeline.quant import Quantize
    model, optim, sched, grid, img, qcfg = qp.setup(hidden, depth, side)
    name, fn = evaluation()
    model.engine(grid, img)                                                      # (the handle exists before the clock starts, as after a fit)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with Quantize(model, optim, qcfg) as q:
        for _ in range(PHASE_STEPS // LOG_STEPS):
            qp.chunk(model, optim, sched, grid, img, LOG_STEPS)
            fn(model, grid, img)
    model = q.convert()
    loss, psnr, psnr8 = fn(model, grid, img)
    torch.cuda.synchronize()
    print(json.dumps({"ms": (time.perf_counter() - t0) * 1e3, "route": name, "loss": loss, "PSNR": psnr, "PSNR_8bit": float(psnr8)}),
          flush=True)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def spawn(tree, mode, shape, **kw):
    return subprocess.Popen(["timeout", "-k", "10", str(WORKER_LIMIT), sys.executable, os.path.abspath(__file__), mode, *map(str, shape)],
                            env=tree_env(tree), cwd=tree, stdout=subprocess.PIPE, text=True, **kw)


def time_shape(trees, shape, repeats, warmup):
    procs = {name: spawn(tree, "--worker", shape, stdin=subprocess.PIPE) for name, tree in trees.items()}
    try:
        for name, p in procs.items():
            line = p.stdout.readline().strip()
            if line != "ready":
                raise RuntimeError(f"{name}: worker did not start ({line!r})")
        got = {name: [] for name in procs}
        for u in range(warmup + repeats):
            for name in (list(procs) if u % 2 == 0 else list(procs)[::-1]):
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
    res = {name: dict(stats([r["ms"] for r in rs[warmup:]]), route=rs[-1]["route"],
                      torch_peak_growth_bytes=max(r["torch_peak_growth_bytes"] for r in rs[warmup:]),
                      loss=rs[-1]["loss"], PSNR=rs[-1]["PSNR"], PSNR_8bit=rs[-1]["PSNR_8bit"]) for name, rs in got.items()}
    par, head = res["parent"], res["head"]
    res["parent_spread_ms"] = par["max_ms"] - par["min_ms"]
    res["accepted"] = bool(head["median_ms"] <= par["median_ms"] + res["parent_spread_ms"])
    res["parent_over_head"] = par["median_ms"] / head["median_ms"]
    res["loss_and_psnr_equal"] = par["loss"] == head["loss"] and par["PSNR"] == head["PSNR"]
    res["psnr8_difference_db"] = abs(par["PSNR_8bit"] - head["PSNR_8bit"])
    return res


def time_phase(trees, runs):
    got = {name: [] for name in trees}
    for _ in range(runs):
        for name, tree in trees.items():
            p = spawn(tree, "--phase", PHASE_SHAPE)
            out, _ = p.communicate(timeout=WORKER_LIMIT + 30)
            if p.returncode:
                raise RuntimeError(f"{name}: the phase worker failed (exit status {p.returncode})")
            got[name].append(json.loads(out.strip().splitlines()[-1]))
    res = {name: dict(stats([r["ms"] for r in rs]), route=rs[-1]["route"], PSNR=[r["PSNR"] for r in rs]) for name, rs in got.items()}
    res["psnr_equal"] = len({p for r in res.values() for p in r["PSNR"]}) == 1
    res["parent_spread_ms"] = res["parent"]["max_ms"] - res["parent"]["min_ms"]
    res["accepted"] = bool(res["head"]["median_ms"] <= res["parent"]["median_ms"] + res["parent_spread_ms"])
    res["parent_over_head"] = res["parent"]["median_ms"] / res["head"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built in place")
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--phase-runs", type=int, default=3)
    ap.add_argument("--shapes", type=int, default=len(SHAPES), help="the first N shapes only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    ap.add_argument("--worker", nargs=4, metavar=("FAMILY", "HIDDEN", "DEPTH", "SIDE"))
    ap.add_argument("--phase", nargs=3, type=int, metavar=("HIDDEN", "DEPTH", "SIDE"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], *map(int, args.worker[1:]))
    if args.phase:
        return phase(*args.phase)
    if not args.parent or not os.path.exists(os.path.join(args.parent, "implicit-image-compression_amd", "csrc", "libsiren_fit.so")):
        ap.error("--parent: a tree of the parent commit with libsiren_fit.so built in place")
    if args.repeats < 24:
        ap.error("--repeats must be at least 24")
    trees = {"parent": os.path.abspath(args.parent), "head": ROOT}
    res = {"what": "host ms of one evaluation plus synchronise - the parent's eval_epoch against this tree's eval_metrics (sf_eval) - "
                   "the two sides alternating call by call in worker processes of their own, and the growth of torch's peak allocation "
                   f"during the call; then the whole quantise phase of the default fit ({PHASE_STEPS} steps, an evaluation every "
                   f"{LOG_STEPS}, the conversion, one more evaluation) in a fresh process per run",
           "shapes": {}}
    for shape in SHAPES[:args.shapes]:
        tag = f"{shape[0]} {shape[1]}x{shape[2]}@{shape[3]}"
        r = res["shapes"][tag] = time_shape(trees, shape, args.repeats, args.warmup)
        print(json.dumps({tag: {k: (round(v["median_ms"], 3), round(v["min_ms"], 3), round(v["max_ms"], 3), v["torch_peak_growth_bytes"])
                                for k, v in r.items() if isinstance(v, dict)}, "accepted": r["accepted"],
                          "parent_over_head": round(r["parent_over_head"], 2)}), flush=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    r = res["quant_phase_of_the_default_fit"] = time_phase(trees, args.phase_runs)
    print(json.dumps({"phase": {k: round(v["median_ms"], 1) for k, v in r.items() if isinstance(v, dict)}, "accepted": r["accepted"],
                      "psnr_equal": r["psnr_equal"]}), flush=True)
    res["accepted"] = all(r["accepted"] for r in res["shapes"].values()) and res["quant_phase_of_the_default_fit"]["accepted"]
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0 if res["accepted"] else 1


if __name__ == "__main__":
    sys.exit(main())
