#!/usr/bin/env python3
"""WaveletSiren (conf/mlp/wavelet_siren.yaml: 128x8, two sub-networks) fit-step time at 2048^2 and 4096^2 on one MI355X.

    python scripts/wavelet_bench.py [--sizes 2048 4096] [--steps 20] [--out profiles/wavelet_bench.json]

Per size: the engine's ms per training step (train_steps, one sf_step call), the per-kernel split from the engine's
profiler (k_wv_compose / k_wv_adjoint / k_wv_inject against the whole step), and in the same process torch eager fp32 and
fp16-autocast eager of the same model (the tests' torch mirror, tests/_wavelet_ref.py, with autograd and torch.optim.Adam).
"""
import argparse
import json
import os

import torch
import torch.nn.functional as F
from _common import ROOT, time_loop

YAML = dict(depth=8, hidden_size=128, wavelet_levels=1, first_omega_0=50.0, hidden_omega_0=30.0, outermost_linear=True)


def engine_leg(S, steps, warmup):
    from implicit_image.models import registry
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, train_steps
    from oracle import siren_oracle as so
    img, grid = so.synthetic_image(S, S, seed=5).cuda(), so.get_grid(S, S).cuda()
    torch.manual_seed(0)
    m = registry["wavelet_siren"](**YAML).cuda()
    optim, sched = get_optimizer_lr_scheduler(m, dict(name="adam", lr=3e-4))
    train_steps(m, optim, grid, img, warmup, lr_scheduler=sched)
    losses = []

    def timed_call():
        losses[:] = train_steps(m, optim, grid, img, steps, lr_scheduler=sched)
    ms = time_loop(timed_call, 1, "host") / steps
    eng = m.engine(grid, img)
    eng.profile(True)
    eng.profile_reset()
    train_steps(m, optim, grid, img, 5, lr_scheduler=sched)
    rep = {k: v for k, v in eng.profile_report().items() if v["launches"]}
    eng.profile(False)
    total = sum(v["total_ms"] for v in rep.values())
    wv = sum(v["total_ms"] for k, v in rep.items() if k.startswith("k_wv_"))
    two_pass = eng.n * eng.n > (1 << 22)
    del m, eng
    torch.cuda.empty_cache()
    return {"ms_per_step": ms, "loss_last": losses[-1], "coefficient_grid": (S + 5) // 2, "two_pass": two_pass,
            "profiled_steps": 5, "kernels": rep, "wv_ms_per_step": wv / 5, "wv_share_of_kernel_time": wv / total}


def torch_leg(S, steps, warmup, autocast):
    import _wavelet_ref as wr
    from oracle import siren_oracle as so
    n = wr.coeff_len(S)
    img = so.synthetic_image(S, S, seed=5).cuda()
    grid = so.get_grid(n, n).cuda()
    torch.manual_seed(0)
    from implicit_image.models import registry
    m = registry["wavelet_siren"](**YAML)
    flat = wr.model_flat(m).cuda().requires_grad_(True)
    opt = torch.optim.Adam([flat], lr=3e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            lfp, hfp = wr.split_flat(flat, 128, 8)
            lf = so.forward(lfp, grid, 50.0, 30.0)
            hf = so.forward(hfp, grid, 50.0, 30.0)
        rgb = wr.compose(lf.float(), hf.float(), S)
        loss = F.mse_loss(rgb, img)
        loss.backward()
        opt.step()

    for _ in range(warmup):
        step()
    ms = time_loop(step, steps, "host")
    del flat, opt
    torch.cuda.empty_cache()
    return {"ms_per_step": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavelet_bench.json"))
    args = ap.parse_args()
    res = {"model": "wavelet_siren 128x8 (conf/mlp/wavelet_siren.yaml), Adam lr 3e-4", "device": torch.cuda.get_device_name(0),
           "sizes": {}}
    for S in args.sizes:
        r = {"engine": engine_leg(S, args.steps, args.warmup)}
        for tag, ac in (("torch_fp32_eager", False), ("torch_fp16_autocast_eager", True)):
            try:
                r[tag] = torch_leg(S, args.torch_steps, 1, ac)
                r[tag]["engine_speedup"] = r[tag]["ms_per_step"] / r["engine"]["ms_per_step"]
            except Exception as e:   # (an out-of-memory torch leg is a result too)
                r[tag] = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
                torch.cuda.empty_cache()
        res["sizes"][str(S)] = r
        print(json.dumps({S: {k: v.get("ms_per_step", v.get("error")) for k, v in r.items()}}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res)[:2000])


if __name__ == "__main__":
    main()
