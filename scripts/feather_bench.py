#!/usr/bin/env python3
"""Feathermap (masking=Feathermap, density 0.2) fit-step cost on the engine: ms per step of the same SIREN dense and with
the feather update (adjoint -> Adam on [V1 | V2 | scalers] -> materialise), in the same run, plus the per-kernel time of
the feather kernels (sf_profile_*) and, where it fits in memory, a torch fp32 eager FeatherNet (the tests' mirror).
Writes profiles/feather_bench.json and prints it.

    python scripts/feather_bench.py [--steps 10] [--out profiles/feather_bench.json]"""
import argparse
import json
import os

import torch
import torch.nn.functional as F
from _common import ROOT, time_loop

from implicit_image.data import get_grid, synthetic_image
from implicit_image.models.siren import Siren
from implicit_image.pipeline.feathermap import FeatherNet
from implicit_image.utils.train_helper import EngineAdam

SHAPES = [(256, 8, 4096, False), (1024, 12, 1024, False), (128, 8, 256, True)]   # hidden, depth, image edge, torch eager
KERNELS = ("k_feather_grad", "k_feather_dv", "k_feather_adam", "k_feather_mat")


def build(hidden, depth, feather):
    torch.manual_seed(0)
    # both at scratch format 16 (the Feathermap default), so the difference is the feather update alone
    m = Siren(depth=depth, hidden_size=hidden, first_omega_0=50, hidden_omega_0=30, scratch_format=16)
    return (FeatherNet(m, compress=0.2) if feather else m).cuda()


def time_engine(hidden, depth, S, feather, steps, grid, img):
    m = build(hidden, depth, feather)
    EngineAdam(m, lr=3e-4)
    eng = m.engine(grid, img)
    eng.step([3e-4] * 2)
    ms = time_loop(lambda: eng.step([3e-4] * steps), 1, "host") / steps
    eng.profile(True)
    eng.profile_reset()
    eng.step([3e-4] * 2)
    rep = eng.profile_report()
    eng.profile(False)
    kern = {k: round(v["total_ms"] * 1e3 / 2, 1) for k, v in rep.items() if k in KERNELS and v["launches"]}
    n_stored = m.num_stored() if feather else sum(p.numel() for p in m._param_list())
    del m, eng
    torch.cuda.empty_cache()
    return ms, kern, n_stored


def time_torch(hidden, depth, steps, grid, img):
    import _feather_ref as fr
    m = build(hidden, depth, True)
    ps = [p.detach().clone().requires_grad_(True) for p in m.parameters()]
    shp = fr.shapes(hidden, depth)
    from oracle import siren_oracle as so
    opt = torch.optim.Adam(ps, lr=3e-4)

    def step():
        opt.zero_grad()
        ws = fr.weights(ps[0], ps[1], [p.reshape(()) for p in ps[2:]], shp)
        F.mse_loss(so.forward(ws, grid), img).backward()
        opt.step()
    for _ in range(2):
        step()
    return time_loop(step, steps, "host")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feather_bench.json"))
    a = ap.parse_args()
    rows = []
    for hidden, depth, S, eager in SHAPES:
        grid, img = get_grid(S, S).cuda(), synthetic_image(S, S, seed=5).cuda()
        dense_ms, _, n_dense = time_engine(hidden, depth, S, False, a.steps, grid, img)
        fth_ms, kern, n_stored = time_engine(hidden, depth, S, True, a.steps, grid, img)
        row = {"siren": f"{hidden}x{depth}", "image": S, "dense_ms": round(dense_ms, 4), "feather_ms": round(fth_ms, 4),
               "overhead_pct": round(100 * (fth_ms - dense_ms) / dense_ms, 2),
               "added_us_per_step": round((fth_ms - dense_ms) * 1e3, 1), "feather_kernels_us": kern,
               "feather_kernels_us_total": round(sum(kern.values()), 1), "dense_params": n_dense, "stored": n_stored}
        if eager:
            row["torch_fp32_eager_ms"] = round(time_torch(hidden, depth, a.steps, grid, img), 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "density": 0.2, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
