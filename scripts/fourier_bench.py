#!/usr/bin/env python3
"""FourierNet (conf/mlp/fourier.yaml: 128 x 8, map 256, scale 16) fit-step timing at 2048^2 and 4096^2: the engine
(sf_step, per-kernel table) beside the same model as plain torch on the same GPU (fp16 autocast, eager, Adam).
Prints one JSON line.

    python scripts/fourier_bench.py [--sizes 2048 4096] [--steps 10] [--torch-steps 5]

FLOPs per pixel-iteration (~6.3e5 at 128 x 8 / map 256): forward 2 P_w, backward data without layer 0, weight gradients."""
import argparse
import json
import math
import time

import torch
import torch.nn.functional as F
from _common import time_loop

from implicit_image.data import get_grid, synthetic_image
from implicit_image.models import registry

CFG = dict(depth=8, hidden_size=128, map_size=256, map_scale=16.0)
PEAK = 2.5e15   # dense fp16 MFMA, MI355X


def flops_per_pixel(hidden=128, n_linear=7, map_size=256, out=3):
    fwd = 2 * (map_size * hidden + (n_linear - 2) * hidden * hidden + hidden * out)
    bwd_data = 2 * ((n_linear - 2) * hidden * hidden + hidden * out)
    wgrad = fwd
    return fwd + bwd_data + wgrad


def time_engine(S, steps, warm=2):
    torch.manual_seed(0)
    m = registry["fourier"](**CFG).cuda()
    grid, img = get_grid(S, S).cuda(), synthetic_image(S, S, seed=5).cuda()
    eng = m.engine(grid, img)
    eng.step([3e-4] * warm)
    ms = time_loop(lambda: eng.step([3e-4] * steps), 1, "event") / steps
    eng.profile(True)
    eng.profile_reset()
    eng.step([3e-4] * 2)
    rep = {k: round(v["total_ms"] / 2, 3) for k, v in eng.profile_report().items() if v["launches"]}
    eng.profile(False)
    m._unbind()
    return ms, rep


class TorchFourier(torch.nn.Module):
    """the reference's FourierNet arithmetic as plain torch modules"""

    def __init__(self, src):
        super().__init__()
        self.B = torch.nn.Parameter(src.encoding.B.detach().clone(), requires_grad=False)
        lins = [torch.nn.Linear(l.in_features, l.out_features) for l in src.layers if isinstance(l, torch.nn.Linear)]
        with torch.no_grad():
            for a, b in zip(lins, [l for l in src.layers if isinstance(l, torch.nn.Linear)]):
                a.weight.copy_(b.weight)
                a.bias.copy_(b.bias)
        self.lins = torch.nn.ModuleList(lins)

    def forward(self, grid):
        h, w, _ = grid.shape
        x = (2 * math.pi * grid.reshape(-1, 2)) @ self.B
        x = torch.cat([torch.sin(x), torch.cos(x)], dim=-1)
        for i, l in enumerate(self.lins):
            x = l(x)
            x = torch.relu(x) if i < len(self.lins) - 1 else torch.sigmoid(x)
        return x.reshape(h, w, -1)


def time_torch(S, steps, warm=2):
    torch.manual_seed(0)
    m = TorchFourier(registry["fourier"](**CFG)).cuda()
    grid, img = get_grid(S, S).cuda(), synthetic_image(S, S, seed=5).cuda()
    opt = torch.optim.Adam(m.parameters(), lr=3e-4)

    def step():
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.float16):
            loss = F.mse_loss(m(grid).float(), img)
        loss.backward()
        opt.step()

    for _ in range(warm):
        step()
    ms = time_loop(step, steps, "event")
    del m, opt, grid, img
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--torch-steps", type=int, default=5)
    a = ap.parse_args()
    fpp = flops_per_pixel()
    out = {"bench": "fourier_fit_step", "model": "fourier 128x8 map256", "device": torch.cuda.get_device_name(0),
           "flops_per_pixel_iter": fpp, "peak_flops": PEAK, "sizes": {}}
    for S in a.sizes:
        px = S * S
        t0 = time.time()
        ms, rep = time_engine(S, a.steps)
        tms = time_torch(S, a.torch_steps)
        out["sizes"][str(S)] = {
            "engine_ms_per_step": round(ms, 3), "engine_mpix_it_per_s": round(px / ms / 1e3, 1),
            "engine_frac_peak": round(fpp * px / (ms * 1e-3) / PEAK, 4),
            "torch_fp16_eager_ms_per_step": round(tms, 3), "torch_mpix_it_per_s": round(px / tms / 1e3, 1),
            "speedup_vs_torch": round(tms / ms, 2), "engine_kernels_ms": rep, "wall_s": round(time.time() - t0, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
