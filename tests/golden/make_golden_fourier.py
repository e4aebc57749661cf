#!/usr/bin/env python3
"""Golden vectors for FourierNet (mlp=fourier), minted by running the REAL reference on the CPU.

    python tests/golden/make_golden_fourier.py [init] [grads] [plateau] [shapes]

The reference's implicit_image/models/fourier.py is imported by file path and trained with its own
train_epoch (utils/train_helper.py:132-185), with the stubs of make_golden_masking.py.  Data only:

  fourier_init.npz       seed-0 init of the 64x4 / map 128 model (every tensor, encoding.B included) and, for the
                         conf/mlp/fourier.yaml model (128x8 / map 256 / scale 16), each tensor's shape and sha256
  fourier_grads.npz      on a ragged 48x40 grid (oracle.synthetic_image seed 5): prediction, loss and every gradient of
                         the 64x4 model; prediction, loss and per-tensor gradient norms of the yaml model
  fourier_plateau.npz    yaml model, 300 steps of train_epoch with Adam lr 3e-4 on the 256x256 synthetic_image (seed 5)
                         and nonsmooth_image: loss curve and final eval PSNR, with 8 and with 2 torch threads (the
                         reference's own run-to-run spread)
  fourier_shapes.npz     for every model of SHAPES (the widths, map sizes, depths and Small_Dense paddings the two
                         models above leave out), seed 0: sha256 of every init tensor (pins the draw order), and on a
                         ragged 24x20 grid (synthetic_image seed 5) prediction, loss and per-tensor gradient norms
"""
import hashlib
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
YAML = dict(depth=8, hidden_size=128, map_size=256, map_scale=16.0)
SMALL = dict(depth=4, hidden_size=64, map_size=128, map_scale=10.0)
# tag -> FourierNet kwargs; tests/_fourier_shapes_child.py runs the same table on the engine
SHAPES = {
    "h32_m64_d3": dict(depth=3, hidden_size=32, map_size=64, map_scale=10.0),
    "h45p_m512_d13": dict(depth=13, hidden_size=64, map_size=512, map_scale=10.0, small_dense_density=0.5),
    "h128_m512_d4": dict(depth=4, hidden_size=128, map_size=512, map_scale=10.0),
    "h256_m256_d4": dict(depth=4, hidden_size=256, map_size=256, map_scale=10.0),
    "h256_m512_d8": dict(depth=8, hidden_size=256, map_size=512, map_scale=16.0),
    "h198p_m64_d5": dict(depth=5, hidden_size=256, map_size=64, map_scale=10.0, small_dense_density=0.6),
}


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m


def _ref():
    sys.path.insert(0, REF)
    _stub("omegaconf", DictConfig=dict, OmegaConf=object)
    _stub("torch_optimizer", Shampoo=object)
    from implicit_image.utils import train_helper as th
    spec = importlib.util.spec_from_file_location("ref_fourier", f"{REF}/implicit_image/models/fourier.py")
    fourier = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fourier)
    sys.path.insert(0, ROOT)
    from oracle import siren_oracle as so
    return th, fourier, so


def model(fourier, seed, **kw):
    torch.manual_seed(seed)
    return fourier.FourierNet(**kw)


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().numpy().astype(np.float32)).tobytes()).hexdigest()


def make_init(fourier):
    out = {}
    for n, p in model(fourier, 0, **SMALL).state_dict().items():
        out["small/" + n] = p.numpy()
    names = []
    for n, p in model(fourier, 0, **YAML).state_dict().items():
        names.append(n)
        out["yaml_shape/" + n] = np.array(p.shape)
        out["yaml_sha/" + n] = np.array(sha(p))
    out["yaml_names"] = np.array(names)
    np.savez(os.path.join(OUT, "fourier_init.npz"), **out)


def make_grads(fourier, so):
    H, W = 48, 40
    img, grid = so.synthetic_image(H, W, seed=5), so.get_grid(H, W)
    out = {}
    for tag, kw in (("small", SMALL), ("yaml", YAML)):
        m = model(fourier, 0, **kw)
        pred = m(grid)
        loss = F.mse_loss(pred, img)
        loss.backward()
        out[f"{tag}/pred"] = pred.detach().numpy()
        out[f"{tag}/loss"] = np.float64(loss.item())
        for n, p in m.named_parameters():
            if p.grad is None:
                continue
            if tag == "small":
                out[f"{tag}/grad/{n}"] = p.grad.numpy()
            else:
                out[f"{tag}/gradnorm/{n}"] = np.float64(p.grad.double().norm().item())
    np.savez(os.path.join(OUT, "fourier_grads.npz"), **out)


def make_shapes(fourier, so):
    H, W = 24, 20
    img, grid = so.synthetic_image(H, W, seed=5), so.get_grid(H, W)
    out = {"tags": np.array(list(SHAPES))}
    for tag, kw in SHAPES.items():
        m = model(fourier, 0, **kw)
        for n, p in m.state_dict().items():
            out[f"{tag}/sha/{n}"] = np.array(sha(p))
        out[f"{tag}/names"] = np.array(list(m.state_dict()))
        pred = m(grid)
        loss = F.mse_loss(pred, img)
        loss.backward()
        out[f"{tag}/pred"] = pred.detach().numpy()
        out[f"{tag}/loss"] = np.float64(loss.item())
        for n, p in m.named_parameters():
            if p.grad is not None:
                out[f"{tag}/gradnorm/{n}"] = np.float64(p.grad.double().norm().item())
    np.savez_compressed(os.path.join(OUT, "fourier_shapes.npz"), **out)


def make_plateau(th, fourier, so, steps=300):
    S = 256
    grid = so.get_grid(S, S)
    out = {"steps": np.int64(steps), "lr": np.float64(3e-4)}
    for name, img in (("synthetic", so.synthetic_image(S, S, seed=5)), ("nonsmooth", so.nonsmooth_image(S, S))):
        for threads in (8, 2):
            torch.set_num_threads(threads)
            m = model(fourier, 0, **YAML)
            optim = torch.optim.Adam(m.parameters(), lr=3e-4)
            losses = [th.train_epoch(m, optim, grid, img) for _ in range(steps)]
            with torch.no_grad():
                mse = F.mse_loss(m(grid), img).item()
            out[f"{name}/t{threads}/losses"] = np.array(losses, dtype=np.float64)
            out[f"{name}/t{threads}/psnr"] = np.float64(10 * math.log10(1 / mse))
            print(name, threads, out[f"{name}/t{threads}/psnr"], flush=True)
    np.savez(os.path.join(OUT, "fourier_plateau.npz"), **out)


def main():
    th, fourier, so = _ref()
    what = set(sys.argv[1:]) or {"init", "grads", "plateau", "shapes"}
    torch.set_num_threads(8)
    if "init" in what:
        make_init(fourier)
    if "grads" in what:
        make_grads(fourier, so)
    if "shapes" in what:
        make_shapes(fourier, so)
    if "plateau" in what:
        make_plateau(th, fourier, so)


if __name__ == "__main__":
    main()
