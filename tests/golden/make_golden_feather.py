#!/usr/bin/env python3
"""Golden vectors for Feathermap (masking=Feathermap), minted by running the REAL reference on the CPU.

    python tests/golden/make_golden_feather.py [init] [grads] [traj] [plateau]

The reference's implicit_image/models/siren.py is imported by file path, its pipeline/feathermap/feathernet.py (with
feathermap/utils.py) through the reference package, and the fits use its own train_epoch (utils/train_helper.py:132-185),
with the stubs of make_golden_fourier.py.  compress = 0.2 (masking.density of conf/masking/Feathermap.yaml).  Data only:

  feather_init.npz     seed-0 init of FeatherNet(SIREN 64x4) (every state_dict tensor) and, for the conf/mlp/siren.yaml
                       model (128x8), each tensor's shape and sha256; n, m and the dense count of both
  feather_grads.npz    on a ragged 48x40 grid (oracle.synthetic_image seed 5): prediction, loss and every feather gradient
                       of the 64x4 model; prediction, loss and per-tensor gradient norms of the yaml model
  feather_traj.npz     64x4 model, 20 steps of train_epoch with Adam lr 1e-3 on the 48x40 image: the loss of every step
  feather_plateau.npz  64x4 model, 300 steps with Adam lr 3e-4 on the 256x256 synthetic_image (seed 5) and
                       nonsmooth_image: loss curve and final eval PSNR, with 8 and with 2 torch threads (the reference's own
                       run-to-run spread)
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
YAML = dict(depth=8, hidden_size=128, first_omega_0=50, hidden_omega_0=30, outermost_linear=True)
SMALL = dict(depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30, outermost_linear=True)
DENSITY = 0.2


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
    from implicit_image.pipeline.feathermap import feathernet
    spec = importlib.util.spec_from_file_location("ref_siren", f"{REF}/implicit_image/models/siren.py")
    siren = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(siren)
    sys.path.insert(0, ROOT)
    from oracle import siren_oracle as so
    return th, siren, feathernet, so


def model(siren, feathernet, seed, **kw):
    torch.manual_seed(seed)
    return feathernet.FeatherNet(siren.Siren(**kw), compress=DENSITY)


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().numpy().astype(np.float32)).tobytes()).hexdigest()


def make_init(siren, feathernet):
    out = {}
    m = model(siren, feathernet, 0, **SMALL)
    for n, p in m.state_dict().items():
        out["small/" + n] = p.numpy()
    out["small/nm"] = np.array([m._size_n, m._size_m, m.get_num_WandB()])
    names = []
    m = model(siren, feathernet, 0, **YAML)
    for n, p in m.state_dict().items():
        names.append(n)
        out["yaml_shape/" + n] = np.array(p.shape)
        out["yaml_sha/" + n] = np.array(sha(p))
    out["yaml_names"] = np.array(names)
    out["yaml/nm"] = np.array([m._size_n, m._size_m, m.get_num_WandB()])
    np.savez(os.path.join(OUT, "feather_init.npz"), **out)


def make_grads(siren, feathernet, so):
    H, W = 48, 40
    img, grid = so.synthetic_image(H, W, seed=5), so.get_grid(H, W)
    out = {}
    for tag, kw in (("small", SMALL), ("yaml", YAML)):
        m = model(siren, feathernet, 0, **kw)
        m.train()
        pred = m(grid)
        loss = F.mse_loss(pred, img)
        loss.backward()
        out[f"{tag}/pred"] = pred.detach().numpy()
        out[f"{tag}/loss"] = np.float64(loss.item())
        for n, p in m.named_parameters():
            if tag == "small":
                out[f"{tag}/grad/{n}"] = p.grad.numpy()
            else:
                out[f"{tag}/gradnorm/{n}"] = np.float64(p.grad.double().norm().item())
    np.savez(os.path.join(OUT, "feather_grads.npz"), **out)


def make_traj(th, siren, feathernet, so, steps=20):
    H, W = 48, 40
    img, grid = so.synthetic_image(H, W, seed=5), so.get_grid(H, W)
    m = model(siren, feathernet, 0, **SMALL)
    optim = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = [th.train_epoch(m, optim, grid, img) for _ in range(steps)]
    np.savez(os.path.join(OUT, "feather_traj.npz"), losses=np.array(losses, dtype=np.float64), lr=np.float64(1e-3))


def make_plateau(th, siren, feathernet, so, steps=300):
    S = 256
    grid = so.get_grid(S, S)
    out = {"steps": np.int64(steps), "lr": np.float64(3e-4)}
    for name, img in (("synthetic", so.synthetic_image(S, S, seed=5)), ("nonsmooth", so.nonsmooth_image(S, S))):
        for threads in (8, 2):
            torch.set_num_threads(threads)
            m = model(siren, feathernet, 0, **SMALL)
            optim = torch.optim.Adam(m.parameters(), lr=3e-4)
            losses = [th.train_epoch(m, optim, grid, img) for _ in range(steps)]
            m.eval()
            with torch.no_grad():
                mse = F.mse_loss(m(grid), img).item()
            out[f"{name}/t{threads}/losses"] = np.array(losses, dtype=np.float64)
            out[f"{name}/t{threads}/psnr"] = np.float64(10 * math.log10(1 / mse))
            print(name, threads, out[f"{name}/t{threads}/psnr"], flush=True)
    np.savez(os.path.join(OUT, "feather_plateau.npz"), **out)


def main():
    th, siren, feathernet, so = _ref()
    what = set(sys.argv[1:]) or {"init", "grads", "traj", "plateau"}
    torch.set_num_threads(8)
    if "init" in what:
        make_init(siren, feathernet)
    if "grads" in what:
        make_grads(siren, feathernet, so)
    if "traj" in what:
        make_traj(th, siren, feathernet, so)
    if "plateau" in what:
        make_plateau(th, siren, feathernet, so)


if __name__ == "__main__":
    main()
