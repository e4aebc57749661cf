#!/usr/bin/env python3
"""Golden vectors for WaveletSiren (mlp=wavelet_siren).

    python tests/golden/make_golden_wavelet.py [idwt] [bilinear] [init] [grads] [traj] [plateau] [shapes]

  wavelet_idwt.npz       PyWavelets 1.1.1 (run as a separate interpreter that has pywt, `pywt` mode of this script): db3
                         rec_lo / rec_hi and idwt2(mode="zero") of random coefficient sets at n = 6, 34, 52, 130 (fp32 inputs;
                         the n = 130 output rounded to fp32), plus one set
                         per detail band with only that band non-zero (pins pytorch_wavelets' (LH, HL, HH) = pywt's
                         (cH, cV, cD))
  wavelet_bilinear.npz   the real F.interpolate(scale_factor=H/n, bilinear, align_corners=False) at H = 8, 64, 100, 256,
                         1024 on inputs drawn from torch.Generator seeded with H (full output up to H = 100, rows
                         0..3, H/2 and H-4..H-1 above)

The reference's implicit_image/models/wavelet_siren.py and siren.py are imported by file path, with the stubs of
tests/_wavelet_ref.py for pytorch_wavelets and kornia, and trained with its own train_epoch.  Data only:

  wavelet_init.npz       seed-0 init of the 64x4 model (every tensor) and the sha256 of every tensor of the conf/mlp yaml
                         model (128x8); the CPU generator's next 8 draws after the first forward
  wavelet_grads.npz      64x64 synthetic_image (seed 5): prediction, loss and every gradient of the small model; prediction,
                         loss and per-tensor gradient norms of the yaml model
  wavelet_traj.npz       small model, 20 steps of train_epoch with Adam lr 1e-3 on that image: losses and final parameters
  wavelet_plateau.npz    yaml model, 300 steps of train_epoch with Adam lr 3e-4 on the 256x256 synthetic_image (seed 5) and
                         nonsmooth_image: loss curve and final eval PSNR, with 8 and with 2 torch threads
  wavelet_shapes.npz     for every model of SHAPES (the widths, depths, output layers, omegas, Small_Dense padding and
                         image sizes the models above leave out: every sub-network kernel path, a sine output layer,
                         first / hidden omega 30 / 50, H = 2 / 4 / 6), seed 0: sha256 of every init tensor, and on
                         synthetic_image(H, H, seed 5) the prediction, the loss and per-tensor gradient norms (sha and
                         norms in the order of the names).  Not in the
                         default set: `python tests/golden/make_golden_wavelet.py shapes`
"""
import hashlib
import importlib.util
import math
import os
import subprocess
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
PYWT_PYTHON = os.environ.get("PYWT_PYTHON", "python3")   # an interpreter with numpy + PyWavelets
SMALL = dict(depth=4, hidden_size=64, first_omega_0=50.0, hidden_omega_0=30.0)
YAML = dict(depth=8, hidden_size=128, wavelet_levels=1, first_omega_0=50.0, hidden_omega_0=30.0, outermost_linear=True,
            simulate_quantization=False)
# tag -> (WaveletSiren kwargs, image side H); tests/_wavelet_shapes_child.py runs the same table on the engine
SHAPES = {
    "h32_d3_s24": (dict(depth=3, hidden_size=32, hidden_omega_0=30.0), 24),
    "h64_d2_s10": (dict(depth=2, hidden_size=64, hidden_omega_0=30.0), 10),
    "h128_d5_sin_s40": (dict(depth=5, hidden_size=128, hidden_omega_0=30.0, outermost_linear=False), 40),
    "h256_d2_s30": (dict(depth=2, hidden_size=256, hidden_omega_0=30.0), 30),
    "h256_d6_s64": (dict(depth=6, hidden_size=256, hidden_omega_0=30.0), 64),
    "h256_d4_sin_om_s48": (dict(depth=4, hidden_size=256, first_omega_0=30.0, hidden_omega_0=50.0, outermost_linear=False),
                           48),
    "h181p_d4_s48": (dict(depth=4, hidden_size=256, hidden_omega_0=30.0, small_dense_density=0.5), 48),
    "h32_d16_s20": (dict(depth=16, hidden_size=32, hidden_omega_0=30.0), 20),
    "h64_d3_s2": (dict(depth=3, hidden_size=64, hidden_omega_0=30.0), 2),
    "h64_d3_s4": (dict(depth=3, hidden_size=64, hidden_omega_0=30.0), 4),
    "h64_d3_s6": (dict(depth=3, hidden_size=64, hidden_omega_0=30.0), 6),
}


def make_pywt():   # runs under an interpreter with numpy + pywt (no torch)
    import pywt
    w = pywt.Wavelet("db3")
    out = {"rec_lo": np.array(w.rec_lo), "rec_hi": np.array(w.rec_hi), "ns": np.array([6, 34, 52, 130])}
    rng = np.random.default_rng(0)
    for n in (6, 34, 52, 130):
        # fp32-representable inputs, stored as fp32; the n = 130 output too (the file stays under 1 MiB)
        cA, cH, cV, cD = (rng.standard_normal((n, n)).astype(np.float32) for _ in range(4))
        out[f"n{n}/cA"], out[f"n{n}/cH"], out[f"n{n}/cV"], out[f"n{n}/cD"] = cA, cH, cV, cD
        y = pywt.idwt2(tuple(np.float64(c) for c in (cA,)) + ((np.float64(cH), np.float64(cV), np.float64(cD)),), "db3",
                       mode="zero")
        out[f"n{n}/y"] = y.astype(np.float32) if n > 100 else y
    n = 6
    for band in ("cH", "cV", "cD"):
        c = {k: np.zeros((n, n)) for k in ("cA", "cH", "cV", "cD")}
        c[band] = rng.standard_normal((n, n))
        out[f"band_{band}/in"] = c[band]
        out[f"band_{band}/y"] = pywt.idwt2((c["cA"], (c["cH"], c["cV"], c["cD"])), "db3", mode="zero")
    np.savez(os.path.join(OUT, "wavelet_idwt.npz"), **out)


def bilinear_input(H):
    import torch
    from _wavelet_ref import coeff_len
    n = coeff_len(H)
    return torch.rand(1, 2, n, n, generator=torch.Generator().manual_seed(H))


def bilinear_rows(H):
    return np.arange(H) if H <= 100 else np.array([0, 1, 2, 3, H // 2, H - 4, H - 3, H - 2, H - 1])


def make_bilinear():
    import torch.nn.functional as F
    from _wavelet_ref import coeff_len
    out = {"Hs": np.array([8, 64, 100, 256, 1024])}
    for H in (8, 64, 100, 256, 1024):
        x = bilinear_input(H)
        y = F.interpolate(x, scale_factor=H / coeff_len(H), mode="bilinear", align_corners=False)
        assert y.shape[-1] == H
        rows = bilinear_rows(H)
        out[f"H{H}/rows"] = rows
        out[f"H{H}/y"] = y[0][:, rows].numpy()
    np.savez(os.path.join(OUT, "wavelet_bilinear.npz"), **out)


def _ref():
    import _wavelet_ref as wr
    wr.install_stubs()
    sys.path.insert(0, REF)
    for name in ("omegaconf", "torch_optimizer"):
        m = types.ModuleType(name)
        m.DictConfig, m.OmegaConf, m.Shampoo = dict, object, object
        sys.modules[name] = m
    from implicit_image.utils import train_helper as th
    spec = importlib.util.spec_from_file_location("ref_wavelet_siren", f"{REF}/implicit_image/models/wavelet_siren.py")
    ws = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ws)
    from oracle import siren_oracle as so
    return th, ws, so


def model(ws, seed, **kw):
    import torch
    torch.manual_seed(seed)
    return ws.WaveletSiren(**kw)


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().numpy().astype(np.float32)).tobytes()).hexdigest()


def make_init(ws, so):
    import torch
    out = {}
    m = model(ws, 0, **SMALL)
    for n, p in m.named_parameters():
        out["small/" + n] = p.detach().numpy()
    out["small_names"] = np.array([n for n, _ in m.named_parameters()])
    m(so.get_grid(64, 64))
    out["draws_after_forward"] = torch.rand(8).numpy()
    y = model(ws, 0, **YAML)
    out["yaml_names"] = np.array([n for n, _ in y.named_parameters()])
    for n, p in y.named_parameters():
        out["yaml_shape/" + n] = np.array(p.shape)
        out["yaml_sha/" + n] = np.array(sha(p))
    np.savez(os.path.join(OUT, "wavelet_init.npz"), **out)


def make_grads(ws, so):
    import torch.nn.functional as F
    H = 64
    img, grid = so.synthetic_image(H, H, seed=5), so.get_grid(H, H)
    out = {}
    for tag, kw in (("small", SMALL), ("yaml", YAML)):
        m = model(ws, 0, **kw)
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
    np.savez(os.path.join(OUT, "wavelet_grads.npz"), **out)


def make_traj(th, ws, so, steps=20):
    import torch
    H = 64
    img, grid = so.synthetic_image(H, H, seed=5), so.get_grid(H, H)
    m = model(ws, 0, **SMALL)
    optim = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = [th.train_epoch(m, optim, grid, img) for _ in range(steps)]
    out = {"losses": np.array(losses, dtype=np.float64), "lr": np.float64(1e-3), "steps": np.int64(steps)}
    for n, p in m.named_parameters():
        out["final/" + n] = p.detach().numpy()
    np.savez(os.path.join(OUT, "wavelet_traj.npz"), **out)


def make_plateau(th, ws, so, steps=300):
    import torch
    import torch.nn.functional as F
    S = 256
    grid = so.get_grid(S, S)
    out = {"steps": np.int64(steps), "lr": np.float64(3e-4)}
    for name, img in (("synthetic", so.synthetic_image(S, S, seed=5)), ("nonsmooth", so.nonsmooth_image(S, S))):
        for threads in (8, 2):
            torch.set_num_threads(threads)
            m = model(ws, 0, **YAML)
            optim = torch.optim.Adam(m.parameters(), lr=3e-4)
            losses = [th.train_epoch(m, optim, grid, img) for _ in range(steps)]
            with torch.no_grad():
                mse = F.mse_loss(m(grid), img).item()
            out[f"{name}/t{threads}/losses"] = np.array(losses, dtype=np.float64)
            out[f"{name}/t{threads}/psnr"] = np.float64(10 * math.log10(1 / mse))
            print(name, threads, out[f"{name}/t{threads}/psnr"], flush=True)
    np.savez(os.path.join(OUT, "wavelet_plateau.npz"), **out)


def make_shapes(ws, so):
    import torch.nn.functional as F
    out = {"tags": np.array(list(SHAPES))}
    for tag, (kw, H) in SHAPES.items():
        img, grid = so.synthetic_image(H, H, seed=5), so.get_grid(H, H)
        m = model(ws, 0, **kw)
        names = [n for n, _ in m.named_parameters()]
        out[f"{tag}/names"] = np.array(names)
        out[f"{tag}/sha"] = np.array([sha(p) for _, p in m.named_parameters()], dtype="S64")
        pred = m(grid)
        loss = F.mse_loss(pred, img)
        loss.backward()
        out[f"{tag}/pred"] = pred.detach().numpy()
        out[f"{tag}/loss"] = np.float64(loss.item())
        out[f"{tag}/gradnorm"] = np.array([p.grad.double().norm().item() for _, p in m.named_parameters()])
    np.savez_compressed(os.path.join(OUT, "wavelet_shapes.npz"), **out)


def main():
    what = set(sys.argv[1:]) or {"idwt", "bilinear", "init", "grads", "traj", "plateau"}
    if what == {"pywt"}:
        return make_pywt()
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    if "idwt" in what:
        subprocess.check_call([PYWT_PYTHON, os.path.abspath(__file__), "pywt"])
    import torch
    torch.set_num_threads(8)
    if "bilinear" in what:
        make_bilinear()
    if what & {"init", "grads", "traj", "plateau", "shapes"}:
        th, ws, so = _ref()
        if "init" in what:
            make_init(ws, so)
        if "grads" in what:
            make_grads(ws, so)
        if "traj" in what:
            make_traj(th, ws, so)
        if "plateau" in what:
            make_plateau(th, ws, so)
        if "shapes" in what:
            make_shapes(ws, so)


if __name__ == "__main__":
    main()
