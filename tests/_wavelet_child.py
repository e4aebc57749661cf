"""Child of tests/test_gpu_wavelet.py: one WaveletSiren GPU case per process."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from _gpu_child import ROOT, child_main
from _gpu_fixtures import golden, relerr
import _wavelet_ref as wr
from oracle import siren_oracle as so  # (test infrastructure: grid and image formulas)

SMALL = dict(depth=4, hidden_size=64, first_omega_0=50.0, hidden_omega_0=30.0)
YAML = dict(depth=8, hidden_size=128, wavelet_levels=1, first_omega_0=50.0, hidden_omega_0=30.0, outermost_linear=True)


def model(seed=0, **kw):
    from implicit_image.models import registry
    torch.manual_seed(seed)
    return registry["wavelet_siren"](**kw).cuda()


def case_kernels():
    """k_wv_compose / k_wv_adjoint on random inputs against the fp64 mirror, and the dot-product identity of the adjoint"""
    from implicit_image._engine import WaveletEngine
    out = {}
    for H in (8, 64, 100, 256):
        n = wr.coeff_len(H)
        g = torch.Generator().manual_seed(H)
        lf, hf, img = (torch.rand(n, n, 3, generator=g), torch.rand(n, n, 3, generator=g), torch.rand(H, H, 3, generator=g))
        eng = WaveletEngine(H, H, 32, 2)
        pred, gy = eng.debug_compose(lf.cuda(), hf.cuda(), img.cuda())
        torch.cuda.synchronize()
        lf64, hf64 = lf.double(), hf.double()
        rgb64 = wr.compose(lf64, hf64, H, interp_dtype=torch.float32)
        d = (rgb64 - img.double()) * (2.0 / (3 * H * H))
        g64 = torch.stack([d[..., 0] + d[..., 1] + d[..., 2], 1.773 * d[..., 2] - 0.344 * d[..., 1],
                           1.403 * d[..., 0] - 0.714 * d[..., 1]], -1)
        # adjoint of (lf, hf) -> (Y, Cb, Cr) applied to the engine's own dL/d(Y, Cb, Cr)
        y = gy.cpu().double()
        a = lf64.clone().requires_grad_(True)
        b = hf64.clone().requires_grad_(True)
        Y = wr.idwt(a[..., 0][None, None], b.permute(2, 0, 1)[None, None])[0, 0]
        # (the upsampling in fp32, as the reference runs it: torch forms the source index and the weights in the input's
        #  type, and k_wv_compose follows that fp32 arithmetic; in fp64 the weights move by up to 5e-6 at H = 100)
        cbcr = F.interpolate(a.float()[..., 1:].permute(2, 0, 1)[None], scale_factor=H / n, mode="bilinear",
                             align_corners=False)[0].double()
        ax_y = (Y * y[..., 0]).sum() + (cbcr.permute(1, 2, 0) * y[..., 1:]).sum()
        da64, db64 = torch.autograd.grad(ax_y, (a, b))
        dlf, dhf = eng.debug_adjoint(gy.contiguous())
        dlf, dhf = dlf.cpu().double(), dhf.cpu().double()
        # <A x, y> with x = (lf, hf) against <x, A^T y> from the engine
        lhs = float(ax_y.detach())
        rhs = float((lf64 * dlf).sum() + (hf64 * dhf).sum())
        scale = float(Y.abs().sum() * y[..., 0].abs().max() + cbcr.abs().sum() * y[..., 1:].abs().max())
        out[f"H{H}"] = {"pred_rel": relerr(pred.cpu(), rgb64), "g_rel": relerr(gy.cpu(), g64),
                        "adj_lf_rel": relerr(dlf, da64), "adj_hf_rel": relerr(dhf, db64),
                        "dot_rel": abs(lhs - rhs) / scale}
        eng.close()
    return out


def case_parity():
    """seed-0 models on the 64x64 fixture image: prediction, loss and gradients against wavelet_grads.npz; the CPU
    generator's draws after the first forward against wavelet_init.npz"""
    g = golden("wavelet_grads")
    H = 64
    img, grid = so.synthetic_image(H, H, seed=5).cuda(), so.get_grid(H, H).cuda()
    out = {}
    for tag, kw in (("small", SMALL), ("yaml", YAML)):
        m = model(**kw)
        pred = m(grid)
        if tag == "small":
            out["draws_rel"] = relerr(torch.rand(8), golden("wavelet_init")["draws_after_forward"])
        sse = m.engine(grid, img).forward_backward()
        out[f"{tag}_pred_maxabs"] = float((pred.cpu() - torch.tensor(g[f"{tag}/pred"])).abs().max())
        ref = float(g[f"{tag}/loss"])
        out[f"{tag}_loss_rel"] = abs(sse / (3 * H * H) - ref) / ref
        names = [n for n, _ in m.named_parameters()]
        for n, p in zip(names, m._param_list()):
            if tag == "small":
                out[f"small_grad_rel/{n}"] = relerr(p.grad.cpu(), g[f"small/grad/{n}"])
            else:
                r = float(g[f"yaml/gradnorm/{n}"])
                out[f"yaml_gradnorm_rel/{n}"] = abs(p.grad.double().norm().item() - r) / r
    return out


def _fit(steps, bulk=True, replay=False, chunk_pixels=0, H=64, lr=1e-3, kw=SMALL):
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, train_epoch, train_steps
    img, grid = so.synthetic_image(H, H, seed=5).cuda(), so.get_grid(H, H).cuda()
    m = model(**kw, chunk_pixels=chunk_pixels)
    optim, sched = get_optimizer_lr_scheduler(m, dict(name="adam", lr=lr))
    if replay:
        m.engine(grid, img).set_graph_replay(True)
    if bulk:
        losses = train_steps(m, optim, grid, img, steps, lr_scheduler=sched)
    else:
        losses = [train_epoch(m, optim, grid, img, lr_scheduler=sched) for _ in range(steps)]
    params = m.engine(grid, img).get_params().cpu()
    # (train_epoch returns the loss as a Python float from the double SSE, sf_step as fp32: compared as fp32)
    return [float(np.float32(x)) for x in losses], params, m


def case_traj():
    """20 steps of Adam lr 1e-3 against wavelet_traj.npz (the reference's own train_epoch)"""
    g = golden("wavelet_traj")
    losses, _, m = _fit(20, bulk=False)
    ref = g["losses"]
    out = {"loss_rel": [abs(a - b) / b for a, b in zip(losses, ref)]}
    names = [n for n, _ in m.named_parameters()]
    # Adam moves an element by at most about lr per step whatever its gradient: elements with near-zero gradients follow
    # the sign of fp16 noise, so the parameters are compared against that step budget (lr * steps) as well
    out["param_rel"] = {n: relerr(p.detach().cpu(), g["final/" + n]) for n, p in zip(names, m._param_list())}
    out["param_maxabs_over_budget"] = max(float((p.detach().cpu() - torch.tensor(g["final/" + n])).abs().max())
                                          for n, p in zip(names, m._param_list())) / (float(g["lr"]) * int(g["steps"]))
    return out


def case_steps():
    """train_steps == step-by-step, run-to-run determinism, graph replay == eager: all bit-identical"""
    l1, p1, _ = _fit(20, bulk=False)
    l2, p2, _ = _fit(20, bulk=True)
    l3, p3, _ = _fit(20, bulk=True)
    l4, p4, _ = _fit(20, bulk=True, replay=True)
    eq = lambda a, b: bool(torch.equal(a, b))  # noqa: E731
    return {"eager_vs_bulk": [l1 == l2, eq(p1, p2)], "bulk_rerun": [l2 == l3, eq(p2, p3)],
            "replay_vs_eager": [l4 == l2, eq(p4, p2)], "loss_first_last": [l1[0], l1[-1]]}


def case_chunk():
    """forced small chunk_pixels (the two-pass path) against the single-chunk run, 64x64 (n^2 = 1156: two chunks of 1024)
    and 100x100 (n^2 = 2704: three)"""
    out = {}
    for H in (64, 100):
        l1, p1, _ = _fit(10, chunk_pixels=0, H=H)
        l2, p2, _ = _fit(10, chunk_pixels=1024, H=H)
        out[f"H{H}"] = {"loss_rel": max(abs(a - b) / b for a, b in zip(l2, l1)), "param_rel": relerr(p2, p1),
                        "first_loss_equal": l1[0] == l2[0]}
    return out


def case_padded():
    """Small_Dense density 0.5: hidden int(64 sqrt(.5)) = 45 runs zero-padded to 64; prediction / loss / gradients against
    the fp64 mirror; padded slots stay exactly 0 through training"""
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, train_epoch
    H = 64
    img, grid = so.synthetic_image(H, H, seed=3).cuda(), so.get_grid(H, H).cuda()
    m = model(depth=4, hidden_size=64, hidden_omega_0=30.0, small_dense_density=0.5)
    pred = m(grid)
    eng = m.engine(grid, img)
    sse = eng.forward_backward()
    m.download_grads()
    flat = wr.model_flat(m).cpu()
    rp, rl, rg = wr.loss_and_grads(flat, 45, 4, img.cpu(), 50.0, 30.0)
    got = torch.cat([p.grad.reshape(-1).cpu() for p in m._param_list()])
    out = {"hidden": m.cfg["hidden_size"], "width": m._engine_width, "pred_maxabs": float((pred.cpu() - rp).abs().max()),
           "loss_rel": abs(sse / (3 * H * H) - rl) / rl, "grad_rel": relerr(got, rg)}
    optim, sched = get_optimizer_lr_scheduler(m, dict(name="adam", lr=1e-3))
    for _ in range(5):
        train_epoch(m, optim, grid, img, lr_scheduler=sched)
    full = m.engine(grid, img).get_params()
    logical = torch.zeros_like(full, dtype=torch.bool)
    logical[m._padded_index(full.device)] = True
    out["padding_max"] = float(full[~logical].abs().max())
    out["n_padding"] = int((~logical).sum())
    return out


def case_plateau():
    """300 steps of the yaml model at lr 3e-4 on the 256x256 fixtures' images: final PSNR per image"""
    from implicit_image.utils.train_helper import eval_epoch, get_optimizer_lr_scheduler, train_steps
    S = 256
    grid = so.get_grid(S, S).cuda()
    out = {}
    for name, img in (("synthetic", so.synthetic_image(S, S, seed=5)), ("nonsmooth", so.nonsmooth_image(S, S))):
        img = img.cuda()
        m = model(**YAML)
        optim, sched = get_optimizer_lr_scheduler(m, dict(name="adam", lr=3e-4))
        losses = train_steps(m, optim, grid, img, 300, lr_scheduler=sched)
        _, loss, psnr, _ = eval_epoch(m, grid, img)
        out[name] = {"psnr": psnr, "losses": [float(x) for x in losses]}
    return out


def case_fit(workdir):
    """make fit KWARGS="mlp=wavelet_siren masking=none quant=none img.height=256 img.width=256 train.num_steps=300" through
    fit.fit_one"""
    from implicit_image.config import load_config
    from implicit_image.fit import fit_one
    os.chdir(workdir)
    cfg = load_config(os.path.join(ROOT, "conf"), ["mlp=wavelet_siren", "masking=none", "quant=none", "img.height=256",
                                                   "img.width=256", "train.num_steps=300"])
    out_dir = os.path.join(workdir, "out")
    res = fit_one(cfg, torch.device("cuda", 0), out_dir)
    sd = torch.load(os.path.join(out_dir, "model.pth"), weights_only=True)["state_dict"]
    return {"PSNR": res["PSNR"], "keys": list(sd), "finite": bool(all(torch.isfinite(v).all() for v in sd.values()))}


if __name__ == "__main__":
    child_main({"kernels": case_kernels, "parity": case_parity, "traj": case_traj, "steps": case_steps, "chunk": case_chunk,
                "padded": case_padded, "plateau": case_plateau, "fit": case_fit})
