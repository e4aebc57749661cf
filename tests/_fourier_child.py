"""Child of tests/test_gpu_fourier.py: one FourierNet GPU case per process."""
import os

import numpy as np
import torch

from _gpu_child import ROOT, child_main
from _gpu_fixtures import golden, relerr, sha
from oracle import siren_oracle as so  # (test infrastructure: grid and image formulas)

SMALL = dict(depth=4, hidden_size=64, map_size=128, map_scale=10.0)
YAML = dict(depth=8, hidden_size=128, map_size=256, map_scale=16.0)


def model(seed=0, **kw):
    from implicit_image.models import registry
    torch.manual_seed(seed)
    return registry["fourier"](**kw).cuda()


def case_parity():
    """forward and gradients of the seed-0 models against the reference on the ragged 48x40 grid"""
    g = golden("fourier_grads")
    H, W = 48, 40
    img, grid = so.synthetic_image(H, W, seed=5).cuda(), so.get_grid(H, W).cuda()
    out = {}
    for tag, kw in (("small", SMALL), ("yaml", YAML)):
        m = model(**kw)
        pred = m(grid)
        eng = m.engine(grid, img)
        sse = eng.forward_backward()
        out[f"{tag}_pred_maxabs"] = float((pred.cpu() - torch.tensor(g[f"{tag}/pred"])).abs().max())
        out[f"{tag}_loss_rel"] = abs(sse / (3 * H * W) - float(g[f"{tag}/loss"])) / float(g[f"{tag}/loss"])
        names = [n for n, p in m.named_parameters() if p.requires_grad]
        for n, p in zip(names, m._param_list()):
            if tag == "small":
                out[f"{tag}_grad_rel/{n}"] = relerr(p.grad.cpu(), g[f"{tag}/grad/{n}"])
            else:
                ref = float(g[f"{tag}/gradnorm/{n}"])
                out[f"{tag}_gradnorm_rel/{n}"] = abs(p.grad.double().norm().item() - ref) / ref
    return out


def _fit(steps, bulk, replay=False, seed=0):
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, train_epoch, train_steps
    H, W = 64, 56
    img, grid = so.synthetic_image(H, W, seed=3).cuda(), so.get_grid(H, W).cuda()
    m = model(seed, **SMALL)
    optim, sched = get_optimizer_lr_scheduler(m, dict(name="adam", lr=1e-3))
    if replay:
        m.engine(grid, img).set_graph_replay(True)
    if bulk:
        losses = train_steps(m, optim, grid, img, steps, lr_scheduler=sched)
    else:
        losses = [train_epoch(m, optim, grid, img, lr_scheduler=sched) for _ in range(steps)]
    torch.cuda.synchronize()
    # (train_epoch returns the loss as a Python float from the double SSE, sf_step as fp32: compared as fp32)
    return [float(np.float32(x)) for x in losses], sha(m.engine(grid, img).get_params())


def case_steps():
    """train_steps == step-by-step, run-to-run determinism, graph replay == eager: all bit-identical"""
    l1, p1 = _fit(20, bulk=False)
    l2, p2 = _fit(20, bulk=True)
    l3, p3 = _fit(20, bulk=True)
    l4, p4 = _fit(20, bulk=True, replay=True)
    return {"eager_vs_bulk": [l1 == l2, p1 == p2], "bulk_rerun": [l2 == l3, p2 == p3], "replay_vs_eager": [l4 == l2, p4 == p2],
            "loss_first_last": [l1[0], l1[-1]]}


def case_padded():
    """Small_Dense density 0.5: hidden int(128 sqrt(.5)) = 90 runs zero-padded to 128; pred / grads against the fp32 mirror"""
    import _fourier_ref as fr
    H, W = 40, 48
    img, grid = so.synthetic_image(H, W, seed=3).cuda(), so.get_grid(H, W).cuda()
    m = model(depth=5, hidden_size=128, map_size=128, map_scale=10.0, small_dense_density=0.5)
    pred = m(grid)
    eng = m.engine(grid, img)
    sse = eng.forward_backward()
    m.download_grads()
    rp, rl, rg = fr.loss_and_grads(m, grid, img)
    out = {"hidden": m.cfg["hidden_size"], "width": m._engine_width, "pred_maxabs": float((pred.cpu() - rp).abs().max()),
           "loss_rel": abs(sse / (3 * H * W) - rl) / rl,
           "grad_rel": max(relerr(p.grad.cpu(), r) for p, r in zip(m._param_list(), rg))}
    # padded neurons stay exactly zero through training
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, train_epoch
    optim, sched = get_optimizer_lr_scheduler(m, dict(name="adam", lr=1e-3))
    for _ in range(5):
        train_epoch(m, optim, grid, img, lr_scheduler=sched)
    flat = m.engine(grid, img).get_params()
    logical = torch.zeros_like(flat, dtype=torch.bool)
    logical[m._padded_index(flat.device)] = True
    out["padding_max"] = float(flat[~logical].abs().max())
    return out


def case_masks():
    """masks pushed through sf_set_masks hold the pruned weights at exactly 0 through Adam (sf_step)"""
    H, W = 48, 48
    img, grid = so.synthetic_image(H, W, seed=3).cuda(), so.get_grid(H, W).cuda()
    m = model(**SMALL)
    eng = m.engine(grid, img)
    g = torch.Generator().manual_seed(1)
    mask = (torch.rand(eng.num_params, generator=g) < 0.6).float().cuda()
    for l in range(m.cfg["n_linear"]):
        _, b = eng.param_offsets(l)
        n_out = 3 if l == m.cfg["n_linear"] - 1 else 64
        mask[b:b + n_out] = 1.0
    m.set_engine_masks(mask)
    with torch.no_grad():
        eng.view("params").mul_(mask)
    eng.params_changed()
    losses = eng.step([1e-3] * 10, want_loss=True)
    p = eng.get_params()
    return {"pruned_nonzero": int((p[mask == 0] != 0).sum()), "kept_nonzero": int((p[mask == 1] != 0).sum()),
            "n_pruned": int((mask == 0).sum()), "losses": [float(x) for x in losses]}


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
        out[name] = {"psnr": psnr, "losses": [float(x) for x in losses[::30]]}
    return out


def case_fit(workdir):
    """make fit mlp=fourier masking=none quant=kmeans entropy_coding=plain through fit.fit_one; the container decodes
    back to the saved (quantised) weights"""
    from implicit_image.config import load_config
    from implicit_image.fit import fit_one
    from implicit_image.pipeline import entropy_coding
    os.chdir(workdir)
    cfg = load_config(os.path.join(ROOT, "conf"), ["mlp=fourier", "masking=none", "quant=kmeans", "entropy_coding=plain",
                                                   "img.height=64", "img.width=64", "mlp.hidden_size=64", "mlp.depth=4",
                                                   "train.num_steps=200", "train.log_steps=100", "quant.num_steps=10",
                                                   "quant.log_steps=10"])
    out_dir = os.path.join(workdir, "out")
    res = fit_one(cfg, torch.device("cuda", 0), out_dir)
    sd = torch.load(os.path.join(out_dir, "model.pth"), weights_only=True)["state_dict"]
    dec = entropy_coding.decompress_state_dict(os.path.join(out_dir, "model_quantized"), "plain")
    return {"res": {k: float(v) for k, v in res.items()}, "keys": list(sd), "dec_keys": list(dec),
            "B_equal": bool(torch.equal(dec["encoding.B"], sd["encoding.B"].float().half().float())),
            "uniq": {k: int(v.unique().numel()) for k, v in dec.items() if k.endswith("weight")},
            "container_bytes": os.path.getsize(os.path.join(out_dir, "model_quantized", "compressed_weights.data"))}


if __name__ == "__main__":
    child_main({"parity": case_parity, "steps": case_steps, "padded": case_padded, "masks": case_masks,
                "plateau": case_plateau, "fit": case_fit})
