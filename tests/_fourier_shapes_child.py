"""Child of tests/test_gpu_fourier_shapes.py: one FourierNet GPU case per process, at the widths, map sizes, depths,
chunkings and grid sizes the fixture models of test_gpu_fourier.py leave out.

Every comparison is on the engine's flat layout (the engine width, zero-padded when Small_Dense narrows the model):
the engine's own parameters go into the CPU models, so padded rows / columns are checked too."""
import os

import numpy as np
import torch

from _gpu_child import ROOT, child_main
from _gpu_fixtures import relerr
import _fourier_ref as fr
from oracle import siren_oracle as so  # (test infrastructure: grid and image formulas)

# tag -> FourierNet kwargs (the table of tests/golden/make_golden_fourier.py, which minted fourier_shapes.npz from it)
SHAPES = {
    "h32_m64_d3": dict(depth=3, hidden_size=32, map_size=64, map_scale=10.0),
    "h45p_m512_d13": dict(depth=13, hidden_size=64, map_size=512, map_scale=10.0, small_dense_density=0.5),
    "h128_m512_d4": dict(depth=4, hidden_size=128, map_size=512, map_scale=10.0),
    "h256_m256_d4": dict(depth=4, hidden_size=256, map_size=256, map_scale=10.0),
    "h256_m512_d8": dict(depth=8, hidden_size=256, map_size=512, map_scale=16.0),
    "h198p_m64_d5": dict(depth=5, hidden_size=256, map_size=64, map_scale=10.0, small_dense_density=0.6),
}
FIX_HW = (24, 20)   # the fixture grid


def model(tag, seed=0, **extra):
    from implicit_image.models import registry
    torch.manual_seed(seed)
    return registry["fourier"](**SHAPES[tag], **extra).cuda()


def dims_of(m):
    return fr.layer_dims(m.cfg["n_linear"], m._engine_width, m.cfg["map_size"])


def names_of(m):
    return [f"layers.{2 * l}.{k}" for l in range(m.cfg["n_linear"]) for k in ("weight", "bias")]


def tensors(flat, dims):
    return [t for pair in fr.split_flat(flat, dims) for t in pair]


def engine_pass(m, grid, img):
    """eval forward (k_ff_fwd<WD, false>), then a training pass: prediction, both SSEs, flat params and grads (CPU)"""
    eng = m.engine(grid, img)
    pred, sse_eval = eng.forward(want_pred=True, want_sse=True)
    sse_train = eng.forward_backward()
    torch.cuda.synchronize()
    return (pred.cpu().double(), sse_eval, sse_train, eng.get_params().cpu().clone(), eng.get_grads().cpu().double().clone())


def compare(m, grid, img, pred, sse, params, grads):
    """engine against the rounding model and the fp64 mirror, on the engine's own parameters"""
    H, W, _ = grid.shape
    dims, B = dims_of(m), m.encoding.B.detach().cpu()
    pm, sm, gm = fr.engine_model_loss_and_grads(B, params, dims, grid.cpu(), img.cpu())
    p64, l64, g64 = fr.flat_loss_and_grads(B, params, dims, grid.cpu(), img.cpu())
    out = {"model_pred_maxabs": float((pred - pm).abs().max()), "model_sse_rel": abs(sse - sm) / sm,
           "fp64_pred_maxabs": float((pred - p64).abs().max()), "fp64_loss_rel": abs(sse / (3 * H * W) - l64) / l64,
           "model_grad_rel": {}, "fp64_grad_rel": {}}
    for n, e, a, b in zip(names_of(m), tensors(grads, dims), tensors(gm, dims), tensors(g64, dims)):
        out["model_grad_rel"][n] = relerr(e, a)
        out["fp64_grad_rel"][n] = relerr(e, b)
    return out


def padding_report(m, flat):
    """max |value| outside the logical (unpadded) entries of a flat engine vector (0.0 when not padded)"""
    if not m._padded:
        return 0.0
    logical = torch.zeros(flat.numel(), dtype=torch.bool)
    logical[m._padded_index(torch.device("cpu"))] = True
    return float(flat[~logical].abs().max())


def case_shape(tag):
    """seed-0 model on the 24x20 fixture grid: engine vs rounding model, fp64 mirror and the reference fixture; eval vs
    training SSE; for padded widths, padding stays zero through 10 Adam steps"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "fourier_shapes.npz"), allow_pickle=False)
    H, W = FIX_HW
    img, grid = so.synthetic_image(H, W, seed=5).cuda(), so.get_grid(H, W).cuda()
    m = model(tag)
    pred, sse_eval, sse_train, params, grads = engine_pass(m, grid, img)
    out = {"width": m._engine_width, "hidden": m.cfg["hidden_size"], "n_linear": m.cfg["n_linear"],
           "padded": m._padded, "sse_eval_eq_train": sse_eval == sse_train, "sse_eval_train": [sse_eval, sse_train]}
    out.update(compare(m, grid, img, pred, sse_train, params, grads))
    ref_loss = float(g[f"{tag}/loss"])
    out["fixture_pred_maxabs"] = float((pred - torch.tensor(g[f"{tag}/pred"]).double()).abs().max())
    out["fixture_loss_rel"] = abs(sse_train / (3 * H * W) - ref_loss) / ref_loss
    out["fixture_gradnorm_rel"] = {}
    for n, e in zip(names_of(m), tensors(grads, dims_of(m))):
        ref = float(g[f"{tag}/gradnorm/{n}"])
        out["fixture_gradnorm_rel"][n] = abs(e.norm().item() - ref) / ref
    if m._padded:
        from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, train_epoch
        out["pad_grad_max"] = padding_report(m, grads)
        optim, sched = get_optimizer_lr_scheduler(m, dict(name="adam", lr=1e-3))
        losses = [train_epoch(m, optim, grid, img, lr_scheduler=sched) for _ in range(10)]
        flat = m.engine(grid, img).get_params().cpu()
        out["pad_param_max_after_10"] = padding_report(m, flat)
        out["losses_first_last"] = [losses[0], losses[-1]]
    return out


def case_chunks(tag):
    """37x29 (1073 pixels) with chunk_pixels 0 (one chunk), 256 (five chunks, the last of 49 pixels) and 768 (768 + 305):
    chunked vs unchunked and each against the rounding model"""
    H, W = 37, 29
    img, grid = so.synthetic_image(H, W, seed=7).cuda(), so.get_grid(H, W).cuda()
    runs = {}
    for cp in (0, 256, 768):
        m = model(tag, chunk_pixels=cp)
        runs[cp] = engine_pass(m, grid, img)
    out = {}
    p0, se0, st0, w0, g0 = runs[0]
    for cp in (0, 256, 768):
        pred, se, st, w, gr = runs[cp]
        r = {"params_equal": bool(torch.equal(w, w0)), "pred_bit_equal": bool(torch.equal(pred, p0)),
             "sse_eval_eq_train": se == st, "sse_rel_vs_unchunked": abs(st - st0) / st0,
             "grad_rel_vs_unchunked": max(relerr(a, b) for a, b in zip(tensors(gr, dims_of(m)), tensors(g0, dims_of(m))))}
        c = compare(m, grid, img, pred, st, w, gr)
        r["model_pred_maxabs"], r["model_sse_rel"] = c["model_pred_maxabs"], c["model_sse_rel"]
        r["model_grad_rel"] = max(c["model_grad_rel"].values())
        r["fp64_grad_rel"] = max(c["fp64_grad_rel"].values())
        out[str(cp)] = r
    return out


def case_tiny(tag):
    """1x1, 1x300 and 300x1 grids (fewer than 256 pixels / a single row / a single column): model and fp64 mirror"""
    out = {}
    for H, W in ((1, 1), (1, 300), (300, 1)):
        img, grid = so.synthetic_image(H, W, seed=2).cuda(), so.get_grid(H, W).cuda()
        m = model(tag)
        pred, se, st, w, gr = engine_pass(m, grid, img)
        c = compare(m, grid, img, pred, st, w, gr)
        out[f"{H}x{W}"] = {"sse_eval_eq_train": se == st, "model_pred_maxabs": c["model_pred_maxabs"],
                           "model_sse_rel": c["model_sse_rel"], "model_grad_rel": max(c["model_grad_rel"].values()),
                           "fp64_pred_maxabs": c["fp64_pred_maxabs"], "fp64_loss_rel": c["fp64_loss_rel"],
                           "fp64_grad_rel": max(c["fp64_grad_rel"].values())}
    return out


def case_traj(tag):
    """20 train_epoch steps (engine Adam, lr 3e-4) against torch.optim.Adam on the fp64 mirror from the same init"""
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, train_epoch
    H, W = FIX_HW
    lr, steps = 3e-4, 20
    img, grid = so.synthetic_image(H, W, seed=5).cuda(), so.get_grid(H, W).cuda()
    m = model(tag)
    dims, B = dims_of(m), m.encoding.B.detach().cpu()
    flat0 = m.engine(grid, img).get_params().cpu().double()
    optim, sched = get_optimizer_lr_scheduler(m, dict(name="adam", lr=lr))
    losses = [float(train_epoch(m, optim, grid, img, lr_scheduler=sched)) for _ in range(steps)]
    p = flat0.clone().requires_grad_(True)
    ref_opt = torch.optim.Adam([p], lr=lr)
    ref = []
    for _ in range(steps):
        ref_opt.zero_grad()
        pred = fr.forward(B, fr.split_flat(p, dims), grid.cpu(), torch.float64)
        loss = torch.nn.functional.mse_loss(pred, img.cpu().double())
        loss.backward()
        ref.append(loss.item())
        ref_opt.step()
    rel = np.abs(np.array(losses) - np.array(ref)) / np.array(ref)
    return {"losses": losses, "ref": ref, "max_rel": float(rel.max()), "rel_first": float(rel[0])}


if __name__ == "__main__":
    child_main({"shape": case_shape, "chunks": case_chunks, "tiny": case_tiny, "traj": case_traj})
