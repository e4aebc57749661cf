"""Child of tests/test_gpu_wavelet_shapes.py: one WaveletSiren GPU case per process, at the widths, depths, output layers,
omegas, image sizes and chunkings the models of test_gpu_wavelet.py leave out.

Every comparison is on the engine's flat layout ([LF | HF] at the engine width, zero-padded when Small_Dense narrows the
model): the engine's own parameters go into the CPU references, so padded rows / columns are checked too."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from _gpu_child import ROOT, child_main
from _gpu_fixtures import relerr
import _wavelet_ref as wr
from oracle import siren_oracle as so  # (test infrastructure: grid and image formulas)

# tag -> (WaveletSiren kwargs, image side H): the table of tests/golden/make_golden_wavelet.py, which minted
# wavelet_shapes.npz from it
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
# two-pass cases: tag -> (model, image side H, chunk_pixels)
TWO_PASS = {
    "h64_d4_s100_c256": ("h64_d4", 100, 256),                      # 2704 coefficients: 11 chunks, the last of 144
    "h256_d4_s64_c1024": ("h256_d4", 64, 1024),                    # 1156: k_fwd_pipe inference + training feed the pass
    "h256_d4_sin_om_s48_c256": ("h256_d4_sin_om_s48", 48, 256),    # 676: sine output, dfac through k_wv_inject
}
MODELS = {"h64_d4": dict(depth=4, hidden_size=64, hidden_omega_0=30.0),
          "h256_d4": dict(depth=4, hidden_size=256, hidden_omega_0=30.0)}


def kwargs_of(tag):
    return SHAPES[tag][0] if tag in SHAPES else MODELS[tag]


def model(kw, seed=0, **extra):
    from implicit_image.models import registry
    torch.manual_seed(seed)
    return registry["wavelet_siren"](**kw, **extra).cuda()


def names_of(m):
    return [n for n, _ in m.named_parameters()]


def tensors(flat, m):
    """engine-layout flat vector -> [LF W0, b0, ..., HF W0, ...] (the order of named_parameters)"""
    lf, hf = wr.split_flat(flat, m._engine_width, m.cfg["depth"])
    return lf + hf


def omegas(m):
    c = m.cfg
    return c["first_omega_0"], c["hidden_omega_0"], c["outermost_linear"]


def engine_pass(m, grid, img):
    """eval forward (inference kernels), then a training pass: prediction, both SSEs, flat params and grads (CPU)"""
    eng = m.engine(grid, img)
    pred, sse_eval = eng.forward(want_pred=True, want_sse=True)
    sse_train = eng.forward_backward()
    torch.cuda.synchronize()
    return (pred.cpu().double(), sse_eval, sse_train, eng.get_params().cpu().clone(), eng.get_grads().cpu().double().clone())


def compare(m, img, pred, sse, params, grads):
    """engine against the rounding model and the fp64 mirror, on the engine's own parameters"""
    H = img.shape[0]
    fo, ho, lin = omegas(m)
    W, D = m._engine_width, m.cfg["depth"]
    pm, sm, gm = wr.engine_model_loss_and_grads(params, W, D, img.cpu(), fo, ho, lin)
    p64, l64, g64 = wr.loss_and_grads(params, W, D, img.cpu(), fo, ho, outermost_linear=lin)
    out = {"model_pred_maxabs": float((pred - pm).abs().max()), "model_sse_rel": abs(sse - sm) / sm,
           "fp64_pred_maxabs": float((pred - p64).abs().max()), "fp64_loss_rel": abs(sse / (3 * H * H) - l64) / l64,
           "model_grad_rel": {}, "fp64_grad_rel": {}}
    for n, e, a, b in zip(names_of(m), tensors(grads, m), tensors(gm, m), tensors(g64, m)):
        out["model_grad_rel"][n] = relerr(e, a)
        out["fp64_grad_rel"][n] = relerr(e, b)
    return out


def padded_mask(m):
    """flat engine-layout bool vector: True at the slots Small_Dense padding added"""
    logical = torch.zeros(2 * m._sub_engine_params(), dtype=torch.bool)
    logical[m._padded_index(torch.device("cpu"))] = True
    return ~logical


def padding_report(m, flat):
    """max |value| outside the logical (unpadded) entries of a flat engine vector (0.0 when not padded)"""
    if not m._padded:
        return 0.0
    return float(flat[padded_mask(m)].abs().max())


def case_shape(tag):
    """seed-0 model on synthetic_image(H, H, seed 5): engine vs rounding model, fp64 mirror and the reference fixture;
    eval vs training SSE; for padded widths, padding stays zero through 5 Adam steps"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "wavelet_shapes.npz"), allow_pickle=False)
    kw, H = SHAPES[tag]
    img, grid = so.synthetic_image(H, H, seed=5).cuda(), so.get_grid(H, H).cuda()
    m = model(kw)
    pred, sse_eval, sse_train, params, grads = engine_pass(m, grid, img)
    out = {"width": m._engine_width, "hidden": m.cfg["hidden_size"], "depth": m.cfg["depth"], "padded": m._padded,
           "sse_eval_eq_train": sse_eval == sse_train, "sse_eval_train": [sse_eval, sse_train]}
    out.update(compare(m, img, pred, sse_train, params, grads))
    ref_loss = float(g[f"{tag}/loss"])
    out["fixture_pred_maxabs"] = float((pred - torch.tensor(g[f"{tag}/pred"]).double()).abs().max())
    out["fixture_loss_rel"] = abs(sse_train / (3 * H * H) - ref_loss) / ref_loss
    assert [str(n) for n in g[f"{tag}/names"]] == names_of(m)
    out["fixture_gradnorm_rel"] = {}
    for n, e, ref in zip(names_of(m), tensors(grads, m), g[f"{tag}/gradnorm"]):
        out["fixture_gradnorm_rel"][n] = abs(e.norm().item() - float(ref)) / float(ref)
    if m._padded:
        from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, train_epoch
        out["pad_grad_max"] = padding_report(m, grads)
        out["grad_max"] = float(grads.abs().max())
        out["pad_grad_max_by_tensor"] = {}
        for n, e, pad in zip(names_of(m), tensors(grads, m), tensors(padded_mask(m), m)):
            if pad.any():
                out["pad_grad_max_by_tensor"][n] = float(e[pad].abs().max())
        optim, sched = get_optimizer_lr_scheduler(m, dict(name="adam", lr=1e-3))
        losses = [train_epoch(m, optim, grid, img, lr_scheduler=sched) for _ in range(5)]
        out["pad_param_max_after_5"] = padding_report(m, m.engine(grid, img).get_params().cpu())
        out["losses_first_last"] = [losses[0], losses[-1]]
    return out


def case_kernels(arg):
    """k_wv_compose / k_wv_adjoint at H = 2 (n = 3 > H: Cb / Cr down-sampled), 4 (bilinear scale exactly 1) and 6 on
    random inputs against the fp64 mirror, and <A x, y> = <x, A^T y> for the engine's adjoint (as test_gpu_wavelet.py's
    kernels case)"""
    from implicit_image._engine import WaveletEngine
    out = {}
    for H in (2, 4, 6):
        n = wr.coeff_len(H)
        gen = torch.Generator().manual_seed(H)
        lf, hf, img = (torch.rand(n, n, 3, generator=gen), torch.rand(n, n, 3, generator=gen),
                       torch.rand(H, H, 3, generator=gen))
        eng = WaveletEngine(H, H, 32, 2)
        pred, gy = eng.debug_compose(lf.cuda(), hf.cuda(), img.cuda())
        torch.cuda.synchronize()
        lf64, hf64 = lf.double(), hf.double()
        rgb64 = wr.compose(lf64, hf64, H, interp_dtype=torch.float32)
        d = (rgb64 - img.double()) * (2.0 / (3 * H * H))
        g64 = torch.stack([d[..., 0] + d[..., 1] + d[..., 2], 1.773 * d[..., 2] - 0.344 * d[..., 1],
                           1.403 * d[..., 0] - 0.714 * d[..., 1]], -1)
        y = gy.cpu().double()
        a = lf64.clone().requires_grad_(True)
        b = hf64.clone().requires_grad_(True)
        Y = wr.idwt(a[..., 0][None, None], b.permute(2, 0, 1)[None, None])[0, 0]
        cbcr = F.interpolate(a.float()[..., 1:].permute(2, 0, 1)[None], scale_factor=H / n, mode="bilinear",
                             align_corners=False)[0].double()
        ax_y = (Y * y[..., 0]).sum() + (cbcr.permute(1, 2, 0) * y[..., 1:]).sum()
        da64, db64 = torch.autograd.grad(ax_y, (a, b))
        dlf, dhf = eng.debug_adjoint(gy.contiguous())
        dlf, dhf = dlf.cpu().double(), dhf.cpu().double()
        lhs = float(ax_y.detach())
        rhs = float((lf64 * dlf).sum() + (hf64 * dhf).sum())
        scale = float(Y.abs().sum() * y[..., 0].abs().max() + cbcr.abs().sum() * y[..., 1:].abs().max())
        out[f"H{H}"] = {"pred_rel": relerr(pred.cpu(), rgb64), "g_rel": relerr(gy.cpu(), g64),
                        "adj_lf_rel": relerr(dlf, da64), "adj_hf_rel": relerr(dhf, db64),
                        "dot_rel": abs(lhs - rhs) / scale}
        eng.close()
    return out


def case_twopass(tag):
    """chunk_pixels small enough for the two-pass path, against the rounding model, the fp64 mirror and the one-chunk run"""
    mt, H, cp = TWO_PASS[tag]
    kw = kwargs_of(mt)
    img, grid = so.synthetic_image(H, H, seed=7).cuda(), so.get_grid(H, H).cuda()
    runs = {}
    for c in (0, cp):
        m = model(kw, chunk_pixels=c)
        runs[c] = engine_pass(m, grid, img)
    p0, se0, st0, w0, g0 = runs[0]
    pred, se, st, w, gr = runs[cp]
    n = wr.coeff_len(H)
    out = {"n2": n * n, "chunks": -(-n * n // cp), "params_equal": bool(torch.equal(w, w0)),
           "pred_bit_equal": bool(torch.equal(pred, p0)), "sse_eval_eq_train": se == st, "sse_equal_one_chunk": st == st0,
           "grad_rel_vs_one_chunk": max(relerr(a, b) for a, b in zip(tensors(gr, m), tensors(g0, m)))}
    c = compare(m, img, pred, st, w, gr)
    out.update({k: c[k] for k in ("model_pred_maxabs", "model_sse_rel", "fp64_pred_maxabs", "fp64_loss_rel")})
    out["model_grad_rel"] = max(c["model_grad_rel"].values())
    out["fp64_grad_rel"] = max(c["fp64_grad_rel"].values())
    return out


def case_natural(arg):
    """32x3 at 4096 x 4096, default chunking: n^2 = 4 202 500 coefficients take two chunks (4 Mi + 8196).  Gradients
    against the fp64 mirror (torch fp64 on the device); the engine's SSE (65 536 k_wv_compose partials through
    k_sse_reduce) against the fp64 sum over its own prediction"""
    H = 4096
    img, grid = so.synthetic_image(H, H, seed=5).cuda(), so.get_grid(H, H).cuda()
    m = model(SHAPES["h32_d3_s24"][0])
    eng = m.engine(grid, img)
    pred, sse_eval = eng.forward(want_pred=True, want_sse=True)
    sse_train = eng.forward_backward()
    torch.cuda.synchronize()
    params, grads = eng.get_params().clone(), eng.get_grads().double().cpu()
    own = float(((pred.double() - img.double()) ** 2).sum())
    del pred
    fo, ho, lin = omegas(m)
    p64, l64, g64 = wr.loss_and_grads(params, m._engine_width, m.cfg["depth"], img, fo, ho, outermost_linear=lin)
    g64 = g64.cpu()
    out = {"n2": wr.coeff_len(H) ** 2, "sse_eval_eq_train": sse_eval == sse_train, "sse_train": sse_train,
           "sse_own_fp64": own, "sse_rel_own": abs(sse_train - own) / own, "sse_eval_rel_own": abs(sse_eval - own) / own,
           "fp64_loss_rel": abs(sse_train / (3 * H * H) - l64) / l64, "fp64_grad_rel": {}}
    for n, e, b in zip(names_of(m), tensors(grads, m), tensors(g64, m)):
        out["fp64_grad_rel"][n] = relerr(e, b)
    return out


def case_replay(arg):
    """set_graph_replay(True) on a multi-chunk WaveletSiren (64x64, chunk 256: 1156 coefficients in five chunks): replay
    covers single-chunk fits only, so train_steps takes the eager path and must match it bit for bit"""
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, train_steps
    H = 64
    img, grid = so.synthetic_image(H, H, seed=5).cuda(), so.get_grid(H, H).cuda()
    res = []
    for replay in (False, True):
        m = model(MODELS["h64_d4"], chunk_pixels=256)
        optim, sched = get_optimizer_lr_scheduler(m, dict(name="adam", lr=1e-3))
        if replay:
            m.engine(grid, img).set_graph_replay(True)
        losses = train_steps(m, optim, grid, img, 10, lr_scheduler=sched)
        res.append(([float(x) for x in losses], m.engine(grid, img).get_params().cpu()))
    return {"losses_equal": res[0][0] == res[1][0], "params_equal": bool(torch.equal(res[0][1], res[1][1])),
            "losses": res[0][0]}


if __name__ == "__main__":
    child_main({"shape": case_shape, "kernels": case_kernels, "twopass": case_twopass, "natural": case_natural,
                "replay": case_replay})
