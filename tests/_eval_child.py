"""Child of tests/test_gpu_eval.py: sf_eval (eval_sums / sse8_view / eval_metrics) on every kernel family, one case per process.
The reference of every exactness case is the handle's own forward(): S = sum(((img * 255).int() - (pred * 255).int()) ** 2) in
int64 on the host side of the binding, and the double forward() reports."""
import ctypes as C
import json
import math
import os
import struct

import torch

from _gpu_child import ROOT, child_main
from _gpu_fixtures import fourier_params, launches, recorder, sha, siren_params, wavelet_params
from implicit_image import _engine as E
from oracle import siren_oracle as so

SENTINEL = -7


def bits(x):
    return struct.pack("<d", float(x)).hex()


def target(shape, seed):
    """fp32 targets in [0, 1]: every third value an exact k / 255, the first two 0 and 1"""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(shape, generator=g)
    flat = img.view(-1)
    flat[::3] = torch.randint(0, 256, (flat[::3].numel(),), generator=g).float() / 255.0
    flat[0], flat[1] = 0.0, 1.0
    return img.contiguous().cuda()


def check(eng, img):
    """the four assertions of one shape, as values the parent compares: img holds the handle's rows"""
    pred, sse = eng.forward()
    S = int((((img * 255).int() - (pred * 255).int()).long() ** 2).sum().item())
    e_sse, e_sse8 = eng.eval_sums()
    view8 = int(eng.sse8_view().item())
    eng.sse8_view().fill_(SENTINEL)
    eng.sse_view().fill_(float(SENTINEL))
    none = eng.eval_sums(sync=False)
    torch.cuda.synchronize()
    return {"S": S, "sse8": int(e_sse8), "view8": view8, "async8": int(eng.sse8_view().item()), "async_returns": list(none),
            "sse": bits(sse), "eval_sse": bits(e_sse), "async_sse": bits(eng.sse_view().item()),
            "below": int((pred < 0).sum()), "above": int((pred > 1).sum()), "npix": int(eng.npix)}


def siren(H, W, hidden, depth, nout=3, dtype="f16", last_scale=40.0, seed=0, **kw):
    eng = E.SirenEngine(H, W, hidden, depth, out_features=nout, compute_dtype=dtype, **kw)
    gh, gw = so.grid_vectors(H, W)
    eng.set_coords(gh.cuda(), gw.cuda())
    eng.set_params(siren_params(hidden, depth, nout, seed, last_scale, 0.0).cuda())
    return eng


def with_target(eng, img):
    rows = img[eng.row_begin:eng.row_end].contiguous()
    eng.set_target(rows)
    return check(eng, rows)


def case_k_fwd():
    """widths 32 and 64 at depth 3, both operand types, every out_features; 5x7: a partial 32-pixel block; 8x8: two whole
    blocks; 33x31 with chunk_pixels 256: four chunks, the last one 255 pixels"""
    out = {}
    for hidden in (32, 64):
        for dtype in ("f16", "bf16"):
            for (H, W, chunk) in ((5, 7, 0), (8, 8, 0), (33, 31, 256)):
                for nout in (1, 2, 3):
                    eng = siren(H, W, hidden, 3, nout, dtype, seed=hidden + nout, chunk_pixels=chunk)
                    out[f"{hidden}_{dtype}_{H}x{W}_{nout}"] = with_target(eng, target((H, W, nout), 11 * H + nout))
                    eng.close()
    return out


def case_k_fwd_pipe():
    """256x3: 9x7 (63 pixels, one short group), 64x48 (12 groups, two chunks of 2048 and 1024 pixels) and 300x301 - more
    256-pixel groups than the device has CUs, so a workgroup of the persistent kernel walks several"""
    out = {}
    for dtype in ("f16", "bf16"):
        for (H, W, chunk) in ((9, 7, 0), (64, 48, 2048), (300, 301, 0)):
            eng = siren(H, W, 256, 3, 3, dtype, seed=5, chunk_pixels=chunk)
            out[f"{dtype}_{H}x{W}"] = with_target(eng, target((H, W, 3), H))
            eng.close()
    return out


def case_wide():
    """512x3 on 9x7 and on 40x33 in two chunks (1024 + 296 pixels); out_features 2 on the small one"""
    out = {}
    for (H, W, chunk, nout, dtype) in ((9, 7, 0, 3, "f16"), (9, 7, 0, 2, "bf16"), (40, 33, 1024, 3, "f16"), (40, 33, 1024, 3, "bf16")):
        eng = siren(H, W, 512, 3, nout, dtype, last_scale=400.0, seed=7, chunk_pixels=chunk)
        out[f"{dtype}_{H}x{W}_{nout}"] = with_target(eng, target((H, W, nout), H + nout))
        eng.close()
    return out


def case_fourier():
    """hidden 32 / map 64 with 2 and 3 Linear layers on 5x7 and on 33x31 (chunk_pixels 256: four chunks, a short last one).
    The sigmoid stays inside (0, 1): truncation alone is exercised here"""
    out = {}
    for n_linear in (2, 3):
        for (H, W, chunk) in ((5, 7, 0), (33, 31, 256)):
            gen = torch.Generator().manual_seed(n_linear * 100 + H)
            eng = E.FourierEngine(H, W, 32, n_linear, 64, chunk_pixels=chunk)
            gh, gw = so.grid_vectors(H, W)
            eng.set_coords(gh.cuda(), gw.cuda())
            eng.set_encoding((torch.randn(2, 32, generator=gen) * 4.0).cuda())
            eng.set_params(fourier_params(32, n_linear, 64, gen).cuda())
            out[f"{n_linear}_{H}x{W}"] = with_target(eng, target((H, W, 3), H))
            eng.close()
    return out


def case_wavelet():
    """32x3 on 8x8 and 14x14 (single pass: 36 / 81 coefficients in one chunk) and on 30x30 with chunk_pixels 256 (289
    coefficients: two chunks, the two-pass route - no smaller even picture has more than one 256-pixel chunk)"""
    out = {}
    for (H, chunk) in ((8, 0), (14, 0), (30, 256)):
        eng = E.WaveletEngine(H, H, 32, 3, chunk_pixels=chunk)
        lin = torch.linspace(0, 1, eng.n).cuda()
        eng.set_coords(lin, lin)
        eng.set_params(wavelet_params(400.0, seed=H, rescale=True, depth=3, hidden_size=32, first_omega_0=50.0, hidden_omega_0=30.0).cuda())
        out[f"{H}_{chunk}"] = with_target(eng, target((H, H, 3), H))
        out[f"{H}_{chunk}"]["two_pass"] = bool(eng.n * eng.n > 256)
        eng.close()
    return out


def case_split():
    """rows [0, 3) and [3, 7) of 7x9 on two handles and the whole picture on a third: the integer sums add up exactly"""
    img = target((7, 9, 3), 3)
    out = {}
    for name, (r0, r1) in (("top", (0, 3)), ("bottom", (3, 7)), ("whole", (0, 7))):
        eng = siren(7, 9, 64, 3, seed=2, row_begin=r0, row_end=r1)
        out[name] = with_target(eng, img)
        eng.close()
    return out


def case_feather():
    """a 64x3 handle with Feathermap attached, its weights what the feather vector materialises to"""
    H, W = 9, 7
    eng = E.SirenEngine(H, W, 64, 3)
    gh, gw = so.grid_vectors(H, W)
    eng.set_coords(gh.cuda(), gw.cuda())
    eng.feather_attach(68, 8, [64, 64, 3], [2, 64, 64])                # 68^2 >= the 4547 parameters of 64x3
    v = eng.feather_view("params")
    v.copy_(torch.randn(v.numel(), generator=torch.Generator().manual_seed(2)).cuda() * 0.3)
    eng.feather_materialise()
    res = with_target(eng, target((H, W, 3), 5))
    eng.close()
    return {"feather": res}


# ---- nothing else moves ----------------------------------------------------------------------------------------------------
def case_state():
    """two handles from one seed, 4 single sf_step calls each, one of them with an sf_eval between every two: losses,
    parameters, moments, scratch bytes; then forward() after one more sf_eval on that handle against the other's"""
    H, W = 33, 31
    img = target((H, W, 3), 1)
    res = {}
    for name in ("plain", "with_eval"):
        eng = siren(H, W, 64, 4, seed=3, last_scale=1.0, chunk_pixels=512, scratch_format=16)
        eng.set_target(img)
        losses = []
        for i in range(4):
            if name == "with_eval" and i:
                eng.eval_sums() if i % 2 else eng.eval_sums(sync=False)
            losses += eng.step([3e-4], want_loss=True)
        m, v, step = eng.get_adam_state()
        scratch = {k: sha(eng.debug_scratch(k)) for k in ("phases", "deltas", "dlast", "slabs")}
        if name == "with_eval":
            eng.eval_sums()
        pred, sse = eng.forward()
        res[name] = {"losses": [bits(x) for x in losses], "params": sha(eng.get_params()), "m": sha(m), "v": sha(v), "step": int(step),
                     "scratch": scratch, "pred": sha(pred), "sse": bits(sse)}
        eng.close()
    return res


def _model(hidden=64, depth=4, side=32):
    from implicit_image.data import get_grid, synthetic_image
    from implicit_image.models import registry
    torch.manual_seed(0)
    m = registry["siren"](depth=depth, hidden_size=hidden, first_omega_0=50, hidden_omega_0=30).cuda()
    return m, get_grid(side, side).cuda(), synthetic_image(side, side, 3).cuda()


def case_metrics():
    """eval_metrics against eval_epoch on 64x4 at 32^2, and torch's allocator across the call"""
    from implicit_image.utils.train_helper import eval_epoch, eval_metrics
    m, grid, img = _model()
    pred, loss, psnr, psnr8 = eval_epoch(m, grid, img)
    S = int((((img * 255).int() - (pred * 255).int()).long() ** 2).sum().item())
    del pred
    eval_metrics(m, grid, img)                                        # (the first call allocates the handle's partial buffer)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    a0, p0 = torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()
    got = eval_metrics(m, grid, img)
    torch.cuda.synchronize()
    a1, p1 = torch.cuda.memory_allocated(), torch.cuda.max_memory_allocated()
    n = img.numel()
    return {"loss": [bits(loss), bits(got[0])], "psnr": [bits(psnr), bits(got[1])], "psnr8_epoch": psnr8, "psnr8": got[2],
            "psnr8_exact": bits(10 * math.log10(65025 / (S / n))), "psnr8_bits": bits(got[2]), "S": S, "n": n,
            "allocated": [a0, a1], "peak": [p0, p1]}


# ---- refusals --------------------------------------------------------------------------------------------------------------
def case_refuse():
    lib = E.load_library()
    out, rec = recorder(lib)
    sse, sse8 = C.c_double(), C.c_uint64()

    def call(name, eng):
        rec(name, lib.sf_eval(eng.h, C.byref(sse), C.byref(sse8)))

    lin8 = torch.linspace(0, 1, 8).cuda()
    renders = {"render_siren": E.RenderEngine(8, 8, 64, 3), "render_wide": E.WideRenderEngine(8, 8, 512, 3),
               "render_fourier": E.FourierRenderEngine(8, 8, 64, 3, 64), "render_wavelet": E.WaveletRenderEngine(8, 64, 3),
               "render_feather": E.FeatherRenderEngine(8, 8, 64, 3, 68, 8, [64, 64, 3], [2, 64, 64])}
    for name, eng in renders.items():
        eng.profile(True)
        call(name, eng)
        out["launches_" + name] = launches(eng)
        eng.close()
    img = torch.rand(8, 8, 3).cuda()
    eng = E.SirenEngine(8, 8, 64, 3)
    eng.profile(True)
    call("no_coords", eng)
    eng.set_coords(lin8, lin8)
    call("no_target", eng)
    out["launches_siren"] = launches(eng)
    eng.set_target(img)
    call("ok_siren", eng)
    eng.close()
    fou = E.FourierEngine(8, 8, 64, 3, 64)
    fou.profile(True)
    fou.set_coords(lin8, lin8)
    fou.set_target(img)
    call("no_encoding", fou)
    out["launches_fourier"] = launches(fou)
    fou.close()
    wv = E.WaveletEngine(8, 8, 64, 3)
    wv.profile(True)
    call("wavelet_no_coords", wv)
    lin = torch.linspace(0, 1, wv.n).cuda()
    wv.set_coords(lin, lin)
    call("wavelet_no_target", wv)
    out["launches_wavelet"] = launches(wv)
    wv.close()
    torch.cuda.synchronize()
    return out


# ---- whole fits ------------------------------------------------------------------------------------------------------------
def _fit(workdir, tag, overrides):
    from implicit_image import fit
    from implicit_image.config import load_config
    from implicit_image._engine import SirenEngine
    calls = {"forward_pred": 0, "eval_sums": 0}
    fwd, ev = SirenEngine.forward, SirenEngine.eval_sums

    def spy_forward(self, want_pred=True, want_sse=True):
        calls["forward_pred"] += bool(want_pred)
        return fwd(self, want_pred, want_sse)

    def spy_eval(self, sync=True):
        calls["eval_sums"] += 1
        return ev(self, sync)

    SirenEngine.forward, SirenEngine.eval_sums = spy_forward, spy_eval
    try:
        run = os.path.join(workdir, tag)
        res = fit.fit_one(load_config(os.path.join(ROOT, "conf"), overrides), torch.device("cuda", 0), run)
    finally:
        SirenEngine.forward, SirenEngine.eval_sums = fwd, ev
    saved = json.load(open(os.path.join(run, "result.json")))
    sd = torch.load(os.path.join(run, "model.pth"))["state_dict"]
    out = {"result": {k: (bits(v) if isinstance(v, float) else v) for k, v in saved.items() if k != "seconds"},
           "values": {k: float(v) for k, v in saved.items() if "8bit" in k},
           "returned_equal_saved": all(saved[k] == res[k] for k in saved if k != "seconds"),
           "model": {k: sha(v) for k, v in sd.items()}, "calls": calls}
    qdir = os.path.join(run, "model_quantized")
    if os.path.isdir(qdir):
        out["container"] = {f: open(os.path.join(qdir, f), "rb").read().hex() for f in sorted(os.listdir(qdir))}
    return out


COMMON = ["mlp.hidden_size=64", "mlp.depth=4", "img.height=32", "img.width=32", "train.num_steps=40", "train.log_steps=20"]


def case_fit_quant(workdir):
    base = COMMON + ["masking=none", "quant=kmeans", "quant.num_steps=20", "quant.log_steps=10", "entropy_coding=plain"]
    return {s: _fit(workdir, s, base + [f"train.device_eval={s}"]) for s in ("auto", "off")}


def case_fit_masked(workdir):
    base = COMMON + ["masking=RigL", "quant=none"]
    return {s: _fit(workdir, s, base + [f"train.device_eval={s}"]) for s in ("auto", "off")}


if __name__ == "__main__":
    child_main({"k_fwd": case_k_fwd, "k_fwd_pipe": case_k_fwd_pipe, "wide": case_wide, "fourier": case_fourier,
                "wavelet": case_wavelet, "split": case_split, "feather": case_feather, "state": case_state, "metrics": case_metrics,
                "refuse": case_refuse, "fit_quant": case_fit_quant, "fit_masked": case_fit_masked})
