"""Child of tests/test_gpu_render.py: one render-path GPU case per process."""
import itertools
import os

import torch

from _gpu_child import ROOT, child_main
from _gpu_fixtures import golden, handle_memory, recorder, refused_training_calls, siren_params, u8_ref, working_calls
from oracle import siren_oracle as so

SHAPES = [(32, 3), (64, 4), (128, 6), (256, 8), (256, 2)]
SIZES = [(67, 45, 0), (256, 256, 0), (1031, 517, 65536)]      # (H, W, chunk_pixels): ragged last group; several chunks


def case_bitid():
    """sf_render(pred) on a render handle == sf_forward(pred) on a training handle, and rgb8 == the torch conversion of the
    kernel's own fp32 output, on every (shape, size, output layer, channels, operand type); once at the SIREN
    initialisation and once with the last layer scaled by 400 so that a linear output layer leaves [0, 1] on both sides"""
    from implicit_image._engine import RenderEngine, SirenEngine
    rows = []
    for (hid, dep), (H, W, chunk), lin, nout, dt in itertools.product(SHAPES, SIZES, (True, False), (3, 1), ("f16", "bf16")):
        tr = SirenEngine(H, W, hid, dep, outermost_linear=lin, out_features=nout, compute_dtype=dt, chunk_pixels=chunk)
        rn = RenderEngine(H, W, hid, dep, outermost_linear=lin, out_features=nout, compute_dtype=dt, chunk_pixels=chunk)
        gh, gw = so.grid_vectors(H, W)
        for e in (tr, rn):
            e.set_coords(gh.cuda(), gw.cuda())
        for scale in (1.0, 400.0):
            # (scaled set: zero output bias, so that 0.5 + 0.5 * scale * (W h) swings to both sides of [0, 1] in every channel)
            flat = siren_params(hid, dep, nout, seed=hid + dep, last_scale=scale,
                                bias_scale=1.0 if scale == 1.0 else 0.0).cuda()
            tr.set_params(flat)
            rn.set_params(flat)
            ref, _ = tr.forward(want_pred=True, want_sse=False)
            u8, pred = rn.render(want_u8=True, want_pred=True)
            u8_only, _ = rn.render(want_u8=True, want_pred=False)
            u8_tr, pred_tr = tr.render(want_u8=True, want_pred=True)       # the same kernel on a training handle
            torch.cuda.synchronize()
            rows.append(dict(hidden=hid, depth=dep, H=H, W=W, chunk=chunk, linear=lin, nout=nout, dtype=dt, scale=scale,
                             pred_equal=bool(torch.equal(pred, ref)), pred_equal_train_handle=bool(torch.equal(pred_tr, ref)),
                             finite=bool(torch.isfinite(ref).all()),
                             u8_equal=bool(torch.equal(u8, u8_ref(pred))), u8_only_equal=bool(torch.equal(u8_only, u8)),
                             u8_train_equal=bool(torch.equal(u8_tr, u8)),
                             below0=int((pred < 0).sum()), above1=int((pred > 1).sum()),
                             pmin=float(pred.min()), pmax=float(pred.max())))
        tr.close()
        rn.close()
    return {"cases": rows}


def container_flat():
    d = golden("container_64x4")
    sd = {k[len("decoded::"):]: torch.tensor(d[k]) for k in d.files if k.startswith("decoded::")}
    from implicit_image.decode import flat_params
    return sd, flat_params(sd, 4)


def case_oracle():
    """the 64x4 container fixture rendered at 64x64 against the fp64 oracle"""
    from implicit_image._engine import RenderEngine
    sd, flat = container_flat()
    H = W = 64
    eng = RenderEngine(H, W, 64, 4)
    gh, gw = so.grid_vectors(H, W)
    eng.set_coords(gh.cuda(), gw.cuda())
    eng.set_params(flat.cuda())
    u8, pred = eng.render(want_u8=True, want_pred=True)
    torch.cuda.synchronize()
    ref = so.forward([t.double() for t in so.unflatten(flat.numpy(), 64, 4)], so.get_grid(H, W).double()).reshape(H, W, 3)
    ref_u8 = torch.trunc(ref.double() * 255).clamp(0, 255)
    return {"max_abs": float((pred.cpu().double() - ref.double()).abs().max()),
            "max_levels": int((u8.cpu().double() - ref_u8).abs().max())}


def case_windows():
    """a window of a grid == the same region of the full render; a banded render == the one-band render"""
    from implicit_image.config import _wrap
    from implicit_image.decode import render_kernel
    sd, _ = container_flat()
    shape = _wrap({"mlp": {"name": "siren", "depth": 4, "hidden_size": 64, "first_omega_0": 50, "hidden_omega_0": 30,
                           "outermost_linear": True}, "engine": {}})
    rows, cols = torch.linspace(0, 1, 128), torch.linspace(0, 1, 128)
    full, fpred = render_kernel(sd, shape, rows, cols, want_pred=True)
    win, wpred = render_kernel(sd, shape, rows[32:96], cols[16:80], want_pred=True)
    band, bpred = render_kernel(sd, shape, rows, cols, band_rows=7, want_pred=True)
    return {"window_equal": bool(torch.equal(win, full[32:96, 16:80])), "window_pred_equal": bool(torch.equal(wpred, fpred[32:96, 16:80])),
            "band_equal": bool(torch.equal(band, full)), "band_pred_equal": bool(torch.equal(bpred, fpred)),
            "distinct_levels": int(full.unique().numel())}


def case_refuse():
    """argument checks only: every call below returns an error code before anything reaches the device"""
    import ctypes as C
    from implicit_image import _engine as E
    lib = E.load_library()
    eng = E.RenderEngine(64, 64, 64, 4)
    buf = torch.zeros(eng.num_params, device="cuda")
    out, rec = recorder(lib)
    refused_training_calls(rec, lib, eng, buf, feather_layers=4, render_to=None, set_target=False)
    rec("sf_render_both_null", lib.sf_render(eng.h, None, None))
    working_calls(rec, lib, eng, buf, offset_layer=1, set_and_count=False)
    rec("ok_sf_profile_enable", lib.sf_profile_enable(eng.h, 0))
    eng.close()
    cfg = E.sf_config(E.SF_ABI_VERSION, 64, 64, 0, 0, 2, 3, 512, 4, 50.0, 30.0, 1, 1, 0.9, 0.999, 1e-8, 0, None, 0, 0)
    h = C.c_void_p()
    rec("wide_create", lib.sf_render_create(C.byref(cfg), C.byref(h)))
    out["wide_handle_null"] = not bool(h.value)
    torch.cuda.synchronize()
    return out


def case_mem(kind):
    """device memory one 256x8 handle at 2048x2048 takes"""
    from implicit_image._engine import RenderEngine, SirenEngine
    taken, eng = handle_memory(lambda: (RenderEngine if kind == "render" else SirenEngine)(2048, 2048, 256, 8))
    out = {"taken": taken}
    if kind == "train":
        out["scratch"] = {k: int(eng.debug_scratch(k).numel()) for k in ("phases", "deltas", "dlast")}
    eng.close()
    return out


def case_e2e(workdir):
    """fit_one -> decode of the run directory, kernel path (masking none and RigL) and fallback path (mlp=fourier)"""
    from implicit_image import decode as dec
    from implicit_image._engine import SirenEngine
    from implicit_image.config import load_config
    from implicit_image.data import get_grid, read_ppm, synthetic_image
    from implicit_image.fit import fit_one
    from implicit_image.models import registry
    from implicit_image.pipeline import entropy_coding
    os.chdir(workdir)
    out = {}
    base = ["img.height=64", "img.width=64", "mlp.hidden_size=64", "mlp.depth=4", "train.num_steps=60", "train.log_steps=60",
            "quant=kmeans", "quant.num_steps=10", "quant.log_steps=10", "entropy_coding=plain"]
    for tag, extra in (("none", ["masking=none"]), ("rigl", ["masking=RigL", "masking.end_when=40", "masking.interval=20"])):
        cfg = load_config(os.path.join(ROOT, "conf"), base + extra)
        run = os.path.join(workdir, tag)
        res = fit_one(cfg, torch.device("cuda", 0), run)
        got = dec.decode([f"decode.dir={run}", "decode.truth=synthetic"])
        ppm = read_ppm(got["out"])
        # the existing engine forward for decompress_state_dict's weights
        sd = entropy_coding.decompress_state_dict(os.path.join(run, "model_quantized"), "plain")
        eng = SirenEngine(64, 64, 64, 4)
        gh, gw = so.grid_vectors(64, 64)
        eng.set_coords(gh.cuda(), gw.cuda())
        eng.set_params(dec.flat_params(sd, 4).cuda())
        pred, _ = eng.forward(want_pred=True, want_sse=False)
        torch.cuda.synchronize()
        pred = pred.cpu()
        ref_u8 = u8_ref(pred)
        img = synthetic_image(64, 64, int(cfg.img.seed))
        mse8 = (((img * 255).int() - ref_u8.int()) ** 2).float().mean()
        psnr8 = (10 * torch.log10(255 ** 2 / mse8)).item()
        out[tag] = {"path": got["path"], "source": got["source"], "ppm_equal": bool(torch.equal(ppm, ref_u8.int())),
                    "psnr8_decode": got["PSNR_8bit"], "psnr8_formula_on_bytes": psnr8, "psnr8_fit": float(res["Quant PSNR 8bit"]),
                    "outside_01": int(((pred < 0) | (pred > 1)).sum()),
                    "has_decode_json": os.path.exists(os.path.join(run, "decode.json"))}
        eng.close()
    cfg = load_config(os.path.join(ROOT, "conf"), ["mlp=fourier", "masking=none", "quant=none", "img.height=64", "img.width=64",
                                                   "mlp.hidden_size=64", "mlp.depth=4", "train.num_steps=60", "train.log_steps=60"])
    run = os.path.join(workdir, "fourier")
    fit_one(cfg, torch.device("cuda", 0), run)
    got = dec.decode([f"decode.dir={run}"])
    ppm = read_ppm(got["out"])
    sd = torch.load(os.path.join(run, "model.pth"), weights_only=True)["state_dict"]
    model = registry["fourier"](**cfg.mlp).cuda()
    model.load_state_dict(sd)
    model.eval()
    with torch.no_grad():
        pred = model(get_grid(64, 64).cuda()).cpu()
    out["fourier"] = {"path": got["path"], "source": got["source"], "shape": list(ppm.shape),
                      "ppm_equal": bool(torch.equal(ppm, u8_ref(pred).int()))}
    return out


if __name__ == "__main__":
    child_main({"bitid": case_bitid, "oracle": case_oracle, "windows": case_windows, "refuse": case_refuse, "mem": case_mem,
                "e2e": case_e2e})
