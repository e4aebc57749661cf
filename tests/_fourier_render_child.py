"""Child of tests/test_gpu_fourier_render.py: one FourierNet render-path GPU case per process."""
import itertools
import os

import torch

from _gpu_child import ROOT, child_main
from _gpu_fixtures import (Guarded, fourier_params, handle_memory, launches, recorder, refused_training_calls,
                           working_calls)

HIDDEN = (32, 64, 128, 256)
MAPS = (64, 512)
EXTRA_MAPS_AT = (128, (128, 256))                    # the other two map sizes, at one width
N_LINEAR = (2, 3, 5)
PICTURES = ((1, 1), (5, 7), (33, 31), (64, 64), (37, 300))
CHUNKS = (0, 256)
MAP_SCALE = 16.0
GUARD = 16


def shapes():
    hm = [(h, ms) for h in HIDDEN for ms in MAPS] + [(EXTRA_MAPS_AT[0], ms) for ms in EXTRA_MAPS_AT[1]]
    return list(itertools.product(hm, N_LINEAR, PICTURES, CHUNKS))


def case_bitid():
    """a training handle and a render handle with the same parameters, encoding and coordinates, on every shape"""
    from implicit_image import decode as dec
    from implicit_image._engine import FourierEngine, FourierRenderEngine, load_library
    lib = load_library()
    rows = []
    for ((hid, ms), nl, (H, W), chunk) in shapes():
        gen = torch.Generator().manual_seed(1000 * hid + 10 * ms + nl)
        flat = fourier_params(hid, nl, ms, gen).cuda()
        B = (torch.randn(2, ms // 2, generator=gen) * MAP_SCALE).cuda()
        gh, gw = torch.linspace(0, 1, H).cuda(), torch.linspace(0, 1, W).cuda()
        tr = FourierEngine(H, W, hid, nl, ms, chunk_pixels=chunk)
        rn = FourierRenderEngine(H, W, hid, nl, ms, chunk_pixels=chunk)
        for e in (tr, rn):
            e.set_params(flat)
            e.set_encoding(B)
            e.set_coords(gh, gw)
        ref, _ = tr.forward(want_pred=True, want_sse=False)
        # both outputs, the byte buffer followed by a 16-byte guard
        buf = Guarded(H * W * 3, 8, GUARD)
        pred = torch.full((H, W, 3), float("nan"), device="cuda")
        rc = lib.sf_render(rn.h, buf.ptr(), pred.data_ptr())
        u8 = buf.samples((H, W, 3))
        u8_only, _ = rn.render(want_u8=True, want_pred=False)
        _, pred_only = rn.render(want_u8=False, want_pred=True)
        u8_tr, pred_tr = tr.render(want_u8=True, want_pred=True)         # the same kernel on the training handle
        torch.cuda.synchronize()
        rows.append(dict(hidden=hid, map_size=ms, n_linear=nl, H=H, W=W, chunk=chunk, rc=int(rc),
                         finite=bool(torch.isfinite(ref).all()),
                         pred_equal=bool(torch.equal(pred, ref)), u8_equal=bool(torch.equal(u8, dec.to_u8(ref))),
                         u8_only_equal=bool(torch.equal(u8_only, u8)), pred_only_equal=bool(torch.equal(pred_only, ref)),
                         train_pred_equal=bool(torch.equal(pred_tr, ref)), train_u8_equal=bool(torch.equal(u8_tr, u8)),
                         guard_intact=buf.guard_intact(),
                         levels=int(u8.unique().numel()), pmin=float(ref.min()), pmax=float(ref.max())))
        tr.close()
        rn.close()
    return {"cases": rows}


def small_model(seed=0, out_gain=8.0, **kw):
    """(CPU state dict, decode shape) of a seeded FourierNet whose output layer is scaled up: a picture, not a constant"""
    from implicit_image.config import _wrap
    from implicit_image.models import registry
    mlp = dict(name="fourier", depth=4, hidden_size=64, map_size=128, map_scale=10.0)
    mlp.update(kw)
    torch.manual_seed(seed)
    m = registry["fourier"](**{k: v for k, v in mlp.items() if k != "name"})
    sd = {k: v.detach().clone().float() for k, v in m.state_dict().items()}
    last = f"layers.{2 * (mlp['depth'] - 2)}.weight"
    sd[last] = sd[last] * out_gain
    return sd, _wrap({"mlp": mlp, "engine": {}})


def case_windows():
    """a window of a grid == the same region of the full render; a banded render == the one-band render"""
    from implicit_image.decode import render_fourier
    sd, shape = small_model()
    rows, cols = torch.linspace(0, 1, 128), torch.linspace(0, 1, 128)
    full, fpred = render_fourier(sd, shape, rows, cols, want_pred=True)
    win, wpred = render_fourier(sd, shape, rows[32:96], cols[16:80], want_pred=True)
    band, bpred = render_fourier(sd, shape, rows, cols, band_rows=7, want_pred=True)
    return {"window_equal": bool(torch.equal(win, full[32:96, 16:80])), "window_pred_equal": bool(torch.equal(wpred, fpred[32:96, 16:80])),
            "band_equal": bool(torch.equal(band, full)), "band_pred_equal": bool(torch.equal(bpred, fpred)),
            "distinct_levels": int(full.unique().numel()), "shape": list(full.shape)}


def case_refuse():
    """argument and state checks only: every call below returns an error code before anything reaches the device"""
    import ctypes as C
    from implicit_image import _engine as E
    lib = E.load_library()
    out, rec = recorder(lib)
    H = W = 64
    u8 = torch.zeros(H * W * 3 + 4, dtype=torch.uint8, device="cuda")
    lin = torch.linspace(0, 1, 64).cuda()
    B = torch.randn(2, 32).cuda()
    # call order: nothing set, the coordinates only, the encoding only
    eng = E.FourierRenderEngine(H, W, 64, 3, 64)
    eng.profile(True)
    rec("before_anything", lib.sf_render(eng.h, u8.data_ptr(), None))
    eng.set_coords(lin, lin)
    rec("before_encoding", lib.sf_render(eng.h, u8.data_ptr(), None))
    out["launches_state_a"] = launches(eng)
    eng.close()
    eng = E.FourierRenderEngine(H, W, 64, 3, 64)
    eng.profile(True)
    eng.set_encoding(B)
    rec("before_coords", lib.sf_render(eng.h, u8.data_ptr(), None))
    eng.set_coords(lin, lin)
    # argument checks of sf_render / sf_wavelet_render
    rec("sf_render_both_null", lib.sf_render(eng.h, None, None))
    rec("sf_render_misaligned", lib.sf_render(eng.h, u8.data_ptr() + 1, None))
    rec("sf_wavelet_render", lib.sf_wavelet_render(eng.h, 0, 64, 0, 64, u8.data_ptr(), None))
    buf = torch.zeros(eng.num_params, device="cuda")
    refused_training_calls(rec, lib, eng, buf, feather_layers=3, render_to=None, set_target=True)
    out["launches_state_b"] = launches(eng)
    out["num_params"] = working_calls(rec, lib, eng, buf, offset_layer=1, set_and_count=True)[2]
    rec("ok_sf_render", lib.sf_render(eng.h, u8.data_ptr(), None))
    rep = eng.profile_report()
    out["k_ff_render_launches"] = int(rep["k_ff_render"]["launches"])
    out["k_fwd_launches"] = int(rep["k_fwd"]["launches"])
    rec("ok_sf_profile_reset", lib.sf_profile_reset(eng.h))
    rec("ok_sf_profile_enable", lib.sf_profile_enable(eng.h, 0))
    torch.cuda.synchronize()
    eng.close()
    # creation: sf_fourier_create's validation, word for word
    h = C.c_void_p()
    for name, kw in (("create_hidden", dict(hidden=100)), ("create_map", dict(map_size=96)), ("create_layers", dict(n_linear=1)),
                     ("create_bf16", dict(compute_dtype=0)), ("create_abi", dict(abi_version=2))):
        f = dict(abi_version=E.SF_ABI_VERSION, height=64, width=64, in_features=2, out_features=3, map_size=64, hidden=64,
                 n_linear=3, compute_dtype=1, beta1=0.0, beta2=0.0, eps=0.0, device=0, stream=None, chunk_pixels=0)
        f.update(kw)
        cfg = E.sf_fourier_config(**f)
        rec(name, lib.sf_fourier_render_create(C.byref(cfg), C.byref(h)))
        out[name]["handle_null"] = not bool(h.value)
        rc_train = lib.sf_fourier_create(C.byref(cfg), C.byref(h))
        out[name]["same_as_train"] = int(rc_train) == out[name]["rc"] and lib.sf_last_error().decode() == out[name]["msg"]
    return out


MEM = dict(height=1024, width=1024, hidden=128, n_linear=7, map_size=256)


def case_mem(kind):
    """device memory one 128 x 7-Linear, map 256 handle at 1024x1024 takes"""
    from implicit_image._engine import FourierEngine, FourierRenderEngine
    taken, eng = handle_memory(lambda: (FourierRenderEngine if kind == "render" else FourierEngine)(**MEM))
    eng.close()
    return {"taken": taken}


def case_e2e(workdir):
    """fit_one (mlp=fourier masking=none quant=none, and a Small_Dense density-0.5 fit: 90 -> 128) -> decode with
    decode.render=kernel against decode.render=torch: files, path names and printed figures"""
    from implicit_image import decode as dec
    from implicit_image.config import load_config
    from implicit_image.fit import fit_one
    os.chdir(workdir)
    out = {}
    base = ["mlp=fourier", "quant=none", "img.height=64", "img.width=64", "mlp.depth=4", "train.num_steps=30", "train.log_steps=30"]

    def pair(run, tag, extra):
        got = {}
        for mode in ("kernel", "torch"):
            got[mode] = dec.decode([f"decode.dir={run}", f"decode.render={mode}", "decode.truth=synthetic",
                                    f"decode.out={os.path.join(run, tag + '_' + mode + '.ppm')}"] + extra)
        k, t = got["kernel"], got["torch"]
        return {"paths": [k["path"], t["path"]], "size": [k["height"], k["width"]],
                "ppm_identical": open(k["out"], "rb").read() == open(t["out"], "rb").read(),
                "figures_kernel": [k[f] for f in ("loss", "PSNR", "PSNR_8bit")],
                "figures_torch": [t[f] for f in ("loss", "PSNR", "PSNR_8bit")]}

    for tag, extra in (("none", ["masking=none", "mlp.hidden_size=64"]),
                       ("small_dense", ["masking=Small_Dense", "masking.density=0.5", "mlp.hidden_size=128"])):
        cfg = load_config(os.path.join(ROOT, "conf"), base + extra)
        run = os.path.join(workdir, tag)
        fit_one(cfg, torch.device("cuda", 0), run)
        shape = dec.resolve_shape(run)
        out[tag] = {"logical_width": dec.engine_width(shape), "engine_width": dec.padded_width(shape),
                    "fitted": pair(run, "fitted", [])}
        if tag == "none":
            out[tag]["resized"] = pair(run, "resized", ["decode.height=96", "decode.width=80"])
            out[tag]["window"] = pair(run, "window", ["decode.rows=10:50", "decode.cols=3:64", "decode.band_rows=5"])
            auto = dec.decode([f"decode.dir={run}", f"decode.out={os.path.join(run, 'auto.ppm')}"])
            out[tag]["auto_path"] = auto["path"]
            out[tag]["auto_identical"] = open(auto["out"], "rb").read() == open(os.path.join(run, "fitted_kernel.ppm"), "rb").read()
    return out


if __name__ == "__main__":
    child_main({"bitid": case_bitid, "windows": case_windows, "refuse": case_refuse, "mem": case_mem, "e2e": case_e2e})
