"""Child of tests/test_gpu_wavelet_render.py: one WaveletSiren render-path GPU case per process."""
import os

import torch

from _gpu_child import ROOT, child_main
from _gpu_fixtures import (golden, handle_memory, launches, recorder, refused_training_calls, u8_ref, wavelet_params,
                           working_calls)

# (hidden, depth, outermost_linear, first_omega_0, hidden_omega_0, H, chunk_pixels): every forward kernel - k_fwd<32 | 64 |
# 128 | 256> and k_fwd_pipe (256, depth >= 3) - depths 2 / 3 / 8 / 16, both output layers, both omegas, the smallest
# pictures, and coefficient grids of 3 and 11 chunks
BITID = [
    (32, 3, True, 50.0, 30.0, 64, 0),
    (32, 16, True, 50.0, 30.0, 6, 0),
    (64, 2, True, 50.0, 30.0, 10, 0),
    (64, 3, True, 50.0, 30.0, 2, 0),
    (64, 3, True, 50.0, 30.0, 4, 0),
    (64, 3, False, 30.0, 50.0, 6, 0),
    (64, 4, True, 50.0, 30.0, 100, 256),       # n = 52: 2704 coefficients in 11 chunks, the last of 144
    (128, 8, True, 50.0, 30.0, 250, 0),        # conf/mlp/wavelet_siren.yaml
    (128, 5, False, 50.0, 30.0, 64, 0),
    (256, 2, True, 50.0, 30.0, 64, 0),         # k_fwd<256>
    (256, 8, True, 50.0, 30.0, 250, 0),        # k_fwd_pipe
    (256, 4, False, 30.0, 50.0, 64, 512),      # k_fwd_pipe, n = 34: 1156 coefficients in 3 chunks
    (256, 16, True, 50.0, 30.0, 64, 0),
]
SMALL = dict(depth=4, hidden_size=64, first_omega_0=50.0, hidden_omega_0=30.0)
YAML = dict(depth=8, hidden_size=128, wavelet_levels=1, first_omega_0=50.0, hidden_omega_0=30.0, outermost_linear=True)


def engines(hid, dep, lin, fo, ho, H, chunk, **rkw):
    from implicit_image._engine import WaveletEngine, WaveletRenderEngine
    tr = WaveletEngine(H, H, hid, dep, fo, ho, lin, chunk_pixels=chunk)
    rn = WaveletRenderEngine(H, hid, dep, fo, ho, lin, chunk_pixels=chunk, **rkw)
    lin_v = torch.linspace(0, 1, tr.n).cuda()
    for e in (tr, rn):
        e.set_coords(lin_v, lin_v)
    return tr, rn


def case_bitid():
    """full-window sf_wavelet_render(pred) on a render handle and on the training handle itself == sf_forward(pred) of the
    training handle; rgb8 == decode.to_u8 of the kernel's own pred, whether or not pred is written, on either handle"""
    from implicit_image.decode import to_u8
    rows = []
    for hid, dep, lin, fo, ho, H, chunk in BITID:
        tr, rn = engines(hid, dep, lin, fo, ho, H, chunk)
        for scale in (1.0, 400.0):
            flat = wavelet_params(scale, seed=hid + dep, rescale=scale != 1.0, depth=dep, hidden_size=hid, first_omega_0=fo,
                                  hidden_omega_0=ho, outermost_linear=lin).cuda()
            tr.set_params(flat)
            rn.set_params(flat)
            ref, _ = tr.forward(want_pred=True, want_sse=False)
            u8, pred = rn.render(want_u8=True, want_pred=True)
            u8_only, _ = rn.render(want_u8=True, want_pred=False)
            u8_tr, pred_tr = tr.render_window(0, H, 0, H, want_u8=True, want_pred=True)
            torch.cuda.synchronize()
            rows.append(dict(hidden=hid, depth=dep, H=H, chunk=chunk, linear=lin, scale=scale,
                             pred_equal=bool(torch.equal(pred, ref)), pred_equal_train_handle=bool(torch.equal(pred_tr, ref)),
                             finite=bool(torch.isfinite(ref).all()),
                             u8_equal=bool(torch.equal(u8, to_u8(pred))), u8_ref_equal=bool(torch.equal(u8, u8_ref(pred))),
                             u8_only_equal=bool(torch.equal(u8_only, u8)), u8_train_equal=bool(torch.equal(u8_tr, u8)),
                             below0=int((pred < 0).sum()), above1=int((pred > 1).sum()),
                             clamped0=int(((pred < 0) & (u8 == 0)).sum()), clamped255=int(((pred > 1) & (u8 == 255)).sum()),
                             pmin=float(pred.min()), pmax=float(pred.max())))
        tr.close()
        rn.close()
    return {"cases": rows}


def case_ragged():
    """output sizes whose byte count is no multiple of 4, windows whose first pixel is no multiple of 64, a guard region
    behind the byte buffer; bytes with and without pred"""
    import ctypes as C
    from implicit_image.decode import to_u8
    GUARD = 256
    out = []
    for H, wins in ((10, [(2, 7, 1, 8), (0, 1, 0, 1), (9, 10, 3, 10), (0, 10, 0, 10), (3, 6, 0, 3)]),
                    (64, [(5, 28, 7, 30), (0, 64, 0, 63), (63, 64, 0, 64), (1, 64, 1, 64)])):
        tr, rn = engines(64, 3, True, 50.0, 30.0, H, 0)
        flat = wavelet_params(400.0, seed=3, rescale=True, depth=3, hidden_size=64, first_omega_0=50.0,
                              hidden_omega_0=30.0).cuda()
        tr.set_params(flat)
        rn.set_params(flat)
        full, _ = tr.forward(want_pred=True, want_sse=False)
        for r0, r1, c0, c1 in wins:
            nb = (r1 - r0) * (c1 - c0) * 3
            row = dict(H=H, win=[r0, r1, c0, c1], nbytes=nb)
            for tag, eng in (("render", rn), ("train", tr)):
                for with_pred in (True, False):
                    buf = torch.full((nb + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
                    pred = torch.full(((r1 - r0), (c1 - c0), 3), float("nan"), device="cuda")
                    rc = eng.lib.sf_wavelet_render(eng.h, r0, r1, c0, c1, buf.data_ptr(), pred.data_ptr() if with_pred else None)
                    torch.cuda.synchronize()
                    want = full[r0:r1, c0:c1]
                    k = f"{tag}_{'pred' if with_pred else 'nopred'}"
                    row[k] = dict(rc=int(rc), bytes_equal=bool(torch.equal(buf[:nb], to_u8(want).reshape(-1))),
                                  guard_intact=bool((buf[nb:] == 0xAB).all()),
                                  pred_equal=bool(torch.equal(pred, want)) if with_pred else True)
            out.append(row)
        tr.close()
        rn.close()
    return {"cases": out}


def case_windows():
    """windows of a picture == that region of the full render, pred and bytes; decode's banded render == one band; a handle
    created for 7 rows refuses 8"""
    from implicit_image.config import _wrap
    from implicit_image.decode import render_wavelet
    from implicit_image.models import registry
    out = {"windows": []}
    for (hid, dep, H) in ((64, 4, 128), (256, 3, 250), (64, 3, 10)):
        tr, rn = engines(hid, dep, True, 50.0, 30.0, H, 0)
        flat = wavelet_params(1.0, seed=1, rescale=False, depth=dep, hidden_size=hid, first_omega_0=50.0,
                              hidden_omega_0=30.0).cuda()
        rn.set_params(flat)
        tr.set_params(flat)
        fu8, fpred = rn.render(want_u8=True, want_pred=True)
        if H == 10:
            wins = [(o, o + 1, 0, H) for o in range(H)] + [(0, H, o, o + 1) for o in range(H)]
        else:
            wins = [(32, 96, 16, 80), (0, 5, 0, 9), (0, 5, H - 9, H), (H - 5, H, 0, 9), (H - 5, H, H - 9, H), (77, 78, 31, 32),
                    (0, 1, 0, 1), (H - 1, H, H - 1, H), (1, H, 3, H - 1)]
        for r0, r1, c0, c1 in wins:
            u8, pred = rn.render(r0, r1, c0, c1, want_u8=True, want_pred=True)
            u8t, predt = tr.render_window(r0, r1, c0, c1, want_u8=True, want_pred=True)
            torch.cuda.synchronize()
            out["windows"].append(dict(H=H, win=[r0, r1, c0, c1],
                                       pred_equal=bool(torch.equal(pred, fpred[r0:r1, c0:c1])),
                                       u8_equal=bool(torch.equal(u8, fu8[r0:r1, c0:c1])),
                                       train_pred_equal=bool(torch.equal(predt, fpred[r0:r1, c0:c1])),
                                       train_u8_equal=bool(torch.equal(u8t, fu8[r0:r1, c0:c1]))))
        out[f"distinct_levels_{H}"] = int(fu8.unique().numel())
        tr.close()
        rn.close()
    # decode's band loop
    kw = dict(name="wavelet_siren", **SMALL, outermost_linear=True)
    torch.manual_seed(2)
    sd = registry["wavelet_siren"](**kw).state_dict()
    shape = _wrap({"mlp": kw, "img": {"height": 128, "width": 128}, "engine": {}})
    one, onep = render_wavelet(sd, shape, 128, (0, 128), (0, 128), want_pred=True)
    band, bandp = render_wavelet(sd, shape, 128, (0, 128), (0, 128), band_rows=7, want_pred=True)
    win, winp = render_wavelet(sd, shape, 128, (32, 96), (16, 80), band_rows=7, want_pred=True)
    out["band_equal"] = bool(torch.equal(band, one))
    out["band_pred_equal"] = bool(torch.equal(bandp, onep))
    out["band_window_equal"] = bool(torch.equal(win, one[32:96, 16:80]) and torch.equal(winp, onep[32:96, 16:80]))
    # max_rows
    from implicit_image._engine import WaveletRenderEngine
    eng = WaveletRenderEngine(128, 64, 4, max_rows=7)
    lin_v = torch.linspace(0, 1, eng.n).cuda()
    eng.set_coords(lin_v, lin_v)
    buf = torch.zeros(8 * 128 * 3, dtype=torch.uint8, device="cuda")
    out["rows7_rc"] = int(eng.lib.sf_wavelet_render(eng.h, 3, 10, 0, 128, buf.data_ptr(), None))
    out["rows8_rc"] = int(eng.lib.sf_wavelet_render(eng.h, 3, 11, 0, 128, buf.data_ptr(), None))
    out["rows8_msg"] = eng.lib.sf_last_error().decode()
    torch.cuda.synchronize()
    eng.close()
    return out


def case_reference():
    """the reference-minted 64x64 predictions of tests/golden/wavelet_grads.npz (seed-0 models)"""
    from implicit_image._engine import WaveletRenderEngine
    from implicit_image.decode import to_u8
    g = golden("wavelet_grads")
    out = {}
    for tag, kw in (("small", SMALL), ("yaml", YAML)):
        flat = wavelet_params(1.0, seed=0, rescale=False, **kw).cuda()
        eng = WaveletRenderEngine(64, kw["hidden_size"], kw["depth"], kw["first_omega_0"], kw["hidden_omega_0"], True)
        lin_v = torch.linspace(0, 1, eng.n).cuda()
        eng.set_coords(lin_v, lin_v)
        eng.set_params(flat)
        u8, pred = eng.render(want_u8=True, want_pred=True)
        torch.cuda.synchronize()
        ref = torch.tensor(g[f"{tag}/pred"])
        out[tag] = {"max_abs": float((pred.cpu() - ref).abs().max()),
                    "max_levels": int((u8.cpu().int() - to_u8(ref).int()).abs().max())}
        eng.close()
    return out


def case_refuse():
    """argument checks only: every call below returns an error code before anything reaches the device"""
    import ctypes as C
    from implicit_image import _engine as E
    lib = E.load_library()
    eng = E.WaveletRenderEngine(64, 64, 4)
    buf = torch.zeros(eng.num_params, device="cuda")
    u8 = torch.zeros(64 * 64 * 3 + 8, dtype=torch.uint8, device="cuda")
    out, rec = recorder(lib)
    eng.profile(True)
    rec("before_set_coords", lib.sf_wavelet_render(eng.h, 0, 64, 0, 64, u8.data_ptr(), None))
    lin_v = torch.linspace(0, 1, eng.n).cuda()
    rec("ok_sf_set_coords", lib.sf_set_coords(eng.h, lin_v.data_ptr(), lin_v.data_ptr()))
    refused_training_calls(rec, lib, eng, buf, feather_layers=4, render_to=u8.data_ptr(), set_target=True)
    # sf_wavelet_render's own argument checks
    rec("wr_both_null", lib.sf_wavelet_render(eng.h, 0, 64, 0, 64, None, None))
    rec("wr_misaligned", lib.sf_wavelet_render(eng.h, 0, 64, 0, 64, u8.data_ptr() + 1, None))
    rec("wr_empty", lib.sf_wavelet_render(eng.h, 5, 5, 0, 64, u8.data_ptr(), None))
    rec("wr_reversed", lib.sf_wavelet_render(eng.h, 0, 64, 9, 3, u8.data_ptr(), None))
    rec("wr_negative", lib.sf_wavelet_render(eng.h, -1, 64, 0, 64, u8.data_ptr(), None))
    rec("wr_beyond", lib.sf_wavelet_render(eng.h, 0, 65, 0, 64, u8.data_ptr(), None))
    rec("wr_beyond_cols", lib.sf_wavelet_render(eng.h, 0, 64, 0, 65, u8.data_ptr(), None))
    sir = E.RenderEngine(64, 64, 64, 4)
    rec("wr_siren_handle", lib.sf_wavelet_render(sir.h, 0, 64, 0, 64, u8.data_ptr(), None))
    sir.close()
    fou = E.FourierEngine(64, 64, 64, 3, 64)
    rec("wr_fourier_handle", lib.sf_wavelet_render(fou.h, 0, 64, 0, 64, u8.data_ptr(), None))
    fou.close()
    out["launches_after_refusals"] = launches(eng)
    out["param_offset_hf_layer1"] = working_calls(rec, lib, eng, buf, offset_layer=5, set_and_count=True)
    rec("ok_sf_wavelet_render", lib.sf_wavelet_render(eng.h, 0, 64, 0, 64, u8.data_ptr(), None))
    rep = eng.profile_report()
    out["k_wv_render_launches"] = int(rep["k_wv_render"]["launches"])
    out["k_render_launches"] = int(rep["k_render"]["launches"])
    rec("ok_sf_profile_reset", lib.sf_profile_reset(eng.h))
    rec("ok_sf_profile_enable", lib.sf_profile_enable(eng.h, 0))
    torch.cuda.synchronize()
    eng.close()
    # creation: what sf_wavelet_create refuses, with its messages
    h = C.c_void_p()
    for name, kw in (("create_odd", dict(height=63)), ("create_hidden", dict(hidden=100)), ("create_bf16", dict(compute_dtype=0)),
                     ("create_depth", dict(depth=1)), ("create_max_rows", dict(max_rows=65)), ("create_abi", dict(abi_version=2))):
        f = dict(abi_version=E.SF_ABI_VERSION, height=64, max_rows=0, max_cols=0, hidden=64, depth=4, first_omega_0=50.0,
                 hidden_omega_0=30.0, outermost_linear=1, compute_dtype=1, device=0, stream=None, chunk_pixels=0)
        f.update(kw)
        cfg = E.sf_wavelet_render_config(**f)
        rec(name, lib.sf_wavelet_render_create(C.byref(cfg), C.byref(h)))
        out[name]["handle_null"] = not bool(h.value)
    return out


def case_mem(kind):
    """device memory one yaml-model (128x8) handle at 2048x2048 takes"""
    from implicit_image._engine import SirenEngine, WaveletEngine, WaveletRenderEngine
    taken, eng = handle_memory(lambda: WaveletRenderEngine(2048, 128, 8) if kind == "render"
                               else WaveletEngine(2048, 2048, 128, 8))
    out = {"taken": taken, "n": eng.n}
    eng.close()
    if kind == "train":   # what one sub-network's phase + delta scratch is: a plain SIREN handle of the same grid and format
        sub = SirenEngine(1026, 1026, 128, 8, scratch_format=16)
        out["sub_scratch"] = {k: int(sub.debug_scratch(k).numel()) for k in ("phases", "deltas")}
        sub.close()
    return out


def case_e2e(workdir):
    """fit_one -> decode of the run directory on the kernel path: WaveletSiren (masking none and Small_Dense 0.5: width
    45 zero-padded to 64), a second picture size, and a SIREN whose Small_Dense width 181 is zero-padded to 256"""
    from implicit_image import decode as dec
    from implicit_image.config import load_config
    from implicit_image.data import get_grid, read_ppm
    from implicit_image.fit import fit_one
    from implicit_image.models import registry
    os.chdir(workdir)
    out = {}

    def model_bytes(cfg, run, name, H, density):
        sd = torch.load(os.path.join(run, "model.pth"), weights_only=True)["state_dict"]
        model = registry[name](**cfg.mlp, small_dense_density=density).cuda()
        model.load_state_dict(sd)
        model.eval()
        with torch.no_grad():
            pred = model(get_grid(H, H).cuda()).cpu()
        return pred, dec.to_u8(pred)

    base = ["img.height=64", "img.width=64", "mlp.hidden_size=64", "mlp.depth=4", "train.num_steps=40", "train.log_steps=40",
            "quant=none"]
    for tag, extra, density in (("none", ["masking=none"], 1.0), ("small_dense", ["masking=Small_Dense", "masking.density=0.5"], 0.5)):
        cfg = load_config(os.path.join(ROOT, "conf"), ["mlp=wavelet_siren"] + base + extra)
        run = os.path.join(workdir, tag)
        fit_one(cfg, torch.device("cuda", 0), run)
        got = dec.decode([f"decode.dir={run}", "decode.truth=synthetic"])
        pred, ref_u8 = model_bytes(cfg, run, "wavelet_siren", 64, density)
        img = dec.load_truth("synthetic", 64, 64)
        out[tag] = {"path": got["path"], "source": got["source"],
                    "ppm_equal": bool(torch.equal(read_ppm(got["out"]), ref_u8.int())),
                    "psnr8_decode": got["PSNR_8bit"], "psnr8_metrics_on_bytes": dec.metrics(pred, ref_u8, img)["PSNR_8bit"],
                    "engine_width": dec.padded_width(dec.resolve_shape(run)), "logical_width": dec.engine_width(dec.resolve_shape(run))}
        big = dec.decode([f"decode.dir={run}", "decode.height=128", "decode.width=128",
                          f"decode.out={os.path.join(run, 'big.ppm')}"])
        _, ref128 = model_bytes(cfg, run, "wavelet_siren", 128, density)
        out[tag]["big_path"] = big["path"]
        out[tag]["big_shape"] = [big["height"], big["width"]]
        out[tag]["big_equal"] = bool(torch.equal(read_ppm(big["out"]), ref128.int()))
        win = dec.decode([f"decode.dir={run}", "decode.rows=10:50", "decode.cols=3:64", "decode.band_rows=7",
                          f"decode.out={os.path.join(run, 'win.ppm')}"])
        out[tag]["window_equal"] = bool(torch.equal(read_ppm(win["out"]), ref_u8.int()[10:50, 3:64]))
    cfg = load_config(os.path.join(ROOT, "conf"), ["masking=Small_Dense", "masking.density=0.5", "img.height=64", "img.width=64",
                                                   "mlp.hidden_size=256", "mlp.depth=4", "train.num_steps=40",
                                                   "train.log_steps=40", "quant=none"])
    run = os.path.join(workdir, "siren181")
    fit_one(cfg, torch.device("cuda", 0), run)
    got = dec.decode([f"decode.dir={run}"])
    _, ref_u8 = model_bytes(cfg, run, "siren", 64, 0.5)
    out["siren181"] = {"path": got["path"], "source": got["source"], "logical_width": dec.engine_width(dec.resolve_shape(run)),
                       "ppm_equal": bool(torch.equal(read_ppm(got["out"]), ref_u8.int()))}
    return out


if __name__ == "__main__":
    child_main({"bitid": case_bitid, "ragged": case_ragged, "windows": case_windows, "reference": case_reference,
                "refuse": case_refuse, "mem": case_mem, "e2e": case_e2e})
