"""Child of tests/test_gpu_render16.py: one 16-bit render GPU case per process."""
import itertools
import os

import torch

from _gpu_child import ROOT, child_main
from _gpu_fixtures import Guarded, fourier_params, launches, recorder, siren_params, u8_ref, u16_ref, wavelet_params
from oracle import siren_oracle as so

FORMS = [(32, 2), (256, 2), (256, 3)]                # k_fwd<32>, k_fwd<256>, k_fwd_pipe
PICTURES = [(1, 1), (5, 7), (33, 31), (64, 64)]      # 5x7: a ragged block, an odd sample count at out_features 1 and 3
CHUNKS = (0, 256)
GUARD = 64                                           # sentinel bytes behind every sample buffer


def check16(call16, call8, shape):
    """The assertions every model shares, for one handle and one output shape.  call16(samples_ptr, pred_ptr) and
    call8(bytes_ptr, pred_ptr) are the two entry points on that handle."""
    from implicit_image.decode import to_u8, to_u16
    n = shape[0] * shape[1] * shape[2]
    both, alone = Guarded(n, 16, GUARD), Guarded(n, 16, GUARD)
    pred16 = torch.full(shape, float("nan"), device="cuda")
    pred8 = torch.full(shape, float("nan"), device="cuda")
    u8, u8_after = Guarded(n, 8, GUARD), Guarded(n, 8, GUARD)
    rcs = [call8(u8.ptr(), pred8.data_ptr()), call16(both.ptr(), pred16.data_ptr()), call16(alone.ptr(), None),
           call8(u8_after.ptr(), None)]
    torch.cuda.synchronize()
    s, after = both.samples(shape), u8_after.samples(shape)
    return dict(rc=[int(r) for r in rcs], finite=bool(torch.isfinite(pred16).all()),
                equals_to_u16=bool(torch.equal(s, to_u16(pred16))), equals_formula=bool(torch.equal(s, u16_ref(pred16))),
                alone_equal=bool(torch.equal(alone.samples(shape), s)),
                pred_bit_identical=bool(torch.equal(pred16.view(torch.int32), pred8.view(torch.int32))),
                guard_intact=both.guard_intact() and alone.guard_intact(),
                u8_after_equal=bool(torch.equal(after, to_u8(pred16)) and torch.equal(after, u8.samples(shape))
                                    and torch.equal(after, u8_ref(pred16))),
                u8_guard_intact=u8_after.guard_intact(),
                levels=int(s.unique().numel()), lo=int((s == 0).sum()), hi=int((s == 65535).sum()))


def case_siren():
    from implicit_image._engine import RenderEngine, SirenEngine
    rows = []
    for (hid, dep), nout, lin, (H, W), chunk in itertools.product(FORMS, (1, 2, 3), (True, False), PICTURES, CHUNKS):
        # zero output bias and a scaled output layer: 0.5 + 0.5 * scale * (W h) leaves [0, 1] on both sides (a linear last layer)
        flat = siren_params(hid, dep, nout, seed=hid + dep, last_scale=40.0, bias_scale=0.0).cuda()
        gh, gw = so.grid_vectors(H, W)
        for kind, cls in (("render", RenderEngine), ("train", SirenEngine)):
            eng = cls(H, W, hid, dep, outermost_linear=lin, out_features=nout, chunk_pixels=chunk)
            eng.set_coords(gh.cuda(), gw.cuda())
            eng.set_params(flat)
            lib, h = eng.lib, eng.h
            row = check16(lambda s, p: lib.sf_render16(h, s, p), lambda s, p: lib.sf_render(h, s, p), (H, W, nout))
            if kind == "train":   # and pred is sf_forward's
                ref, _ = eng.forward(want_pred=True, want_sse=False)
                _, pr = eng.render(want_u8=False, want_pred=True, bits=16)
                torch.cuda.synchronize()
                row["pred_is_forward"] = bool(torch.equal(pr, ref))
            row.update(hidden=hid, depth=dep, nout=nout, linear=lin, H=H, W=W, chunk=chunk, handle=kind)
            rows.append(row)
            eng.close()
    return {"cases": rows}


def case_fourier():
    from implicit_image._engine import FourierEngine, FourierRenderEngine
    rows = []
    for hid, (H, W), chunk in itertools.product((32, 256), PICTURES, CHUNKS):
        gen = torch.Generator().manual_seed(1000 * hid + 3)
        flat = fourier_params(hid, 3, 64, gen).cuda()
        B = (torch.randn(2, 32, generator=gen) * 16.0).cuda()
        gh, gw = torch.linspace(0, 1, H).cuda(), torch.linspace(0, 1, W).cuda()
        for kind, cls in (("render", FourierRenderEngine), ("train", FourierEngine)):
            eng = cls(H, W, hid, 3, 64, chunk_pixels=chunk)
            eng.set_params(flat)
            eng.set_encoding(B)
            eng.set_coords(gh, gw)
            lib, h = eng.lib, eng.h
            row = check16(lambda s, p: lib.sf_render16(h, s, p), lambda s, p: lib.sf_render(h, s, p), (H, W, 3))
            if kind == "train":
                ref, _ = eng.forward(want_pred=True, want_sse=False)
                _, pr = eng.render(want_u8=False, want_pred=True, bits=16)
                torch.cuda.synchronize()
                row["pred_is_forward"] = bool(torch.equal(pr, ref))
            row.update(hidden=hid, H=H, W=W, chunk=chunk, handle=kind)
            rows.append(row)
            eng.close()
    return {"cases": rows}


# H -> windows (row0, row1, col0, col1): the full picture, odd origins and sizes, one pixel, an odd pixel count that is no
# multiple of 64 (15, 49, 529), a first pixel that is no multiple of 64
WAVELET_WINDOWS = {
    6: [(0, 6, 0, 6), (1, 4, 1, 6), (5, 6, 3, 4)],
    10: [(0, 10, 0, 10), (1, 8, 3, 10), (9, 10, 9, 10), (3, 6, 0, 3)],
    64: [(0, 64, 0, 64), (5, 28, 7, 30), (3, 4, 5, 6), (63, 64, 0, 63), (1, 64, 1, 64)],
}


def case_wavelet():
    from implicit_image._engine import WaveletEngine, WaveletRenderEngine
    rows = []
    for (hid, dep), H in itertools.product(((32, 2), (256, 3)), sorted(WAVELET_WINDOWS)):
        flat = wavelet_params(400.0, seed=hid + dep, rescale=True, depth=dep, hidden_size=hid, first_omega_0=50.0,
                              hidden_omega_0=30.0).cuda()
        tr = WaveletEngine(H, H, hid, dep, 50.0, 30.0, True)
        rn = WaveletRenderEngine(H, hid, dep, 50.0, 30.0, True)
        lin_v = torch.linspace(0, 1, tr.n).cuda()
        for e in (tr, rn):
            e.set_coords(lin_v, lin_v)
            e.set_params(flat)
        full, _ = tr.forward(want_pred=True, want_sse=False)
        for (r0, r1, c0, c1), (kind, eng) in itertools.product(WAVELET_WINDOWS[H], (("render", rn), ("train", tr))):
            lib, h = eng.lib, eng.h
            row = check16(lambda s, p: lib.sf_wavelet_render16(h, r0, r1, c0, c1, s, p),
                          lambda s, p: lib.sf_wavelet_render(h, r0, r1, c0, c1, s, p), (r1 - r0, c1 - c0, 3))
            _, pr = eng.render_window(r0, r1, c0, c1, want_u8=False, want_pred=True, bits=16)
            torch.cuda.synchronize()
            row["pred_is_forward"] = bool(torch.equal(pr, full[r0:r1, c0:c1]))
            row.update(hidden=hid, depth=dep, H=H, win=[r0, r1, c0, c1], handle=kind)
            rows.append(row)
        tr.close()
        rn.close()
    return {"cases": rows}


def case_refuse():
    """argument and state checks only: every call below returns an error code before anything reaches the device"""
    from implicit_image import _engine as E
    lib = E.load_library()
    out, rec = recorder(lib)
    buf = torch.zeros(64 * 64 * 3 * 2 + 8, dtype=torch.uint8, device="cuda")
    ptr = buf.data_ptr()
    lin = torch.linspace(0, 1, 64).cuda()
    # sf_render16 on a SIREN render handle
    eng = E.RenderEngine(64, 64, 64, 4)
    eng.profile(True)
    rec("r16_before_coords", lib.sf_render16(eng.h, ptr, None))
    eng.set_coords(lin, lin)
    rec("r16_both_null", lib.sf_render16(eng.h, None, None))
    rec("r16_odd_base", lib.sf_render16(eng.h, ptr + 1, None))
    rec("r16_two_byte_base", lib.sf_render16(eng.h, ptr + 2, None))        # 2-byte but not 4-byte aligned
    rec("r16_null_handle", lib.sf_render16(None, ptr, None))
    rec("w16_siren_handle", lib.sf_wavelet_render16(eng.h, 0, 64, 0, 64, ptr, None))
    out["launches_siren"] = launches(eng)
    rec("ok_r16", lib.sf_render16(eng.h, ptr, None))
    rep = eng.profile_report()
    out["k_render_launches"] = int(rep["k_render"]["launches"])
    out["k_render_bytes_per_launch"] = float(rep["k_render"]["bytes_per_launch"])
    eng.close()
    # the wide path
    wide = E.SirenEngine(64, 64, 512, 4)
    wide.set_coords(lin, lin)
    rec("r16_wide_handle", lib.sf_render16(wide.h, ptr, None))
    wide.close()
    # FourierNet: the encoding must be there too
    fou = E.FourierRenderEngine(64, 64, 64, 3, 64)
    fou.profile(True)
    rec("r16_fourier_before_coords", lib.sf_render16(fou.h, ptr, None))
    fou.set_coords(lin, lin)
    rec("r16_fourier_before_encoding", lib.sf_render16(fou.h, ptr, None))
    rec("w16_fourier_handle", lib.sf_wavelet_render16(fou.h, 0, 64, 0, 64, ptr, None))
    out["launches_fourier"] = launches(fou)
    fou.close()
    # WaveletSiren: sf_render16 is refused on both kinds of handle; sf_wavelet_render16's own checks
    wr = E.WaveletRenderEngine(64, 64, 4, max_rows=7)
    wr.profile(True)
    rec("w16_before_coords", lib.sf_wavelet_render16(wr.h, 0, 7, 0, 64, ptr, None))
    lin_n = torch.linspace(0, 1, wr.n).cuda()
    wr.set_coords(lin_n, lin_n)
    rec("r16_wavelet_render_handle", lib.sf_render16(wr.h, ptr, None))
    rec("w16_both_null", lib.sf_wavelet_render16(wr.h, 0, 7, 0, 64, None, None))
    rec("w16_odd_base", lib.sf_wavelet_render16(wr.h, 0, 7, 0, 64, ptr + 1, None))
    rec("w16_two_byte_base", lib.sf_wavelet_render16(wr.h, 0, 7, 0, 64, ptr + 2, None))
    rec("w16_empty", lib.sf_wavelet_render16(wr.h, 5, 5, 0, 64, ptr, None))
    rec("w16_reversed", lib.sf_wavelet_render16(wr.h, 0, 7, 9, 3, ptr, None))
    rec("w16_negative", lib.sf_wavelet_render16(wr.h, -1, 6, 0, 64, ptr, None))
    rec("w16_beyond", lib.sf_wavelet_render16(wr.h, 60, 65, 0, 64, ptr, None))
    rec("w16_beyond_cols", lib.sf_wavelet_render16(wr.h, 0, 7, 0, 65, ptr, None))
    rec("w16_larger_than_max_rows", lib.sf_wavelet_render16(wr.h, 0, 8, 0, 64, ptr, None))
    rec("w16_null_handle", lib.sf_wavelet_render16(None, 0, 7, 0, 64, ptr, None))
    out["launches_wavelet"] = launches(wr)
    rec("ok_w16", lib.sf_wavelet_render16(wr.h, 0, 7, 0, 64, ptr, None))
    wr.close()
    wt = E.WaveletEngine(64, 64, 64, 4)
    wt.set_coords(lin_n, lin_n)
    rec("r16_wavelet_train_handle", lib.sf_render16(wt.h, ptr, None))
    wt.close()
    torch.cuda.synchronize()
    # the binding: bits is 8 or 16
    eng = E.RenderEngine(8, 8, 32, 2)
    try:
        eng.render(bits=12)
        out["binding_bits_12"] = "no error"
    except ValueError as e:
        out["binding_bits_12"] = str(e)
    eng.set_coords(lin[:8].contiguous(), lin[:8].contiguous())
    s, _ = eng.render(bits=16)
    out["binding_dtype"], out["binding_shape"], out["binding_itemsize"] = str(s.dtype), list(s.shape), s.element_size()
    eng.close()
    return out


def case_e2e(workdir):
    """fit_one -> decode decode.bits=16 of the run directory, one fit per model (the shapes of the existing decode tests)"""
    from implicit_image import decode as dec
    from implicit_image.config import load_config
    from implicit_image.data import get_grid, read_ppm
    from implicit_image.fit import fit_one
    from implicit_image.models import registry
    os.chdir(workdir)
    out = {}
    size = ["img.height=64", "img.width=64", "quant=none", "masking=none"]
    fits = {
        "siren": (size + ["mlp.hidden_size=64", "mlp.depth=4", "train.num_steps=40", "train.log_steps=40"], "kernel", []),
        "fourier": (["mlp=fourier"] + size + ["mlp.hidden_size=64", "mlp.depth=4", "train.num_steps=30", "train.log_steps=30"],
                    "kernel", ["decode.render=kernel"]),
        "wavelet_siren": (["mlp=wavelet_siren"] + size + ["mlp.hidden_size=64", "mlp.depth=4", "train.num_steps=40",
                                                          "train.log_steps=40"], "kernel", []),
    }
    for name, (ov, want_path, extra) in fits.items():
        cfg = load_config(os.path.join(ROOT, "conf"), ov)
        run = os.path.join(workdir, name)
        fit_one(cfg, torch.device("cuda", 0), run)

        def go(tag, more):
            return dec.decode([f"decode.dir={run}", f"decode.out={os.path.join(run, tag + '.ppm')}"] + more)
        k16 = go("k16", extra + ["decode.bits=16", "decode.truth=synthetic"])
        t16 = go("t16", ["decode.render=torch", "decode.bits=16"])
        plain = go("plain", extra + ["decode.truth=synthetic"])
        b8 = go("b8", extra + ["decode.bits=8", "decode.truth=synthetic"])
        # the fitted model's own forward on the grid
        sd = torch.load(os.path.join(run, "model.pth"), weights_only=True)["state_dict"]
        model = registry[name](**cfg.mlp).cuda()
        model.load_state_dict(sd)
        model.eval()
        with torch.no_grad():
            pred = model(get_grid(64, 64).cuda()).cpu()
        raw = open(k16["out"], "rb").read()
        ppm = read_ppm(k16["out"])
        psnr16 = k16.get("PSNR_16bit")
        out[name] = {"path": k16["path"], "want_path": want_path, "torch_path": t16["path"],
                     "header_ok": raw.startswith(b"P6\n64 64\n65535\n") and len(raw) == len(b"P6\n64 64\n65535\n") + 64 * 64 * 6,
                     "ppm_equals_model": bool(torch.equal(ppm, u16_ref(pred))), "ppm_equals_to_u16": bool(torch.equal(ppm, dec.to_u16(pred))),
                     "torch_file_identical": open(t16["out"], "rb").read() == raw,
                     "levels": int(ppm.unique().numel()),
                     "psnr16": psnr16, "psnr16_finite": psnr16 is not None and bool(torch.isfinite(torch.tensor(psnr16))),
                     "psnr16_formula": dec.metrics(pred, dec.to_u8(pred), dec.load_truth("synthetic", 64, 64), ppm)["PSNR_16bit"],
                     "keys16": sorted(k for k in k16 if k.startswith("PSNR") or k == "loss"),
                     "keys8": sorted(k for k in plain if k.startswith("PSNR") or k == "loss"),
                     "bits8_file_identical": open(b8["out"], "rb").read() == open(plain["out"], "rb").read(),
                     "bits8_figures_identical": all(b8[k] == plain[k] for k in ("loss", "PSNR", "PSNR_8bit")) and sorted(b8) == sorted(plain),
                     "plain_is_8bit": open(plain["out"], "rb").read().startswith(b"P6\n64 64\n255\n")}
    return out


if __name__ == "__main__":
    child_main({"siren": case_siren, "fourier": case_fourier, "wavelet": case_wavelet, "refuse": case_refuse, "e2e": case_e2e})
