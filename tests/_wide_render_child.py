"""Child of tests/test_gpu_wide_render.py: one wide-render GPU case per process."""
import ctypes as C
import itertools
import os

import torch

from _gpu_child import ROOT, child_main
from _gpu_fixtures import (Guarded, handle_memory, launches, recorder, refused_training_calls, siren_params, u8_ref, u16_ref,
                           working_calls)
from oracle import siren_oracle as so

SHAPES = [(512, 3), (512, 4), (1024, 3), (1024, 5)]    # depth 3: one hidden product; depth >= 4: the two planes wrap
# (H, W, chunk_pixels): one pixel; one ragged block; a ragged last 256-pixel group; 1024 groups = 2048 / 4096 tiles on at most one
# workgroup per CU, so every persistent workgroup runs several tiles (the NEP wait); nine chunks, the last one ragged
PICTURES = [(1, 1, 0), (5, 7, 0), (67, 45, 0), (512, 512, 0), (1031, 517, 65536)]
GUARD = 64


def widen(u16):
    """uint16 samples as int32 (through int16: every torch build converts and compares that type on the device)"""
    return u16.view(torch.int16).to(torch.int32) & 0xFFFF


def variants(hidden, depth):
    """(out_features, operand type) of a shape: 1 and 3 channels at depth 3, bf16 operands at (512, 4) only"""
    nouts = (3, 1) if depth == 3 else (3,)
    dtypes = ("f16", "bf16") if (hidden, depth) == (512, 4) else ("f16",)
    return list(itertools.product(nouts, dtypes))


def case_bitid(hidden, depth):
    """WideRenderEngine.render(pred) == SirenEngine.forward(pred), and the samples == the conversion of the kernel's own fp32
    output at 8 and 16 bits with and without pred, for one shape on every picture, output layer and variant; once at the
    SIREN initialisation and once with the last layer scaled by 400 and zero output bias"""
    from implicit_image._engine import SirenEngine, WideRenderEngine
    hid, dep = int(hidden), int(depth)
    rows = []
    for (H, W, chunk), lin, (nout, dt) in itertools.product(PICTURES, (True, False), variants(hid, dep)):
        kw = dict(outermost_linear=lin, out_features=nout, compute_dtype=dt, chunk_pixels=chunk)
        tr, rn = SirenEngine(H, W, hid, dep, **kw), WideRenderEngine(H, W, hid, dep, **kw)
        gh, gw = so.grid_vectors(H, W)
        for e in (tr, rn):
            e.set_coords(gh.cuda(), gw.cuda())
        for scale in (1.0, 400.0):
            flat = siren_params(hid, dep, nout, seed=hid + dep, last_scale=scale, bias_scale=1.0 if scale == 1.0 else 0.0).cuda()
            tr.set_params(flat)
            rn.set_params(flat)
            ref, _ = tr.forward(want_pred=True, want_sse=False)
            u8, pred = rn.render(want_u8=True, want_pred=True)
            u8_only, _ = rn.render(want_u8=True, want_pred=False)
            u16, pred16 = rn.render(want_u8=True, want_pred=True, bits=16)
            u16_only, _ = rn.render(want_u8=True, want_pred=False, bits=16)
            _, pred_only = rn.render(want_u8=False, want_pred=True)
            torch.cuda.synchronize()
            w16 = widen(u16)
            rows.append(dict(hidden=hid, depth=dep, H=H, W=W, chunk=chunk, linear=lin, nout=nout, dtype=dt, scale=scale,
                             pred_equal=bool(torch.equal(pred, ref)), pred16_equal=bool(torch.equal(pred16, ref)),
                             pred_only_equal=bool(torch.equal(pred_only, ref)), finite=bool(torch.isfinite(ref).all()),
                             u8_equal=bool(torch.equal(u8, u8_ref(pred))), u8_only_equal=bool(torch.equal(u8_only, u8)),
                             u16_equal=bool(torch.equal(w16, u16_ref(pred))), u16_only_equal=bool(torch.equal(widen(u16_only), w16)),
                             below0=int((pred < 0).sum()), above1=int((pred > 1).sum()),
                             pmin=float(pred.min()), pmax=float(pred.max()), render_format=rn.scratch_format))
        tr.close()
        rn.close()
    return {"cases": rows}


def case_formats():
    """training handles of scratch_format 16, 12 and 8 at (512, 4), 512x512, fp16 give the render handle's pred: their
    phases change form, their activations do not"""
    from implicit_image._engine import SirenEngine, WideRenderEngine
    H = W = 512
    gh, gw = so.grid_vectors(H, W)
    flat = siren_params(512, 4, 3, seed=516, last_scale=400.0, bias_scale=0.0).cuda()
    rn = WideRenderEngine(H, W, 512, 4)
    rn.set_coords(gh.cuda(), gw.cuda())
    rn.set_params(flat)
    _, pred = rn.render(want_u8=False, want_pred=True)
    out = {}
    for fmt in (16, 12, 8):
        tr = SirenEngine(H, W, 512, 4, scratch_format=fmt)
        tr.set_coords(gh.cuda(), gw.cuda())
        tr.set_params(flat)
        ref, _ = tr.forward(want_pred=True, want_sse=False)
        torch.cuda.synchronize()
        out[str(fmt)] = {"format": tr.scratch_format, "pred_equal": bool(torch.equal(pred, ref))}
        tr.close()
    rn.close()
    return out


def case_guards():
    """5x7 (105 bytes: a ragged last dword; 105 samples: an odd count at 16 bits), 1x1 and 3x3 at one channel (9 samples)
    into buffers with sentinel bytes behind them"""
    from implicit_image._engine import WideRenderEngine
    rows = []
    for (H, W, nout), (hid, dep) in itertools.product([(5, 7, 3), (1, 1, 3), (1, 1, 1), (3, 3, 1), (9, 29, 3)], [(512, 3), (1024, 4)]):
        eng = WideRenderEngine(H, W, hid, dep, out_features=nout)
        gh, gw = so.grid_vectors(H, W)
        eng.set_coords(gh.cuda(), gw.cuda())
        eng.set_params(siren_params(hid, dep, nout, seed=7, last_scale=400.0, bias_scale=0.0).cuda())
        n, shape = H * W * nout, (H, W, nout)
        b8, b8_alone, b16, b16_alone = (Guarded(n, bits, GUARD) for bits in (8, 8, 16, 16))
        pred = torch.full(shape, float("nan"), device="cuda")
        lib, h = eng.lib, eng.h
        rcs = [lib.sf_wide_render(h, b8.ptr(), pred.data_ptr()), lib.sf_wide_render(h, b8_alone.ptr(), None),
               lib.sf_wide_render16(h, b16.ptr(), None), lib.sf_wide_render16(h, b16_alone.ptr(), None)]
        torch.cuda.synchronize()
        rows.append(dict(H=H, W=W, nout=nout, hidden=hid, depth=dep, rc=[int(r) for r in rcs], finite=bool(torch.isfinite(pred).all()),
                         u8_equal=bool(torch.equal(b8.samples(shape), u8_ref(pred))),
                         u8_alone_equal=bool(torch.equal(b8_alone.samples(shape), b8.samples(shape))),
                         u16_equal=bool(torch.equal(b16.samples(shape), u16_ref(pred))),
                         u16_alone_equal=bool(torch.equal(b16_alone.samples(shape), b16.samples(shape))),
                         guards_intact=all(b.guard_intact() for b in (b8, b8_alone, b16, b16_alone))))
        eng.close()
    return {"cases": rows}


def case_oracle():
    """(512, 3) at 64x64 from seeded parameters against the fp64 oracle"""
    from implicit_image._engine import WideRenderEngine
    H = W = 64
    p = so.siren_init(512, 3, seed=3)
    flat = torch.tensor(so.flatten(p))
    eng = WideRenderEngine(H, W, 512, 3)
    gh, gw = so.grid_vectors(H, W)
    eng.set_coords(gh.cuda(), gw.cuda())
    eng.set_params(flat.cuda())
    u8, pred = eng.render(want_u8=True, want_pred=True)
    u16, _ = eng.render(want_u8=True, want_pred=False, bits=16)
    torch.cuda.synchronize()
    ref = so.forward([t.double() for t in so.unflatten(flat.numpy(), 512, 3)], so.get_grid(H, W).double()).reshape(H, W, 3)
    ref_u8 = torch.trunc(ref.double() * 255).clamp(0, 255)
    eng.close()
    return {"max_abs": float((pred.cpu().double() - ref.double()).abs().max()),
            "max_levels": int((u8.cpu().double() - ref_u8).abs().max()), "distinct_levels": int(u8.unique().numel()),
            "u16_equal": bool(torch.equal(widen(u16), u16_ref(pred)))}


def case_refuse():
    """argument and state checks only: every call below returns an error code before anything reaches the device"""
    from implicit_image import _engine as E
    lib = E.load_library()
    out, rec = recorder(lib)
    h = C.c_void_p()
    cfg = E.sf_config(E.SF_ABI_VERSION, 64, 64, 0, 0, 2, 3, 256, 4, 50.0, 30.0, 1, 1, 0.9, 0.999, 1e-8, 0, None, 0, 0)
    rec("create_256", lib.sf_wide_render_create(C.byref(cfg), C.byref(h)))
    out["create_256_handle_null"] = not bool(h.value)
    lin = torch.linspace(0, 1, 64).cuda()
    out_buf = torch.zeros(64 * 64 * 3 * 2 + 8, dtype=torch.uint8, device="cuda")
    ptr = out_buf.data_ptr()
    narrow = E.RenderEngine(64, 64, 64, 4)
    narrow.set_coords(lin, lin)
    narrow.profile(True)
    rec("wide_render_on_narrow_render_handle", lib.sf_wide_render(narrow.h, ptr, None))
    rec("wide_render16_on_narrow_render_handle", lib.sf_wide_render16(narrow.h, ptr, None))
    out["launches_narrow"] = launches(narrow)
    narrow.close()
    train = E.SirenEngine(64, 64, 512, 4)
    train.set_coords(lin, lin)
    train.profile(True)
    rec("wide_render_on_wide_training_handle", lib.sf_wide_render(train.h, ptr, None))
    rec("sf_render_on_wide_training_handle", lib.sf_render(train.h, ptr, None))
    out["launches_train"] = launches(train)
    train.close()
    eng = E.WideRenderEngine(64, 64, 512, 4)
    eng.profile(True)
    buf = torch.zeros(eng.num_params, device="cuda")
    rec("before_coords", lib.sf_wide_render(eng.h, ptr, None))
    eng.set_coords(lin, lin)
    rec("both_null", lib.sf_wide_render(eng.h, None, None))
    rec("both_null16", lib.sf_wide_render16(eng.h, None, None))
    rec("odd_base", lib.sf_wide_render(eng.h, ptr + 1, None))
    rec("two_byte_base16", lib.sf_wide_render16(eng.h, ptr + 2, None))
    rec("null_handle", lib.sf_wide_render(None, ptr, None))
    refused_training_calls(rec, lib, eng, buf, feather_layers=4, render_to=None, set_target=True)
    rec("sf_render_on_wide_render_handle", lib.sf_render(eng.h, ptr, None))
    rec("sf_render16_on_wide_render_handle", lib.sf_render16(eng.h, ptr, None))
    li = (C.c_int32 * 4)(512, 512, 512, 3)
    rec("sf_feather_render_attach", lib.sf_feather_render_attach(eng.h, 727, 8, 4, li, li))
    out["launches_render"] = launches(eng)
    out["offsets"] = working_calls(rec, lib, eng, buf, offset_layer=1, set_and_count=True)
    out["format"] = eng.scratch_format
    rec("ok_render", lib.sf_wide_render(eng.h, ptr, None))
    rec("ok_render16", lib.sf_wide_render16(eng.h, ptr, None))
    torch.cuda.synchronize()
    rep = eng.profile_report()
    out["k_render_launches"] = int(rep["k_render"]["launches"])
    out["other_launches"] = int(sum(v["launches"] for k, v in rep.items() if k not in ("k_render", "k_images")))
    eng.close()
    return out


def case_mem(kind):
    """device memory one 512x4 handle at 1024x1024 takes"""
    from implicit_image._engine import SirenEngine, WideRenderEngine
    taken, eng = handle_memory(lambda: (WideRenderEngine if kind == "render" else SirenEngine)(1024, 1024, 512, 4))
    eng.close()
    return {"taken": taken}


def case_e2e(workdir, tag):
    """fit_one at engine width 512, depth 3 (64x64, 30 steps) -> decode under decode.render=wide and decode.render=torch;
    tag: pth (quant=none), container (k-means, plain container) or padded (mlp.hidden_size=300 -> 512)"""
    from implicit_image import decode as dec
    from implicit_image.config import load_config
    from implicit_image.data import read_ppm
    from implicit_image.fit import fit_one
    os.chdir(workdir)
    ov = {"pth": ["mlp.hidden_size=512", "quant=none"],
          "container": ["mlp.hidden_size=512", "quant=kmeans", "quant.num_steps=5", "quant.log_steps=5", "entropy_coding=plain"],
          "padded": ["mlp.hidden_size=300", "quant=none"]}[tag]
    cfg = load_config(os.path.join(ROOT, "conf"), ["img.height=64", "img.width=64", "mlp.depth=3", "train.num_steps=30",
                                                   "train.log_steps=30", "masking=none"] + ov)
    run = os.path.join(workdir, tag)
    fit_one(cfg, torch.device("cuda", 0), run)

    def go(name, *more):
        res = dec.decode([f"decode.dir={run}", f"decode.out={os.path.join(run, name + '.ppm')}", *more])
        return res, open(res["out"], "rb").read()

    w8, w8_raw = go("w8", "decode.render=wide")
    t8, t8_raw = go("t8", "decode.render=torch")
    w16, w16_raw = go("w16", "decode.render=wide", "decode.bits=16")
    t16, t16_raw = go("t16", "decode.render=torch", "decode.bits=16")
    auto, auto_raw = go("auto")
    out = {"wide_path": w8["path"], "wide_why": w8["why"], "torch_path": t8["path"], "auto_path": auto["path"], "source": w8["source"],
           "files8_identical": w8_raw == t8_raw, "files16_identical": w16_raw == t16_raw, "auto_identical": auto_raw == t8_raw,
           "wide16_path": w16["path"], "header16_ok": w16_raw.startswith(b"P6\n64 64\n65535\n"),
           "levels": int(read_ppm(w8["out"]).unique().numel())}
    if tag != "padded":
        full = read_ppm(w8["out"])
        win, _ = go("win", "decode.render=wide", "decode.rows=8:40", "decode.cols=4:36")
        band, band_raw = go("band", "decode.render=wide", "decode.band_rows=7")
        full16 = read_ppm(w16["out"])
        win16, _ = go("win16", "decode.render=wide", "decode.bits=16", "decode.rows=8:40", "decode.cols=4:36", "decode.band_rows=7")
        out.update(window_equal=bool(torch.equal(read_ppm(win["out"]), full[8:40, 4:36])), window_shape=[win["height"], win["width"]],
                   band_identical=band_raw == w8_raw, window_path=win["path"],
                   window16_equal=bool(torch.equal(read_ppm(win16["out"]), full16[8:40, 4:36])))
    return out


if __name__ == "__main__":
    child_main({"bitid": case_bitid, "formats": case_formats, "guards": case_guards, "oracle": case_oracle, "refuse": case_refuse,
                "mem": case_mem, "e2e": case_e2e})
