"""Child of tests/test_gpu_feather_render.py: one Feathermap render-path GPU case per process."""
import ctypes as C
import json
import os
import sys

import torch

from _gpu_child import ROOT, child_main, run
from _gpu_fixtures import handle_memory, recorder, siren_params

# hidden, depth, density, P, n, m, engine width (tests/test_feather_render_host.py checks the figures against FeatherNet)
SHAPES = [(32, 2, 0.2, 195, 14, 2, 32), (64, 4, 0.2, 8707, 94, 10, 64), (96, 3, 0.5, 9891, 100, 25, 128),
          (128, 8, 0.2, 99843, 316, 32, 128), (256, 3, 0.1, 67331, 260, 13, 256)]
CHUNKED = 1                                    # the shape that also runs at chunk_pixels=256 (six chunks of the grid)
FP64 = (1, 2, 3)
H, W = 37, 41
MEM = dict(height=1024, width=1024, hidden=128, depth=8)
MEM_FEATHER = (316, 32, [128] * 7 + [3], [2] + [128] * 7)
FIT = ["masking=Feathermap", "quant=none", "mlp.hidden_size=64", "mlp.depth=4", "img.height=64", "img.width=64",
       "train.num_steps=50", "train.log_steps=50"]


def feathernet(hidden, depth, density, seed, chunk_pixels=0):
    from implicit_image.models.siren import Siren
    from implicit_image.pipeline.feathermap import FeatherNet
    torch.manual_seed(seed)
    return FeatherNet(Siren(depth=depth, hidden_size=hidden, first_omega_0=50, hidden_omega_0=30, outermost_linear=True,
                            chunk_pixels=chunk_pixels), compress=density).cuda()


def feather_vector(net):
    return torch.cat([p.detach().reshape(-1) for p in net._param_list()]).float().contiguous()


def render_engine(hidden, depth, n, m, width, height=H, w=W, chunk_pixels=0):
    from implicit_image._engine import FeatherRenderEngine
    from implicit_image.data import get_grid, grid_vectors
    outs, ins = [hidden] * (depth - 1) + [3], [2] + [hidden] * (depth - 1)
    eng = FeatherRenderEngine(height, w, width, depth, n, m, outs, ins, 50.0, 30.0, True, 3, "f16", chunk_pixels=chunk_pixels)
    rows, cols = grid_vectors(get_grid(height, w))
    eng.set_coords(rows.cuda(), cols.cuda())
    return eng


def logical_index(hidden, depth, width):
    """flat engine index of every logical weight and bias element, in V.view(-1) order"""
    idx, off = [], 0
    for l in range(depth):
        fin, fout = (2 if l == 0 else hidden), (3 if l == depth - 1 else hidden)
        fin_p, fout_p = (2 if l == 0 else width), (3 if l == depth - 1 else width)
        idx.append((off + torch.arange(fout)[:, None] * fin_p + torch.arange(fin)[None, :]).reshape(-1))
        off += fin_p * fout_p
        idx.append(off + torch.arange(fout))
        off += fout_p
    return idx, off


def case_bitid(which):
    """a FeatherNet training handle (materialised, then sf_forward) against a FeatherRenderEngine given the same feather
    vector, on a 37x41 grid; shape CHUNKED also at chunk_pixels=256; shapes FP64 also against scaler * (V1 V2) in float64"""
    from implicit_image import decode as dec
    from implicit_image.data import get_grid
    hidden, depth, density, P, n, m, width = SHAPES[int(which)]
    grid = get_grid(H, W).cuda()
    rows = []
    for chunk in (0, 256) if int(which) == CHUNKED else (0,):
        net = feathernet(hidden, depth, density, seed=10 + int(which), chunk_pixels=chunk)
        assert (net.get_num_WandB(), net._size_n, net._size_m, net.module._engine_width) == (P, n, m, width)
        tr = net.engine(grid)                                   # binds and materialises
        ref, _ = tr.forward(want_pred=True, want_sse=False)
        w_train = tr.base.get_params()
        flat = feather_vector(net)
        rn = render_engine(hidden, depth, n, m, width, chunk_pixels=chunk)
        rn.profile(True)
        rn.load_feather(flat)
        w_render = rn.get_params()
        u8, pred = rn.render(want_u8=True, want_pred=True)
        u16, _ = rn.render(want_u8=True, want_pred=False, bits=16)
        torch.cuda.synchronize()
        rep = rn.profile_report()
        idx, total = logical_index(hidden, depth, width)
        covered = torch.zeros(total, dtype=torch.bool)
        covered[torch.cat(idx)] = True
        row = dict(hidden=hidden, depth=depth, chunk=chunk, num_params=[tr.base.num_params, rn.num_params, total],
                   feather_elems=[int(flat.numel()), rn.feather_elems],
                   finite=bool(torch.isfinite(ref).all()), levels=int(u8.unique().numel()),
                   w_equal=bool(torch.equal(w_render, w_train)),
                   padding_max=float(w_render.cpu()[~covered].abs().max()) if (~covered).any() else 0.0,
                   padding_slots=int((~covered).sum()), w_nonzero=int((w_render != 0).sum()),
                   pred_equal=bool(torch.equal(pred, ref)), u8_equal=bool(torch.equal(u8, dec.to_u8(ref))),
                   u16_equal=bool(torch.equal(u16.cpu().to(torch.int32), dec.to_u16(ref).cpu())),
                   mat_launches=int(rep["k_feather_mat"]["launches"]), render_launches=int(rep["k_render"]["launches"]))
        if int(which) in FP64 and chunk == 0:
            V = (net._V1.detach().double().cpu() @ net._V2.detach().double().cpu()).reshape(-1)
            sc = [float(p.detach().cpu()) for p in net._param_list()[2:]]
            want, off = torch.zeros(total, dtype=torch.float64), 0
            for k, ix in enumerate(idx):
                want[ix] = sc[k] * V[off:off + ix.numel()]
                off += ix.numel()
            row["fp64_rel"] = float((w_render.double().cpu() - want).abs().max() / want.abs().max())
        rows.append(row)
        rn.close()
    return {"cases": rows}


def case_reload():
    """a second load_feather with another network's vector on the same handle gives that network's picture"""
    from implicit_image.data import get_grid
    hidden, depth, density, P, n, m, width = SHAPES[1]
    grid = get_grid(H, W).cuda()
    refs, flats = [], []
    for seed in (21, 22):
        net = feathernet(hidden, depth, density, seed=seed)
        refs.append(net(grid).clone())
        flats.append(feather_vector(net).clone())
    rn = render_engine(hidden, depth, n, m, width)
    got = []
    for f in flats:
        rn.load_feather(f)
        got.append(rn.render(want_u8=False, want_pred=True)[1].clone())
    torch.cuda.synchronize()
    rn.close()
    return {"first_equal": bool(torch.equal(got[0], refs[0])), "second_equal": bool(torch.equal(got[1], refs[1])),
            "networks_differ": not torch.equal(refs[0], refs[1])}


def case_refuse():
    """argument and state checks of the two entry points, each recorded with its status and message; then a plain
    RenderEngine in the same process still takes set_params and renders"""
    from implicit_image import _engine as E
    lib = E.load_library()
    out, rec = recorder(lib)
    outs, ins = (C.c_int32 * 4)(64, 64, 64, 3), (C.c_int32 * 4)(2, 64, 64, 64)
    lin = torch.linspace(0, 1, 64).cuda()
    u8 = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    vec = torch.zeros(2 * 94 * 10 + 8, device="cuda")
    tr = E.SirenEngine(64, 64, 64, 4)
    rec("attach_training_handle", lib.sf_feather_render_attach(tr.h, 94, 10, 4, outs, ins))
    rec("load_training_handle", lib.sf_feather_render_load(tr.h, vec.data_ptr()))
    tr.close()
    ff = E.FourierRenderEngine(64, 64, 64, 3, 64)
    rec("attach_fourier_render", lib.sf_feather_render_attach(ff.h, 94, 10, 3, outs, ins))
    ff.close()
    rn = E.RenderEngine(64, 64, 64, 4)
    rn.profile(True)
    rn.set_coords(lin, lin)
    rec("load_before_attach", lib.sf_feather_render_load(rn.h, vec.data_ptr()))
    rec("attach_wrong_layers", lib.sf_feather_render_attach(rn.h, 94, 10, 3, outs, ins))
    rec("attach_small_n", lib.sf_feather_render_attach(rn.h, 93, 10, 4, outs, ins))          # 93^2 = 8649 < 8707
    rec("attach_m_above_n", lib.sf_feather_render_attach(rn.h, 94, 95, 4, outs, ins))
    rec("attach_bad_sizes", lib.sf_feather_render_attach(rn.h, 94, 10, 4, ins, outs))
    rec("ok_attach", lib.sf_feather_render_attach(rn.h, 94, 10, 4, outs, ins))
    rec("attach_twice", lib.sf_feather_render_attach(rn.h, 94, 10, 4, outs, ins))
    rec("render_before_load", lib.sf_render(rn.h, u8.data_ptr(), None))
    rec("render16_before_load", lib.sf_render16(rn.h, u8.data_ptr(), None))
    buf = torch.zeros(rn.num_params, device="cuda")
    rec("set_params_after_attach", lib.sf_set_params(rn.h, buf.data_ptr()))
    rec("params_changed_after_attach", lib.sf_params_changed(rn.h))
    rec("training_attach_on_render_handle", lib.sf_feather_attach(rn.h, 94, 10, 4, outs, ins))
    rec("materialise_on_render_handle", lib.sf_feather_materialise(rn.h))
    out["launches_before_load"] = int(sum(v["launches"] for v in rn.profile_report().values()))
    rec("ok_load", lib.sf_feather_render_load(rn.h, vec.data_ptr()))
    rec("ok_render", lib.sf_render(rn.h, u8.data_ptr(), None))
    rec("ok_get_params", lib.sf_get_params(rn.h, buf.data_ptr()))
    p, cnt, wo, bo = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
    rec("ok_state_ptr_params", lib.sf_state_ptr(rn.h, 0, C.byref(p)))
    rec("ok_num_params", lib.sf_num_params(rn.h, C.byref(cnt)))
    rec("ok_param_offset", lib.sf_param_offset(rn.h, 1, C.byref(wo), C.byref(bo)))
    torch.cuda.synchronize()
    rn.close()
    # the binding: set_params raises with the library's message; a bad size leaves no handle behind
    fe = E.FeatherRenderEngine(64, 64, 64, 4, 94, 10, list(outs), list(ins))
    for name, call in (("binding_set_params", lambda: fe.set_params(buf)),
                       ("binding_bad_size", lambda: E.FeatherRenderEngine(64, 64, 64, 4, 93, 10, list(outs), list(ins)))):
        try:
            call()
            out[name] = ""
        except RuntimeError as e:
            out[name] = str(e)
    out["binding_feather_elems"] = fe.feather_elems
    fe.close()
    plain = E.RenderEngine(64, 64, 64, 4)
    plain.set_coords(lin, lin)
    plain.set_params(siren_params(64, 4, 3, 0, 1.0, 1.0).cuda())
    got, _ = plain.render()
    torch.cuda.synchronize()
    out["plain_levels"] = int(got.unique().numel())
    plain.close()
    return out


def free_bytes():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return int(torch.cuda.mem_get_info()[0])


def case_mem(kind):
    """device memory one 128x8 handle at 1024x1024 takes: feather_render (FeatherRenderEngine, density 0.2), render (a plain
    RenderEngine), train (SirenEngine + sf_feather_attach).  feather_render then runs two create / load / render / close
    rounds and reports what the second leaves behind."""
    from implicit_image._engine import FeatherRenderEngine, RenderEngine, SirenEngine

    def train():
        eng = SirenEngine(**MEM, scratch_format=16)
        eng.feather_attach(*MEM_FEATHER)
        return eng
    make = {"feather_render": lambda: FeatherRenderEngine(MEM["height"], MEM["width"], MEM["hidden"], MEM["depth"], *MEM_FEATHER),
            "render": lambda: RenderEngine(**MEM), "train": train}[kind]
    taken, eng = handle_memory(make)
    out = {"taken": taken}
    if kind == "feather_render":
        out["feather_elems"] = eng.feather_elems
    eng._views.clear()
    eng.close()
    if kind == "feather_render":
        lin = torch.linspace(0, 1, 1024).cuda()
        vec = (torch.rand(2 * 316 * 32 + 16, generator=torch.Generator().manual_seed(0)) - 0.5).cuda()
        for rnd in range(2):                     # round 0: the process's first use of the kernels is not a handle's
            free0 = free_bytes()
            eng = make()
            eng.set_coords(lin, lin)
            eng.load_feather(vec)
            u8, _ = eng.render()
            out["levels"] = int(u8.unique().numel())
            del u8
            eng.close()
            out["shortfall"] = free0 - free_bytes()
    return out


def case_e2e(workdir):
    """fit (masking=Feathermap, 64x4, 64x64, 50 steps) and decode as the command-line programs, then the reloaded FeatherNet
    and further decodes of the same run in this process"""
    from implicit_image import decode as dec
    from implicit_image.data import get_grid, load_img, read_ppm
    from implicit_image.config import load_config
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "implicit-image-compression_amd"))
    run([sys.executable, "-m", "implicit_image.fit"] + FIT, timeout=200, cwd=workdir, env=env)
    found = None
    for dp, _, files in os.walk(os.path.join(workdir, "outputs")):
        if "model.pth" in files:
            found = dp
    log = run([sys.executable, "-m", "implicit_image.decode", f"decode.dir={found}", "decode.truth=synthetic"], timeout=120,
              cwd=workdir, env=env, split=True)
    printed = json.loads([l for l in log.splitlines() if l.startswith("{")][-1])
    res = json.load(open(os.path.join(found, "result.json")))
    # the picture `fit` evaluated: a FeatherNet reloaded from model.pth (tests/_feather_child.py::case_fit)
    sd = torch.load(os.path.join(found, "model.pth"))["state_dict"]
    net = feathernet(64, 4, 0.2, seed=7)
    net.load_state_dict(sd)
    cfg = load_config(os.path.join(ROOT, "conf"), FIT)
    img = load_img(**cfg.img)
    with torch.no_grad():
        pred = net(get_grid(64, 64).cuda()).cpu()
    full = read_ppm(os.path.join(found, "decoded.ppm"))
    want = dec.metrics(pred, dec.to_u8(pred), img)
    out = {"keys": list(sd), "files": sorted(os.listdir(found)), "result_psnr": float(res["PSNR"]), "printed": printed,
           "metrics_on_reloaded": want, "ppm_equal": bool(torch.equal(full, dec.to_u8(pred).int())),
           "levels": int(full.unique().numel())}

    def again(name, *extra):
        got = dec.decode([f"decode.dir={found}", f"decode.out={os.path.join(found, name + '.ppm')}", *extra])
        return got, read_ppm(got["out"])
    got, win = again("window", "decode.rows=8:24", "decode.cols=4:40")
    out["window_equal"] = bool(torch.equal(win, full[8:24, 4:40]))
    out["window_size"] = [got["height"], got["width"]]
    got, band = again("band", "decode.band_rows=7")
    out["band_equal"] = bool(torch.equal(band, full))
    out["kernel_path"] = [got["path"], got["why"], got["source"]]
    got, deep = again("deep", "decode.bits=16")
    out["bits16_equal"] = bool(torch.equal(deep, dec.to_u16(pred)))
    got, tor = again("torch", "decode.render=torch")
    out["torch_equal"] = bool(torch.equal(tor, full))
    out["torch_path"] = got["path"]
    return out


if __name__ == "__main__":
    child_main({"bitid": case_bitid, "reload": case_reload, "refuse": case_refuse, "mem": case_mem, "e2e": case_e2e})
