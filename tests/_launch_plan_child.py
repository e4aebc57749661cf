"""Child of tests/test_gpu_launch_plan.py: every launch path of the engine runs once, eagerly and with profiling on, in ONE
fresh process; per case the per-kernel launch counts with their flops / bytes figures (profile_report), the loss and a
sha256 of the gradient or of the rendered bytes go into the JSON the parent reads.  One more case runs with profiling off
(graph replay needs that): sf_step on a WaveletSiren handle, eagerly and replayed, whose sub-handles launch through the
handle's own launch context - on the capturing stream while a step is captured.
(SIREN_FIT_LIB=<another build> records that build's plan)"""
import os

import torch

from _gpu_child import child_main
from _gpu_fixtures import sha
from implicit_image import _engine as E
from oracle import siren_oracle as so


def plan(eng):
    return {k: {f: v[f] for f in ("launches", "flops_per_launch", "bytes_per_launch")}
            for k, v in eng.profile_report().items() if v["launches"]}


def randn(n, seed, scale):
    return (scale * torch.randn(n, generator=torch.Generator().manual_seed(seed))).cuda()


def siren_flat(hidden, depth):
    return torch.tensor(so.flatten(so.siren_init(hidden, depth, seed=0))).cuda()


def train_passes(eng, img):
    """target, profiling on, one sf_forward and one sf_forward_backward"""
    eng.set_target(img)
    eng.profile(True)
    _, sse_f = eng.forward()
    sse_fb = eng.forward_backward()
    return {"sse_forward": sse_f, "sse_forward_backward": sse_fb, "sha256": sha(eng.get_grads())}


def finish(eng, res):
    res["plan"] = plan(eng)
    eng.profile(False)
    eng.close()
    return res


def siren(H, W, hidden, depth, fmt, dtype="f16", chunk=0, feather=False):
    rows, cols = (t.cuda() for t in so.grid_vectors(H, W))
    eng = E.SirenEngine(H, W, hidden, depth, compute_dtype=dtype, chunk_pixels=chunk, scratch_format=fmt)
    eng.set_coords(rows, cols)
    if feather:      # 68^2 >= the 4547 parameters of 64x3
        eng.feather_attach(68, 8, [hidden] * (depth - 1) + [3], [2] + [hidden] * (depth - 1))
        eng.feather_view("params").copy_(randn(eng.feather_view("params").numel(), 2, 0.1))
        eng.feather_materialise()
    else:
        eng.set_params(siren_flat(hidden, depth))
    res = train_passes(eng, so.synthetic_image(H, W, seed=3).cuda().contiguous())
    if feather:
        eng.adam_step(3e-4)
        res["sha256_params"] = sha(eng.get_params())
    return finish(eng, res)


def fourier(hidden, map_size):
    H, W = 40, 52
    rows, cols = (t.cuda() for t in so.grid_vectors(H, W))
    eng = E.FourierEngine(H, W, hidden, 3, map_size, chunk_pixels=1024)
    eng.set_coords(rows, cols)
    eng.set_encoding(randn(map_size, 0, 1.0).reshape(2, map_size // 2))
    eng.set_params(randn(eng.num_params, 1, 0.05))
    return finish(eng, train_passes(eng, so.synthetic_image(H, W, seed=3).cuda().contiguous()))


def wavelet(H, chunk):
    eng = E.WaveletEngine(H, H, 64, 3, chunk_pixels=chunk)
    rows = cols = torch.linspace(0, 1, eng.n).cuda()
    eng.set_coords(rows, cols)
    eng.set_params(torch.cat([siren_flat(64, 3)] * 2))
    return finish(eng, train_passes(eng, so.synthetic_image(H, H, seed=3).cuda().contiguous()))


def rendered(eng, **kw):
    eng.profile(True)
    u8, pred = eng.render(want_u8=True, want_pred=True, **kw)
    return finish(eng, {"sha256": sha(u8), "sha256_pred": sha(pred)})


def render(hidden, depth, cls=E.RenderEngine, **kw):
    H, W = 40, 52
    rows, cols = (t.cuda() for t in so.grid_vectors(H, W))
    eng = cls(H, W, hidden, depth, chunk_pixels=1024)
    eng.set_coords(rows, cols)
    eng.set_params(siren_flat(hidden, depth))
    return rendered(eng, **kw)


def fourier_render():
    H, W = 40, 52
    rows, cols = (t.cuda() for t in so.grid_vectors(H, W))
    eng = E.FourierRenderEngine(H, W, 64, 3, 64, chunk_pixels=1024)
    eng.set_coords(rows, cols)
    eng.set_encoding(randn(64, 0, 1.0).reshape(2, 32))
    eng.set_params(randn(eng.num_params, 1, 0.05))
    return rendered(eng)


def wavelet_render(**kw):
    eng = E.WaveletRenderEngine(30, 64, 3, chunk_pixels=256)
    rows = cols = torch.linspace(0, 1, eng.n).cuda()
    eng.set_coords(rows, cols)
    eng.set_params(torch.cat([siren_flat(64, 3)] * 2))
    return rendered(eng, **kw)


STEP_LRS = (1e-3, 5e-4, 2.5e-4)


def wavelet_step():
    """64x3 at H = 2 (9 coefficients, one chunk, as wavelet_64x3_H2_one_chunk): sf_step with three learning rates and
    want_loss from the same parameters on two fresh handles, eager and with set_graph_replay(True); the three losses and
    the sha256 of the parameters after them"""
    res = {}
    for mode in ("eager", "replay"):
        eng = E.WaveletEngine(2, 2, 64, 3)
        rows = cols = torch.linspace(0, 1, eng.n).cuda()
        eng.set_coords(rows, cols)
        eng.set_params(torch.cat([siren_flat(64, 3)] * 2))
        eng.set_target(so.synthetic_image(2, 2, seed=3).cuda().contiguous())
        eng.set_graph_replay(mode == "replay")
        losses = eng.step(list(STEP_LRS), want_loss=True)
        res[mode] = {"losses": losses, "sha256_params": sha(eng.get_params())}
        eng.close()
    return res


def cases():
    out = []
    for hidden in (32, 64, 128, 256):
        for depth in (2, 3, 4):
            for fmt, dtype in ((16, "f16"), (12, "f16"), (8, "f16"), (16, "bf16")):
                out.append((f"siren_{hidden}x{depth}_fmt{fmt}_{dtype}_40x52",
                            lambda a=(40, 52, hidden, depth, fmt, dtype, 1024): siren(*a)))
    for fmt in (8, 16):
        out.append((f"siren_256x4_fmt{fmt}_f16_300x300", lambda f=fmt: siren(300, 300, 256, 4, f)))
    for hidden, fmt in ((512, 16), (512, 12), (512, 8), (1024, 12)):
        out.append((f"wide_{hidden}x3_fmt{fmt}_40x52", lambda a=(40, 52, hidden, 3, fmt, "f16", 1024): siren(*a)))
    for hidden in (32, 256):
        for ms in (64, 128):
            out.append((f"fourier_{hidden}x3_ms{ms}_40x52", lambda a=(hidden, ms): fourier(*a)))
    out.append(("wavelet_64x3_H2_one_chunk", lambda: wavelet(2, 0)))
    out.append(("wavelet_64x3_H30_two_pass", lambda: wavelet(30, 256)))
    out.append(("render_64x3_40x52", lambda: render(64, 3)))
    out.append(("render_256x4_40x52", lambda: render(256, 4)))
    out.append(("fourier_render_64x3_ms64_40x52", fourier_render))
    out.append(("wavelet_render_64x3_H30", wavelet_render))
    out.append(("render16_64x3_40x52", lambda: render(64, 3, bits=16)))
    # pixel rows 6 .. 21, columns 9 .. 29 of H = 30 read the 10 x 13 coefficient window at (3, 4) of the 17 x 17 grid
    out.append(("wavelet_render16_window_64x3_H30", lambda: wavelet_render(r0=6, r1=22, c0=9, c1=30, bits=16)))
    # the wide render handle: at depth 4 the last layer reads the plane that layer 0 wrote (the two planes wrap)
    out.append(("wide_render_512x3_40x52", lambda: render(512, 3, E.WideRenderEngine)))
    out.append(("wide_render16_1024x4_40x52", lambda: render(1024, 4, E.WideRenderEngine, bits=16)))
    out.append(("feather_64x3_fmt16_40x52", lambda: siren(40, 52, 64, 3, 16, feather=True)))
    return out


def case_launch_plan():
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    res = {}
    for name, fn in cases():
        res[name] = fn()
        print(name, res[name]["sha256"][:12], flush=True)
    step = wavelet_step()
    print("wavelet_step", step["eager"]["sha256_params"][:12], step["replay"]["sha256_params"][:12], flush=True)
    return {"lib": os.path.basename(E._LIB_PATH), "cases": res, "wavelet_step": step}


if __name__ == "__main__":
    child_main({"launch_plan": case_launch_plan})
