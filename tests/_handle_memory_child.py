"""Child of tests/test_gpu_handle_memory.py: every creator's handle is built, used and destroyed in ONE fresh process, and
the device memory free before each create is compared with what is free after that handle's destroy."""
import torch

from _gpu_child import child_main
from oracle import siren_oracle as so

LR = [3e-4, 3e-4]


def free_bytes():
    """what the device has free once torch's caching allocator holds nothing it does not use"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return int(torch.cuda.mem_get_info()[0])


def train_two_steps(eng, rows, cols, img, flat):
    """coordinates, target, parameters, then one sf_step of two steps with graph replay on"""
    eng.set_coords(rows, cols)
    eng.set_target(img)
    eng.set_params(flat)
    eng.set_graph_replay(True)
    return eng.step(LR, want_loss=True)


def use_siren():
    """auto format at 2^20 pixels (8), a mask (the scratch moves to format 16), graph replay before and after, k-means"""
    from implicit_image._engine import SirenEngine
    H = W = 1024
    rows, cols = (t.cuda() for t in so.grid_vectors(H, W))
    img = torch.rand(H, W, 3, device="cuda")
    flat = torch.tensor(so.flatten(so.siren_init(64, 4, seed=0))).cuda()
    w = torch.randn(4096, device="cuda")
    guess = torch.linspace(float(w.min()), float(w.max()), 7, device="cuda")
    free0 = free_bytes()
    eng = SirenEngine(H, W, 64, 4)
    info = {"format_at_create": eng.scratch_format}
    info["loss"] = train_two_steps(eng, rows, cols, img, flat)
    eng.set_masks(torch.ones_like(flat))
    info["format_with_mask"] = eng.scratch_format
    info["loss_masked"] = eng.step(LR + LR[:1], want_loss=True)      # three steps: longer step tables, a new graph
    out = eng.kmeans_fit(w, guess)
    info["n_centroids"] = int(out[1].item())
    del out
    eng.close()
    return free0, free_bytes(), info


def use_feather():
    """a second SIREN handle with sf_feather_attach"""
    from implicit_image._engine import SirenEngine
    H = W = 64
    rows, cols = (t.cuda() for t in so.grid_vectors(H, W))
    img = so.synthetic_image(H, W, seed=3).cuda().contiguous()
    flat = torch.tensor(so.flatten(so.siren_init(64, 4, seed=0))).cuda()
    free0 = free_bytes()
    eng = SirenEngine(H, W, 64, 4, scratch_format=16)
    eng.feather_attach(94, 8, [64, 64, 64, 3], [2, 64, 64, 64])      # 94^2 >= the 8707 parameters
    eng.feather_view("params").normal_(0.0, 0.1)
    eng.feather_materialise()
    eng.set_coords(rows, cols)
    eng.set_target(img)
    eng.set_graph_replay(True)
    info = {"loss": eng.step(LR, want_loss=True)}
    eng._views.clear()
    eng.close()
    return free0, free_bytes(), info


def use_fourier():
    from implicit_image._engine import FourierEngine
    H = W = 128
    rows, cols = (t.cuda() for t in so.grid_vectors(H, W))
    img = so.synthetic_image(H, W, seed=3).cuda().contiguous()
    B = torch.randn(2, 32, generator=torch.Generator().manual_seed(0)).cuda()
    free0 = free_bytes()
    eng = FourierEngine(H, W, 64, 4, 64)
    flat = 0.05 * torch.randn(eng.num_params, generator=torch.Generator().manual_seed(1)).cuda()
    eng.set_encoding(B)
    info = {"loss": train_two_steps(eng, rows, cols, img, flat)}
    eng.close()
    del flat
    return free0, free_bytes(), info


def use_wavelet():
    from implicit_image._engine import WaveletEngine
    H = 128
    n = (H + 5) // 2
    rows = cols = torch.linspace(0, 1, n).cuda()
    img = so.synthetic_image(H, H, seed=3).cuda().contiguous()
    sub = torch.tensor(so.flatten(so.siren_init(64, 4, seed=0)))
    flat = torch.cat([sub, sub]).cuda()
    free0 = free_bytes()
    eng = WaveletEngine(H, H, 64, 4)
    info = {"loss": train_two_steps(eng, rows, cols, img, flat)}
    eng.close()
    return free0, free_bytes(), info


def use_render():
    from implicit_image._engine import RenderEngine
    H = W = 256
    rows, cols = (t.cuda() for t in so.grid_vectors(H, W))
    flat = torch.tensor(so.flatten(so.siren_init(64, 4, seed=0))).cuda()
    free0 = free_bytes()
    eng = RenderEngine(H, W, 64, 4)
    eng.set_coords(rows, cols)
    eng.set_params(flat)
    u8, _ = eng.render()
    info = {"levels": int(u8.unique().numel())}
    del u8
    eng.close()
    return free0, free_bytes(), info


def use_wavelet_render():
    from implicit_image._engine import WaveletRenderEngine
    H = 128
    n = (H + 5) // 2
    rows = cols = torch.linspace(0, 1, n).cuda()
    sub = torch.tensor(so.flatten(so.siren_init(64, 4, seed=0)))
    flat = torch.cat([sub, sub]).cuda()
    free0 = free_bytes()
    eng = WaveletRenderEngine(H, 64, 4)
    eng.set_coords(rows, cols)
    eng.set_params(flat)
    u8, _ = eng.render()
    info = {"levels": int(u8.unique().numel())}
    del u8
    eng.close()
    return free0, free_bytes(), info


CASES = [("sf_create", use_siren), ("sf_create+sf_feather_attach", use_feather), ("sf_fourier_create", use_fourier),
         ("sf_wavelet_create", use_wavelet), ("sf_render_create", use_render), ("sf_wavelet_render_create", use_wavelet_render)]


def case_handle_memory():
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    rows = []
    # round 0 is the process's first use of every kernel and of graph capture: what the runtime sets up once (code objects,
    # its own pools) is not a handle's; round 1 is the one that is measured
    for rnd in range(2):
        for name, fn in CASES:
            free0, free1, info = fn()
            rows.append(dict(round=rnd, creator=name, free_before=free0, free_after=free1, shortfall=free0 - free1, **info))
            print(rows[-1], flush=True)
    return {"cases": rows}


if __name__ == "__main__":
    child_main({"handle_memory": case_handle_memory})
