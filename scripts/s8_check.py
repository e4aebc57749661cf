"""Engine (8-bit and 16-bit scratch) vs its numerics model vs the fp32 oracle: relative L2 gradient errors."""
import numpy as np
import _common  # noqa: F401  (path setup)
from _gpu_fixtures import siren_engine
from oracle import siren_oracle as so, engine_model as em

def rel(a, b): return float(np.linalg.norm(a - b) / np.linalg.norm(b))

for (H, W, hid, dep, seed) in [(32, 40, 64, 4, 0), (32, 40, 256, 8, 0), (48, 56, 128, 6, 0), (5, 7, 32, 3, 1), (1, 1, 64, 2, 1),
                               (64, 64, 256, 8, 0), (128, 128, 256, 8, 0)]:
    p = so.siren_init(hid, dep, seed=seed)
    img = so.synthetic_image(H, W, seed=2)
    grid = so.get_grid(H, W)
    _, sse, g32 = so.loss_and_grads(p, grid, img)
    g32 = so.flatten(g32)
    row = [f"{H}x{W} {hid}x{dep}"]
    for scratch in (16, 12, 8):
        eng = siren_engine(H, W, hid, dep, "f16", p, img, scratch_format=scratch)
        sse_e = eng.forward_backward()
        g = eng.get_grads().cpu().numpy()
        _, sse_m, gm, _ = em.loss_and_grads(p, grid, img, scratch=scratch)   # (12: modelled as 16 below, phases differ)
        gm = so.flatten(gm)
        row.append(f"s{scratch}: eng-vs-model {rel(g, gm):.2e} eng-vs-fp32 {rel(g, g32):.2e} model-vs-fp32 {rel(gm, g32):.2e} finite {np.isfinite(g).all()}")
        # per layer
        if scratch in (8, 12):
            off = 0; per = []; perb = []
            for fin, fout in so.layer_dims(hid, dep):
                n = fin * fout
                per.append(f"{rel(g[off:off+n], gm[off:off+n]):.1e}")
                perb.append(f"{rel(g[off+n:off+n+fout], gm[off+n:off+n+fout]):.1e}")
                off += n + fout
            row.append("per-layer eng-vs-model W " + " ".join(per) + " b " + " ".join(perb))
    print(" | ".join(row), flush=True)
