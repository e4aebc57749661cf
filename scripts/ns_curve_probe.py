"""GPU: loss curve of the engine (formats 16 / 12 / 8) against the reference's on the non-smooth plateau fixture, and the
first-step gradient error per layer: where does the PSNR deviation on non-smooth content come from?"""
import math, os, sys
import numpy as np
from _common import ROOT
from _gpu_fixtures import siren_engine
from oracle import siren_oracle as so
S = int(sys.argv[1]) if len(sys.argv) > 1 else 256
d = np.load(os.path.join(ROOT, "tests", "golden", f"plateau_ns_256x8_{S}.npz"))
img, grid = so.nonsmooth_image(S, S), so.get_grid(S, S)
p0 = so.siren_init(256, 8, seed=0)
_, _, gref = so.loss_and_grads(p0, grid, img)
gref = so.flatten(gref)
idx = [0, 1, 2, 3, 5, 10, 20, 40, 80, 120, 160, 199]
print("ref   ", " ".join(f"{d['losses'][i]:.5e}" for i in idx), f"psnr {float(d['psnr']):.4f}")
for fmt in (16, 12, 8):
    eng = siren_engine(S, S, 256, 8, "f16", p0, img, scratch_format=fmt)
    eng.forward_backward()
    g = eng.get_grads().cpu().numpy()
    off, errs = 0, []
    dims = [2] + [256] * 7 + [3]
    for l in range(8):
        n = dims[l] * dims[l + 1] + dims[l + 1]
        errs.append(np.linalg.norm(g[off:off + n] - gref[off:off + n]) / np.linalg.norm(gref[off:off + n])); off += n
    losses = np.array(eng.step([3e-4 * 0.5 ** (t // 40) for t in range(200)], want_loss=True))
    _, sse = eng.forward(want_pred=False)
    print(f"fmt {fmt:2d}", " ".join(f"{losses[i]:.5e}" for i in idx), f"psnr {10 * math.log10(3 * S * S / sse):.4f}")
    print("       first-step gradient error per layer:", " ".join(f"{e:.1e}" for e in errs))
    eng.close()
