import os, numpy as np, torch
from _common import ROOT
from _gpu_fixtures import siren_engine
from oracle import siren_oracle as so
d = np.load(os.path.join(ROOT, "tests/golden/rigl_256x8_48.npz"))
p = so.siren_init(256, 8, seed=0)
bits = np.unpackbits(d["mask0"]); off = 0
for l in range(8):
    n = p[2 * l].numel()
    p[2 * l] = p[2 * l] * torch.tensor(bits[off:off + n].astype(np.float32)).view(p[2 * l].shape); off += n
img = torch.tensor(d["img"]); H = W = 48
grid = so.get_grid(H, W)
_, _, g32 = so.loss_and_grads(p, grid, img)
for fmt in (16, 12, 8):
    eng = siren_engine(H, W, 256, 8, "f16", p, img, scratch_format=fmt)
    eng.forward_backward()
    g = eng.get_grads().cpu()
    w_off, _ = eng.param_offsets(7)
    gl = g[w_off:w_off + 768].view(3, 256); rl = g32[14]
    zc = (gl.abs().sum(0) == 0).nonzero().flatten().tolist()
    print(f"fmt {fmt}: last-layer zero columns {zc}; rel err {float((gl - rl).norm() / rl.norm()):.3e}; ref col 8 {rl[:, 8].tolist()} eng col 8 {gl[:, 8].tolist()}")
    for l in (6, 5, 1):
        wo, _ = eng.param_offsets(l)
        gw_ = g[wo:wo + 65536].view(256, 256); rw = g32[2 * l]
        zr = (gw_.abs().sum(0) == 0).nonzero().flatten().tolist()
        print(f"   layer {l}: zero columns {zr[:10]} rel err {float((gw_ - rw).norm() / rw.norm()):.3e}")
