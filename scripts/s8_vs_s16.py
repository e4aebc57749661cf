"""8-bit vs 16-bit scratch on large grids: gradient agreement (relative L2, per layer) and loss curves."""
import torch
import _common  # noqa: F401  (path setup)
from _gpu_fixtures import siren_engine
from oracle import siren_oracle as so
from bench import device_image

def mk(H, W, scratch, chunk=0):
    return siren_engine(H, W, 256, 8, "f16", so.siren_init(256, 8, seed=0), scratch_format=scratch, chunk_pixels=chunk)

for (H, chunk) in [(1024, 0), (2048, 0), (2048, 1 << 20), (4096, 0)]:
    img = device_image(H, H, torch.device("cuda"))
    a, b = mk(H, H, 16, chunk), mk(H, H, 8, chunk)
    a.set_target(img); b.set_target(img)
    sa, sb = a.forward_backward(), b.forward_backward()
    ga, gb = a.get_grads(), b.get_grads()
    per, off = [], 0
    for fin, fout in so.layer_dims(256, 8):
        n = fin * fout
        per.append("%.1e" % ((ga[off:off+n] - gb[off:off+n]).norm() / ga[off:off+n].norm()).item())
        off += n + fout
    print(f"{H}^2 chunk {chunk}: sse {sa:.6e} {sb:.6e} grad rel L2 {((ga-gb).norm()/ga.norm()).item():.2e} per-layer {per}", flush=True)
    la = a.step([3e-4] * 25, want_loss=True); lb = b.step([3e-4] * 25, want_loss=True)
    print("   loss16", ["%.5f" % x for x in la[::4]]); print("   loss8 ", ["%.5f" % x for x in lb[::4]], flush=True)
    del a, b
