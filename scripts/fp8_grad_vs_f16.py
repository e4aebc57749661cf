"""Per-layer accuracy of the format-8 gradient against the format-16 one on the same weights, over the first steps of the non-smooth fit\n(evidence that the per-layer fp8 scales leave the early gradients as accurate as the single scale did: <= 1.3 % per layer)."""
import numpy as np
import _common  # noqa: F401  (path setup)
from _gpu_fixtures import siren_engine
from oracle import siren_oracle as so
H = W = 256
img = so.nonsmooth_image(H, W); p = so.siren_init(256, 8, seed=0)
e16, e8 = (siren_engine(H, W, 256, 8, "f16", p, img, scratch_format=fmt) for fmt in (16, 8))
for it in range(0, 12):
    e16.forward_backward(); e8.set_params(e16.get_params()); e8.forward_backward()
    g16, g8 = e16.get_grads().cpu().numpy(), e8.get_grads().cpu().numpy()
    out = []
    sizes = [512] + [65536] * 6 + [768]
    for l in range(8):
        ow = e16.param_offsets(l)[0]
        a, b = g16[ow:ow + sizes[l]], g8[ow:ow + sizes[l]]
        out.append("%.3f/%.3f" % (np.linalg.norm(b - a) / np.linalg.norm(a), np.linalg.norm(b) / np.linalg.norm(a)))
    print("step", it, "per layer W: rel |g8 - g16| / |g16| and |g8| / |g16|:", " ".join(out))
    e16.adam_step(3e-4)
