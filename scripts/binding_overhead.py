"""What the model <-> engine binding costs per step: 200 train_epoch calls of Siren 64x4 on 64x64 after 20 warm-up calls (a
launch-latency-bound fit: Siren.engine() runs once per call), one JSON line.  TREE_ROOT (default: this checkout) lets two
checkouts be timed alternately, each run in a fresh process.  HIDDEN (default 64) sets the width: 60 runs zero-padded to 64,
the path whose parameters and moments are scattered and gathered every step.  Usage: binding_overhead.py [TREE_ROOT [HIDDEN]]"""
import json
import os
import sys
import time

root = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
hidden = int(sys.argv[2]) if len(sys.argv) > 2 else 64
sys.path.insert(0, root)
sys.path.insert(0, root + "/implicit-image-compression_amd")
import torch  # noqa: E402

from implicit_image.data import get_grid, synthetic_image  # noqa: E402
from implicit_image.models import registry  # noqa: E402
from implicit_image.utils.train_helper import EngineAdam, train_epoch  # noqa: E402

torch.manual_seed(0)
grid, img = get_grid(64, 64).cuda(), synthetic_image(64, 64, seed=3).cuda()
m = registry["siren"](depth=4, hidden_size=hidden).cuda()
opt = EngineAdam(m, lr=3e-4)
for _ in range(20):
    train_epoch(m, opt, grid, img)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(200):
    loss = train_epoch(m, opt, grid, img)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(json.dumps({"tree": root, "hidden": hidden, "us_per_train_epoch": round(dt / 200 * 1e6, 2), "loss": loss}))
