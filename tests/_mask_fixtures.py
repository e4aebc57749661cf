"""What the tests of the two device topology updates (sf_mask_update, sf_mask_prune_global) share: the configurations, the
small helpers of their children, the loader of a captured reference update into a live model, the fit on both routes, and
the engine the host tests put under a Masking.  Nothing here touches the device at import."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

KNOB = "SIREN_FIT_DEVICE_MASK"


class Cfg(dict):
    __getattr__ = dict.get


# conf/masking/RigL.yaml
RIGL = Cfg(name="RigL", density=0.5, sparse_init="erdos-renyi-kernel", dense_gradients=True, growth_mode="absolute-gradient",
           prune_mode="magnitude", redistribution_mode="none", dense=False, prune_rate=0.1, decay_schedule="cosine",
           end_when=1500, interval=20)
# conf/masking/Pruning.yaml's keys on a schedule short enough that six updates three steps apart prune something every time
PRUNING = Cfg(name="Pruning", density=1.0, sparse_init="random", final_density=0.5, dense_gradients=True, growth_mode="none",
              prune_mode="global-magnitude", redistribution_mode="none", dense=False, decay_schedule="magnitude-prune",
              start_when=0, end_when=40, interval=3)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def slices_of(eng, layers):
    out = []
    for l in layers:
        w, b = eng.param_offsets(l)
        out.append((w, b - w))
    return out


def copy_flat(dsts, flat):
    off = 0
    for t in dsts:
        t.copy_(torch.tensor(flat[off:off + t.numel()]).view(t.shape))
        off += t.numel()


def seeded_sides(mcfg, hidden, depth):
    """two (model, optimiser, scheduler, mask) from the same seed on the device: the host side and the device side"""
    from implicit_image.models import registry
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, setup_mask
    sides = []
    for _ in range(2):
        torch.manual_seed(0)
        m = registry["siren"](depth=depth, hidden_size=hidden, first_omega_0=50, hidden_omega_0=30).to("cuda")
        optim, sched = get_optimizer_lr_scheduler(m, Cfg(name="adam", lr=3e-4))
        sides.append((m, optim, sched, setup_mask(m, optim, mcfg)))
    return sides


def flat_state(m, mask):
    eng = m.bound_engine
    return [eng.view(w).clone().cpu() for w in ("params", "grads", "exp_avg", "exp_avg_sq")] + [mask.flat_mask().cpu()]


# ---- a captured update of the real reference in a live model ---------------------------------------------------------------
def load_captured(name, mcfg, upd):
    """tests/golden/<name>.npz (the real reference's run on the 64x4 model): a model, optimiser and mask under mcfg, bound to
    an engine, holding the reference's state before its update at step `upd` - weights, gradients, moments, masks, mask_step,
    adjustments, the totals of the statistics.  -> a namespace: d (the file), pre / post (its key prefixes before and after
    the update), mask, optim, params, names, mask_bits(), out ({"init_equal": ...})"""
    from _gpu_fixtures import golden
    from implicit_image.data import get_grid
    from implicit_image.models import registry
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, setup_mask
    d = golden(name)
    torch.manual_seed(0)
    m = registry["siren"](depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30).to("cuda")
    optim, _ = get_optimizer_lr_scheduler(m, Cfg(name="adam", lr=3e-4))
    mask = setup_mask(m, optim, mcfg)
    names = [str(n) for n in d["mask_names"]]

    def mask_bits():
        return np.packbits(np.concatenate([mask.mask_dict[n].cpu().numpy().ravel().astype(np.uint8) for n in names]))
    out = {"init_equal": bool(np.array_equal(mask_bits(), d["mask_init"]))}
    eng = m.engine(get_grid(16, 16).cuda())
    optim._bind_state(eng)
    params = m._param_list()
    pre, post = f"u{upd}_", f"a{upd}_"
    with torch.no_grad():
        copy_flat([p.data for p in params], d[pre + "w"])
        copy_flat([p.grad for p in params], d[pre + "g"])
        copy_flat([optim.state[p]["exp_avg"] for p in params], d[pre + "m"])
        copy_flat([optim.state[p]["exp_avg_sq"] for p in params], d[pre + "v"])
    mb, off = np.unpackbits(d[pre + "mask"]), 0
    for n in names:
        sh = mask.mask_dict[n].shape
        mask.mask_dict[n] = torch.tensor(mb[off:off + sh.numel()].astype(np.float32)).view(sh).cuda()
        off += sh.numel()
    mask.mask_step = int(d[pre + "mask_step"])
    mask.adjusted_growth = float(d[pre + "adjusted_growth"])
    mask.adjustments = list(d[pre + "adjustments"])
    mask.stats.total_nonzero, mask.stats.total_zero = int(d[pre + "total_nonzero"]), int(d[pre + "total_zero"])
    return SimpleNamespace(d=d, pre=pre, post=post, mask=mask, optim=optim, params=params, names=names, mask_bits=mask_bits,
                           out=out)


def update_captured(c):
    """update_connections() on load_captured()'s model against the reference's state after the update -> c.out"""
    d, post, mask = c.d, c.post, c.mask
    mask.update_connections()
    c.out["device_updates"] = len(mask._pending)
    got_w = np.concatenate([p.detach().cpu().numpy().ravel() for p in c.params])
    got_m = np.concatenate([c.optim.state[p]["exp_avg"].cpu().numpy().ravel() for p in c.params])
    c.out.update(mask_equal=bool(np.array_equal(c.mask_bits(), d[post + "mask"])),
                 w_equal=bool(np.array_equal(got_w.view(np.int32), d[post + "w"].view(np.int32))),
                 m_equal=bool(np.array_equal(got_m.view(np.int32), d[post + "m"].view(np.int32))),
                 nnz_equal=[int(mask.mask_dict[n].sum().item()) for n in c.names] == d[post + "nnz"].tolist(),
                 mask_step_equal=mask.mask_step == int(d[post + "mask_step"]),
                 density_error=abs(mask.stats.total_density - float(d[post + "density"])))
    return c.out


# ---- a whole fit on both routes --------------------------------------------------------------------------------------------
def fit_on_both_routes(workdir, over, method):
    """fit_one under the overrides `over` with SIREN_FIT_DEVICE_MASK=0 and on the device route; `method`: the engine method
    whose calls are the device updates.  -> what result.json and model.pth of the two runs say"""
    from _gpu_child import ROOT
    from implicit_image import _engine as E
    from implicit_image.config import load_config
    from implicit_image.fit import fit_one
    out, calls, plain = {}, [0], getattr(E.SirenEngine, method)

    def counted(self, *a, **kw):
        calls[0] += 1
        return plain(self, *a, **kw)
    setattr(E.SirenEngine, method, counted)
    for side, knob in (("host", "0"), ("device", "1")):
        os.environ[KNOB] = knob
        calls[0] = 0
        cfg = load_config(os.path.join(ROOT, "conf"), over)
        run_dir = os.path.join(workdir, side)
        res = fit_one(cfg, torch.device("cuda", 0), run_dir)
        sd = torch.load(os.path.join(run_dir, "model.pth"), weights_only=True)["state_dict"]
        weights = torch.cat([v.reshape(-1) for k, v in sd.items() if k.endswith("weight")])
        saved = json.load(open(os.path.join(run_dir, "result.json")))
        out[side] = {"device_updates": calls[0], "PSNR": saved["PSNR"], "loss": saved["loss"], "PSNR_8bit": saved["PSNR_8bit"],
                     "density": float((weights != 0).float().mean()), "returned_psnr": res["PSNR"]}
    os.environ.pop(KNOB)
    a, b = (open(os.path.join(workdir, s, "model.pth"), "rb").read() for s in ("host", "device"))
    out["pth_equal"] = a == b
    out["pth_bytes"] = len(a)
    return out


# ---- the engine of the host tests ------------------------------------------------------------------------------------------
class FakeEngine:
    """what Masking asks of an engine, on CPU tensors.  It has neither route, like FourierEngine: a host test overrides the
    method of the route it restates."""
    device = torch.device("cpu")
    mask_update = None
    mask_prune_global = None

    def __init__(self, model):
        self.lib = SimpleNamespace(sf_mask_update=None, sf_mask_prune_global=None)
        self.sizes = [p.numel() for p in model._param_list()]
        self.num_params = sum(self.sizes)
        self.vecs = {w: torch.zeros(self.num_params) for w in ("params", "grads", "exp_avg", "exp_avg_sq", "masks")}
        self.updates = 0
        self.quiet = False

    def view(self, which):
        return self.vecs[which]

    def param_offsets(self, layer):
        off = sum(self.sizes[:2 * layer])
        return off, off + self.sizes[2 * layer]

    def set_masks(self, flat):
        self.vecs["masks"].copy_(flat)

    def params_changed(self):
        pass

    def state_and_slices(self, layers):
        v = self.vecs
        return ([v["params"], v["grads"], v["exp_avg"], v["exp_avg_sq"], v["masks"]],
                [(self.param_offsets(l)[0], self.sizes[2 * l]) for l in layers])
