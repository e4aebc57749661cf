"""Child of tests/test_gpu_binding_trace.py: drives every model family through its binding to an engine handle, in ONE fresh
process, and writes what the models asked of the handles: each call on a handle (method, shapes / dtypes of tensor arguments,
repr of the others, a sha256 of tensor content where the host alone determines it) and, after every scripted step, named
bool / int observations of the binding (pointers inside the engine's views, the optimiser's moments, what a re-made handle
carried over).  No float computed on the device goes into the output, so the parent compares it for equality with
tests/golden/binding_trace.json, which this same file wrote on the binding as it stood before models/binding.py.
Uses only names both sides have."""
import copy

import torch

from _gpu_child import child_main
from _gpu_fixtures import sha
from oracle import siren_oracle as so

LOG = []                       # the running scenario's entries: handle calls and step observations, in order
HANDLES = []                   # every handle a _new_engine made in this scenario (raw, not the proxy)
SHA_ALWAYS = set()             # methods whose tensor arguments are hashed in this scenario
SHA_ONCE = set()               # ... hashed at their first call only


def describe(v, hashed):
    if isinstance(v, torch.Tensor):
        d = {"shape": list(v.shape), "dtype": str(v.dtype)}
        if hashed:
            d["sha256"] = sha(v)
        return d
    return repr(v)


class Proxy:
    """an engine handle that logs every public method call before passing it on; everything else goes straight through"""

    def __init__(self, raw, idx):
        object.__setattr__(self, "_raw", raw)
        object.__setattr__(self, "_idx", idx)

    def __getattr__(self, name):
        v = getattr(self._raw, name)
        if name.startswith("_") or not callable(v):
            return v

        def call(*args, **kwargs):
            hashed = name in SHA_ALWAYS or name in SHA_ONCE
            SHA_ONCE.discard(name)
            LOG.append({"h": self._idx, "call": name, "args": [describe(a, hashed) for a in args],
                        "kwargs": {k: describe(kwargs[k], hashed) for k in sorted(kwargs)}})
            return v(*args, **kwargs)
        return call

    def __setattr__(self, name, value):
        setattr(self._raw, name, value)


def patch(cls):
    orig = cls._new_engine

    def _new_engine(self, H, w, row_begin, row_end, device):
        raw = orig(self, H, w, row_begin, row_end, device)
        HANDLES.append(raw)
        LOG.append({"h": len(HANDLES) - 1, "new_engine": type(self).__name__, "class": type(raw).__name__,
                    "args": [repr(x) for x in (H, w, row_begin, row_end, device)]})
        return Proxy(raw, len(HANDLES) - 1)
    cls._new_engine = _new_engine


def step(name, **obs):
    for k, v in obs.items():
        assert isinstance(v, (bool, int, str)) or (isinstance(v, list) and all(isinstance(x, (bool, int)) for x in v)), (k, v)
    LOG.append({"step": name, "obs": obs})


def refusal(call):
    try:
        call()
    except Exception as e:
        return type(e).__name__ + ": " + str(e)
    return "no exception"


def raw_views(model):
    """(raw handle, its params / grads / exp_avg / exp_avg_sq views as the model's Parameters are laid out in them)"""
    eng = model._engine
    if "base" in vars(eng):                                  # FeatherEngine: the feather vector
        raw = eng.base._raw
        return raw, [raw.feather_view(w) for w in ("params", "grads", "exp_avg", "exp_avg_sq")]
    raw = eng._raw
    return raw, [raw.view(w) for w in ("params", "grads", "exp_avg", "exp_avg_sq")]


def inside(t, view):
    return t is not None and view.data_ptr() <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= view.data_ptr() + 4 * view.numel()


def bound(model):
    """[every p.data inside the params view, every p.grad inside the grads view]"""
    _, (pv, gv, _, _) = raw_views(model)
    ps = model._param_list()
    return [all(inside(p.data, pv) for p in ps), all(inside(p.grad, gv) for p in ps)]


def optim_bound(model, optim):
    _, (_, _, mv, vv) = raw_views(model)
    ps = model._param_list()
    return all("exp_avg" in optim.state[p] and inside(optim.state[p]["exp_avg"], mv)
               and inside(optim.state[p]["exp_avg_sq"], vv) for p in ps)


def adam_state(model):
    """(exp_avg, exp_avg_sq clones, step count as the model's handle reports it, masks clone)"""
    raw, (_, _, mv, vv) = raw_views(model)
    return mv.clone(), vv.clone(), int(model._engine.adam_steps), raw.view("masks").clone()


def has_mask(model):
    return bool(getattr(model, "_has_engine_mask", False))


def pad_zero(model):
    """(are the padded slots of the engine's parameters all zero, how many there are).  After a step they are zero with
    16-bit phases only: with phase bytes (the auto format of a dense fit) a padded neuron outputs sin(2 pi kPhaseEps), the
    weights it feeds get a gradient and Adam moves their slots; the next pass scatters into a zeroed vector again
    (the comment on Siren.WIDTHS), so the answer depends on the scratch format, not on rounding"""
    raw, (pv, _, _, _) = raw_views(model)
    keep = torch.ones(raw.num_params, dtype=torch.bool, device=pv.device)
    keep[model._padded_index(pv.device)] = False
    return bool((pv[keep] == 0).all().item()), int(keep.sum().item())


def calls(name, h=None):
    return sum(1 for e in LOG if e.get("call") == name and (h is None or e["h"] == h))


class Cfg(dict):
    __getattr__ = dict.get


RIGL = Cfg(name="RigL", density=0.5, sparse_init="erdos-renyi-kernel", dense_gradients=True, growth_mode="absolute-gradient",
           prune_mode="magnitude", redistribution_mode="none", dense=False, prune_rate=0.3, decay_schedule="cosine",
           end_when=1000, interval=100)


def data(h, w):
    return so.get_grid(h, w).cuda(), so.synthetic_image(h, w, seed=0).cuda()


def scenario_a():
    from implicit_image.models.siren import Siren
    from implicit_image.utils.train_helper import EngineAdam, setup_mask, train_epoch
    SHA_ALWAYS.update({"set_masks", "set_coords"})
    torch.manual_seed(0)
    grid, img = data(32, 32)
    m = Siren(depth=3, hidden_size=32).cuda()
    m(grid)
    step("A1 forward", bound=bound(m), handles=len(HANDLES), has_mask=has_mask(m))
    opt = EngineAdam(m, lr=3e-4)
    for _ in range(2):
        train_epoch(m, opt, grid, img)
    step("A2 two train_epoch", bound=bound(m), optim_bound=optim_bound(m, opt), adam_steps=adam_state(m)[2], handles=len(HANDLES))
    w = m.layers[1].linear.weight
    w.data = w.data.clone()
    before = bound(m)
    m(grid)
    step("A3 replaced weight.data", bound_before=before, bound=bound(m), handles=len(HANDLES))
    mask = setup_mask(m, opt, RIGL)
    train_epoch(m, opt, grid, img, mask=mask)
    step("A4 RigL", bound=bound(m), optim_bound=optim_bound(m, opt), has_mask=has_mask(m), handles=len(HANDLES),
         set_masks_per_handle=[calls("set_masks", h) for h in range(len(HANDLES))], adam_steps=adam_state(m)[2])
    m0, v0, s0, k0 = adam_state(m)
    m.set_scratch_format(12)
    m.engine(grid, img)
    m1, v1, s1, k1 = adam_state(m)
    step("A5 scratch format 12: rebuilt", handles=len(HANDLES), steps_before=s0, steps_after=s1, exp_avg_equal=torch.equal(m0, m1),
         exp_avg_sq_equal=torch.equal(v0, v1), masks_equal=torch.equal(k0, k1), has_mask=has_mask(m), bound=bound(m),
         optim_bound=optim_bound(m, opt))
    train_epoch(m, opt, grid, img, mask=mask)
    step("A5 train_epoch", bound=bound(m), optim_bound=optim_bound(m, opt), adam_steps=adam_state(m)[2], handles=len(HANDLES),
         set_masks_per_handle=[calls("set_masks", h) for h in range(len(HANDLES))])
    m0, v0, s0, k0 = adam_state(m)
    opt2 = EngineAdam(m, lr=3e-4, betas=(0.8, 0.99))
    m.engine(grid, img)
    m1, v1, s1, k1 = adam_state(m)
    step("A6 second EngineAdam: rebuilt", handles=len(HANDLES), steps_before=s0, steps_after=s1, exp_avg_equal=torch.equal(m0, m1),
         exp_avg_sq_equal=torch.equal(v0, v1), masks_equal=torch.equal(k0, k1), has_mask=has_mask(m), bound=bound(m),
         optim_bound=[optim_bound(m, opt), optim_bound(m, opt2)])
    train_epoch(m, opt2, grid, img)
    step("A6 train_epoch", bound=bound(m), optim_bound=[optim_bound(m, opt), optim_bound(m, opt2)], adam_steps=adam_state(m)[2],
         handles=len(HANDLES))
    grid2, img2 = data(48, 32)
    train_epoch(m, opt2, grid2, img2)
    step("A7 48x32", handles=len(HANDLES), adam_steps=adam_state(m)[2], has_mask=has_mask(m), bound=bound(m),
         optim_bound=[optim_bound(m, opt), optim_bound(m, opt2)], set_masks_per_handle=[calls("set_masks", h) for h in range(len(HANDLES))])
    c = copy.deepcopy(m)
    step("A8 deepcopy", copy_engine_is_none=c._engine is None, model_engine_is_none=m._engine is None, copy_is_cuda=next(c.parameters()).is_cuda,
         copy_has_mask=has_mask(c), copy_adam=repr(c._adam))
    m.half()
    step("A8 half", model_engine_is_none=m._engine is None, dtype=str(m.layers[0].linear.weight.dtype), closes=calls("close"),
         grads_none=all(p.grad is None for p in m._param_list()))


def scenario_b():
    from implicit_image.models.siren import Siren
    from implicit_image.utils.train_helper import EngineAdam, train_epoch
    SHA_ALWAYS.update({"set_coords"})
    SHA_ONCE.update({"set_params"})
    torch.manual_seed(0)
    grid, img = data(32, 32)
    m = Siren(depth=3, hidden_size=20).cuda()
    opt = EngineAdam(m, lr=3e-4)
    for i in range(2):
        train_epoch(m, opt, grid, img)
        zero, slots = pad_zero(m)
        ps = m._param_list()
        step(f"B train_epoch {i + 1}", padded=bool(m._padded), engine_width=int(m._engine_width), bound=bound(m), pad_slots=slots,
             pad_slots_zero=zero, adam_steps=adam_state(m)[2], handles=len(HANDLES),
             grads_are_own_tensors=all(p.grad is not None and p.grad.shape == p.shape for p in ps),
             moments_are_copies=all(tuple(opt.state[p]["exp_avg"].shape) == tuple(p.shape) for p in ps) and not optim_bound(m, opt))


def scenario_c():
    from implicit_image.models.fourier import FourierNet
    from implicit_image.utils.train_helper import EngineAdam, train_epoch
    SHA_ALWAYS.update({"set_coords", "set_encoding"})
    torch.manual_seed(0)
    grid, img = data(32, 24)
    m = FourierNet(depth=4, hidden_size=32, map_size=64).cuda()
    m(grid)
    opt = EngineAdam(m, lr=3e-4)
    train_epoch(m, opt, grid, img)
    step("C1 forward, train_epoch", bound=bound(m), optim_bound=optim_bound(m, opt), handles=len(HANDLES), set_encoding=calls("set_encoding"),
         adam_steps=adam_state(m)[2])
    m.encoding.B.mul_(1.0)
    m(grid)
    m(grid)
    step("C2 version bump", set_encoding=calls("set_encoding"), handles=len(HANDLES), bound=bound(m))
    step("C3 row range", refusal=refusal(lambda: m.engine(grid, row_begin=1)), handles=len(HANDLES))


def scenario_d():
    from implicit_image.models.wavelet_siren import WaveletSiren
    from implicit_image.utils.train_helper import EngineAdam, train_epoch
    torch.manual_seed(0)                  # (set_coords is not hashed here: the coefficient grid is a device linspace)
    grid, img = data(16, 16)
    m = WaveletSiren(depth=3, hidden_size=32).cuda()
    m(grid)
    opt = EngineAdam(m, lr=3e-4)
    train_epoch(m, opt, grid, img)
    step("D1 forward, train_epoch", bound=bound(m), optim_bound=optim_bound(m, opt), handles=len(HANDLES), adam_steps=adam_state(m)[2],
         LF_h=int(m.LF_h))
    grid2, _ = data(20, 20)
    step("D2 20x20", refusal=refusal(lambda: m(grid2)), handles=len(HANDLES), LF_h=int(m.LF_h))
    step("D3 row range", refusal=refusal(lambda: m.engine(grid, row_begin=2)), handles=len(HANDLES))


def scenario_e():
    from implicit_image.models.siren import Siren
    from implicit_image.pipeline.feathermap.feathernet import FeatherNet
    from implicit_image.utils.train_helper import EngineAdam, train_epoch
    SHA_ALWAYS.update({"set_coords"})
    torch.manual_seed(0)
    grid, img = data(32, 32)
    m = FeatherNet(Siren(depth=3, hidden_size=32), compress=0.5).cuda()
    opt = EngineAdam(m, lr=3e-4)
    for _ in range(2):
        train_epoch(m, opt, grid, img)
    step("E1 two train_epoch", bound=bound(m), optim_bound=optim_bound(m, opt), adam_steps=adam_state(m)[2], handles=len(HANDLES),
         scratch_format=int(m.cfg["scratch_format"]), feather_attach_per_handle=[calls("feather_attach", h) for h in range(len(HANDLES))],
         dense_weights_are_tensors=all(not isinstance(l.linear.weight, torch.nn.Parameter) for l in m.module.layers))
    m0, v0, s0, _ = adam_state(m)
    m.set_scratch_format(12)
    m.engine(grid, img)
    m1, v1, s1, _ = adam_state(m)
    step("E2 scratch format 12: rebuilt", handles=len(HANDLES), steps_before=s0, steps_after=s1, exp_avg_equal=torch.equal(m0, m1),
         exp_avg_sq_equal=torch.equal(v0, v1), bound=bound(m), optim_bound=optim_bound(m, opt),
         feather_attach_per_handle=[calls("feather_attach", h) for h in range(len(HANDLES))])
    train_epoch(m, opt, grid, img)
    step("E2 train_epoch", bound=bound(m), optim_bound=optim_bound(m, opt), handles=len(HANDLES), closes=calls("close"))


def case_binding_trace():
    torch.cuda.init()
    from implicit_image.models.fourier import FourierNet
    from implicit_image.models.siren import Siren
    from implicit_image.models.wavelet_siren import WaveletSiren
    for cls in (Siren, FourierNet, WaveletSiren):
        patch(cls)
    res = {}
    for name, run in (("A", scenario_a), ("B", scenario_b), ("C", scenario_c), ("D", scenario_d), ("E", scenario_e)):
        del LOG[:], HANDLES[:]
        SHA_ALWAYS.clear()
        SHA_ONCE.clear()
        run()
        torch.cuda.synchronize()
        res[name] = list(LOG)
        print(name, len(LOG), "entries,", len(HANDLES), "handles", flush=True)
    return res


def case_step_paths():
    """train_steps(n = 4) on a Siren against four train_epoch calls on a deep copy of it made before the first step, both under
    lr 3e-4 with StepLR(2, 0.5), at width 32 (live state) and 20 (padded to 32), without masks and under RigL at density 0.5
    with dense and with sparse gradients: everything a step leaves behind on either side, and which calls on a handle ran"""
    from implicit_image import _engine
    from implicit_image.models.siren import Siren
    from implicit_image.utils.train_helper import EngineAdam, setup_mask, train_epoch, train_steps
    torch.cuda.init()
    ran = {"step": 0, "forward_backward": 0}
    for name in ran:
        def counted(self, *args, _name=name, _plain=getattr(_engine.SirenEngine, name), **kwargs):
            ran[_name] += 1
            return _plain(self, *args, **kwargs)
        setattr(_engine.SirenEngine, name, counted)
    grid, img = data(16, 16)
    masks = {"none": None, "dense": RIGL, "sparse": Cfg(RIGL, dense_gradients=False)}
    res = {}
    for hidden in (32, 20):
        for tag, mcfg in masks.items():
            torch.manual_seed(0)
            first = Siren(depth=3, hidden_size=hidden).cuda()
            sides = []
            for m in (first, copy.deepcopy(first)):
                torch.manual_seed(1)                             # the masks' initial draw: the same on both sides
                opt = EngineAdam(m, lr=3e-4)
                sched = torch.optim.lr_scheduler.StepLR(opt, 2, gamma=0.5)
                sides.append((m, opt, sched, setup_mask(m, opt, mcfg) if mcfg else None))
            out, calls_of = [], []
            for bulk, (m, opt, sched, mask) in zip((True, False), sides):
                before = dict(ran)
                if bulk:
                    losses = train_steps(m, opt, grid, img, 4, lr_scheduler=sched, mask=mask)
                else:
                    losses = [train_epoch(m, opt, grid, img, lr_scheduler=sched, mask=mask) for _ in range(4)]
                torch.cuda.synchronize()
                calls_of.append({k: ran[k] - before[k] for k in ran})
                out.append({"losses": [float(x) for x in losses], "optim_step": [float(opt.state[p]["step"]) for p in m._param_list()],
                            "lr": float(opt.param_groups[0]["lr"]), "last_epoch": int(sched.last_epoch),
                            "mask_step": None if mask is None else int(mask.mask_step),
                            "prune_rate": None if mask is None else float(mask.prune_rate)})
            (a, _, _, ka), (b, _, _, kb) = sides
            res[f"{hidden}_{tag}"] = {
                "live": bool(a.state_is_live), "train_steps": out[0], "train_epochs": out[1], "calls": calls_of,
                "params_equal": [bool(torch.equal(p.data, q.data)) for p, q in zip(a._param_list(), b._param_list())],
                "masks_equal": ka is None or all(bool(torch.equal(ka.mask_dict[n], kb.mask_dict[n])) for n in ka.mask_dict),
                "density": None if ka is None else float(ka.flat_mask().mean().item())}
    return res


if __name__ == "__main__":
    child_main({"binding_trace": case_binding_trace, "step_paths": case_step_paths})
