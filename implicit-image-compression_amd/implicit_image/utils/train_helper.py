"""Step harness with the reference's signatures (reference: implicit_image/utils/train_helper.py).

  train_epoch(model, optim, grid, img, **kwargs) -> float          (:132-185)
  eval_epoch(model, grid, img, **kwargs) -> (pred, loss, PSNR, PSNR_8bit)   (:41-59)
  eval_metrics(model, grid, img) -> (loss, PSNR, PSNR_8bit)       eval_epoch's figures without its prediction (sf_eval)
  train_steps_many(models, optims, grid, imgs, n, lr_schedulers, masks) -> list of loss lists    train_steps for several
                                                                       fits of one shape at once (sf_step_many)
  get_optimizer_lr_scheduler(model, optim_cfg, quantize_mode=False)  (:69-86)
  setup_mask(model, optim, masking_cfg)                               (:89-129)
  get_device(device_str)                                               (:62-66)

One `train_epoch` is one full-batch fit step executed by the HIP engine: forward + MSE + backward
(sf_forward_backward) and Adam(+mask) (sf_adam_step through the optimiser facade).

Every way of running n steps is train_epoch called n times, bit for bit, and shares its pieces: _step (the body of a step around
a route's pass), _run_ahead (the bookkeeping of n steps the device runs alone), _unsupported (what every route refuses).  The
routes: train_steps' docstring and DESIGN.md section 13.
"""
import contextlib
import logging
import math
from typing import Dict, Tuple

import torch
from torch.nn import Module, functional as F
from torch.optim import Optimizer

from .. import _engine
from ..parallel import SseTable, as_float
from ..pipeline.masking import Masking, decay_registry
from ..pipeline.quant.kmeans import KmeansQuant

# what a fit split by image rows (train.pixel_split) refuses, here and - before any GPU work - in fit.check_pixel_split
SPLIT_PADDED_UNSUPPORTED = ("pixel-split with a zero-padded width is not built: the padded layout's Parameters and .grad are "
                            "gathered copies, not the handle's vectors that the ranks reduce in place and the device topology "
                            "routes read; use a hidden size the kernels are instantiated for")
SPLIT_EVAL_EPOCH_UNSUPPORTED = ("train.device_eval=off under pixel-split: eval_epoch needs the whole prediction, a rank holds "
                                "its rows alone; use train.device_eval=auto")


class EngineAdam(Optimizer):
    """torch.optim.Optimizer facade over the engine's fused Adam kernel (Seam 3).

    `state[p]["exp_avg"/"exp_avg_sq"]` are views of the engine's moment buffers,
    `defaults["lr"]` / `param_groups[0]["lr"]` behave as in torch.optim.Adam (StepLR edits them),
    `zero_grad()` is a no-op (the engine overwrites the gradient every backward)."""

    applies_engine_mask = True

    def __init__(self, model: Module, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0, amsgrad: bool = False):
        if weight_decay != 0 or amsgrad:
            raise NotImplementedError("EngineAdam supports weight_decay=0, amsgrad=False (reference defaults)")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and eps >= 0.0):
            raise ValueError(f"invalid Adam hyper-parameters betas={betas} eps={eps}")
        self.model = model
        model.set_adam_hparams(tuple(float(b) for b in betas), float(eps))   # sf_config.beta1/beta2/eps of the engine
        super().__init__(model._param_list(), dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False))
        self._bound = None
        model.register_optimizer(self)        # engine() rebinds it when it re-creates the handle

    def _bind_state(self, eng, again=False):
        """state[p]["exp_avg" / "exp_avg_sq"]: the model's moments on `eng`, taken once per handle unless `again` (the binding's
        hooks around the device step say when: models/binding.py)"""
        if self._bound is not eng or again:
            for p, (m, v) in zip(self.model._param_list(), self.model.adam_moments()):
                self.state[p].setdefault("step", torch.tensor(0.0))
                self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"] = m, v
            self._bound = eng

    def handle_changed(self):
        """the model's engine() re-made its handle: what is held belongs to the old one"""
        self._bound = None
        self.prepare()

    def prepare(self):
        """the binding's share before the device step(s) -> the handle they run on"""
        eng = self.model.bound_engine
        if eng is None:
            raise RuntimeError("EngineAdam.step() before any forward/backward: the engine is created by train_epoch")
        self.model.before_optimizer_step(self._bind_state)
        return eng

    def count_steps(self, n: int):
        """the host's bookkeeping of `n` device steps: state[p]["step"], and the mark lr_scheduler.step() looks for"""
        self._opt_called = True              # (what the scheduler's wrapper around Optimizer.step() records)
        for p in self.model._param_list():
            self.state[p]["step"] += n

    def zero_grad(self, set_to_none: bool = True):
        return None

    @torch.no_grad()
    def step(self, closure=None):
        eng = self.prepare()
        eng.adam_step(float(self.param_groups[0]["lr"]))
        self.model.after_optimizer_step(self._bind_state)
        self.count_steps(1)


def get_device(device_str: str) -> torch.device:
    if device_str == "cuda" and torch.cuda.is_available():
        return torch.device(device_str)
    return torch.device("cpu")


def get_optimizer_lr_scheduler(model: Module, optim_cfg: Dict, quantize_mode: bool = False
                               ) -> Tuple[Optimizer, torch.optim.lr_scheduler._LRScheduler]:
    """Adam (conf/optim/adam.yaml) + StepLR(2000, 0.5), StepLR(1000, 0.5) in the quantise phase."""
    name = optim_cfg["name"] if isinstance(optim_cfg, dict) else optim_cfg.name
    kwargs = {k: v for k, v in dict(optim_cfg).items() if k != "name"}
    if name != "adam":
        raise NotImplementedError(f"optimiser '{name}': only 'adam' is on the accelerated path")
    optim = EngineAdam(model, **kwargs)
    lr_scheduler = torch.optim.lr_scheduler.StepLR(optim, 1000 if quantize_mode else 2000, gamma=0.5)
    return optim, lr_scheduler


def _cfg_get(cfg, key, default=None):
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


def setup_mask(model: Module, optim: Optimizer, masking_cfg=None) -> Masking:
    """Masking instance wrapping `model`, or None for dense fits (reference :89-129)."""
    if not masking_cfg or _cfg_get(masking_cfg, "dense"):
        return None
    if model.mask_unsupported:      # FourierNet: the reference itself fails here (models/fourier.py)
        raise NotImplementedError(model.mask_unsupported)
    schedule = _cfg_get(masking_cfg, "decay_schedule")
    if schedule not in decay_registry:
        raise NotImplementedError(f"decay_schedule '{schedule}' is outside the accelerated RigL path")
    if schedule == "magnitude-prune":                                              # reference :100-106
        decay = decay_registry[schedule](final_sparsity=1 - _cfg_get(masking_cfg, "final_density"),
                                         T_max=_cfg_get(masking_cfg, "end_when"),
                                         T_start=_cfg_get(masking_cfg, "start_when"),
                                         interval=_cfg_get(masking_cfg, "interval"))
    else:
        decay = decay_registry[schedule](prune_rate=_cfg_get(masking_cfg, "prune_rate"),
                                         T_max=_cfg_get(masking_cfg, "end_when"))
    mask = Masking(optim, decay, input_size=(1, 1, 2), density=_cfg_get(masking_cfg, "density"),
                   dense_gradients=_cfg_get(masking_cfg, "dense_gradients"),
                   sparse_init=_cfg_get(masking_cfg, "sparse_init"), prune_mode=_cfg_get(masking_cfg, "prune_mode"),
                   growth_mode=_cfg_get(masking_cfg, "growth_mode"),
                   redistribution_mode=_cfg_get(masking_cfg, "redistribution_mode"))
    # Topology updates rank weight.grad entries against each other (grow.py:86-95).  With phase bytes the candidates'
    # small gradients carry relatively more quantisation noise, the masks drift from the reference's, and the settled
    # PSNR of the config-4 fixture moves by +0.19 dB (criterion: 0.05; with unorm16 phases it holds).  Masked fits
    # therefore run with unorm16 phases unless the model was built with an explicit format.  (Exact-zero gradients -
    # ties the sort resolves arbitrarily - no longer occur with phase bytes: kPhaseEps in siren_kernels.hip.)
    # ONE rule, the engine's own (sf_set_masks moves every auto handle to 16 when a mask is set): an auto model is created
    # with format 16 here, so the engine never allocates the 8-bit scratch first only to free it at the first mask push.
    # An EXPLICIT 8 or 12 stays as given on both sides (topology updates with it are unsupported: DESIGN.md section 2).
    if model.cfg.get("scratch_format", 0) == 0:
        model.set_scratch_format(16)
    model.train()
    mask.add_module(model)
    return mask


def _unsupported(kwargs):
    """why the engine cannot take these keyword arguments of a step, else None: the one statement of what every route refuses.
    'scaler' / 'context' are accepted and ignored: autocast is never entered by the reference (train_helper.py:141) and
    GradScaler is an exact no-op on fp32 gradients."""
    if kwargs.get("criterion", F.mse_loss) is not F.mse_loss:
        return "the engine fuses F.mse_loss (reduction='mean'); other criteria are not supported"
    if kwargs.get("preconditioner") is not None:
        return "preconditioners (EKFAC) are dead code in the reference and not supported"
    return None


def _step(model: Module, optim: Optimizer, grid, img, the_pass, **kwargs):
    """The one body of a step on the host, around `the_pass(eng)` - what a route does between binding the handle and looking
    at the gradient - whose result it returns: model.train, zero_grad, engine() (the pre-pass callbacks of a quantise phase run
    there: sf_quant_pass), the pass, download_grads (a no-op unless the width is zero-padded), the post-backward callbacks,
    mask.step() or optim.step(), pbar, the scheduler."""
    mask, pbar, lr_scheduler = kwargs.get("mask"), kwargs.get("pbar"), kwargs.get("lr_scheduler")
    model.train()
    optim.zero_grad()
    out = the_pass(model.engine(grid, img))
    model.download_grads()
    for cb in list(model.post_backward_callbacks):
        cb()
    if mask:
        mask.step(kwargs.get("scaler"))
    else:
        optim.step()
    if pbar:
        pbar.update(1)
    if lr_scheduler:
        lr_scheduler.step()
    return out


def _run_ahead(optim: Optimizer, lr_scheduler, n: int):
    """The host's bookkeeping of `n` steps that the device runs without it -> their n learning rates"""
    optim.count_steps(n)                     # (first: the scheduler looks for the optimiser's mark at its first step)
    lrs = []
    for _ in range(n):                       # the schedule is host-side bookkeeping: run it ahead
        lrs.append(float(optim.param_groups[0]["lr"]))
        if lr_scheduler:
            lr_scheduler.step()
    return lrs


def train_epoch(model: Module, optim: Optimizer, grid, img, **kwargs) -> float:
    """One full-batch optimiser step; returns the loss of the step like `train_loss.item()`."""
    if getattr(model, "row_split", None) is not None:
        return _split_steps(model, optim, grid, img, 1, **kwargs)[0]
    why = _unsupported(kwargs)
    if why:
        raise NotImplementedError(why)
    sse = _step(model, optim, grid, img, lambda eng: eng.forward_backward(sync=True), **kwargs)
    # a float's value, as `.item()` of the reference's float32 loss is and as sf_step reports a step's: (float)(sse / n)
    return as_float(sse / (img.shape[0] * img.shape[1] * img.shape[2]))


def _split_steps(model: Module, optim: Optimizer, grid, img, n: int, **kwargs):
    """`n` steps of a fit split by image rows (model.row_split, a parallel.RowSplit; grid / img: this rank's rows), returned as
    the list of their losses: (float)(sse / n) of the FULL image, the same on every rank.

    A step is train_epoch's (_step) with the reduction where the loss used to be read: split.reduce_pass - the pass enqueued,
    the in-place all-reduce of the handle's own gradient view and SSE double.  Nothing is read per step: every step's reduced
    SSE is copied into a table on the device, and the table is read once after the last step.  The bulk calls (sf_step,
    sf_quant_step) are not used: a collective cannot run inside them.  A world of one reduces nothing and is, kernel for
    kernel, the step-by-step loop the bulk calls are bit-identical to."""
    why = _unsupported(kwargs)
    if why:
        raise NotImplementedError(why)
    if not model.state_is_live:
        raise NotImplementedError(SPLIT_PADDED_UNSUPPORTED)
    split, table = model.row_split, SseTable(n)
    for k in range(n):
        # (the reduced SSE into the table before the next pass overwrites it)
        _step(model, optim, grid, img, lambda eng: table.put(k, split.reduce_pass(eng)), **kwargs)
    return [as_float(sse / split.n_values(img)) for sse in table.read()]


def _quant_phase(model: Module, optim: Optimizer):
    """the KmeansQuant whose two callbacks are the model's only ones and which steps `optim`, when it wants the device route:
    the quantise phase as train_steps can hand it to sf_quant_step once the handle is there.  Else None."""
    post = model.post_backward_callbacks
    kq = getattr(post[0], "__self__", None) if len(post) == 1 else None
    return kq if (isinstance(kq, KmeansQuant) and kq.is_whole_phase_of(model, optim) and kq.device_wanted()) else None


def _plain(model: Module, optim: Optimizer, **kwargs) -> bool:
    """the engine's own state, optimiser and loss: what both bulk routes of train_steps need"""
    return model.state_is_live and isinstance(optim, EngineAdam) and _unsupported(kwargs) is None


def _bulk(model: Module, optim: Optimizer, n: int, **kwargs) -> bool:
    """train_steps' condition for handing n steps to the engine in one sf_step call: nothing on the host has to look at the
    state between two steps"""
    mask = kwargs.get("mask")
    return (n > 1 and _plain(model, optim, **kwargs) and not model.post_backward_callbacks
            and (mask is None or mask.steps_need_no_host))


def train_steps(model: Module, optim: Optimizer, grid, img, n: int, **kwargs):
    """`n` consecutive train_epoch() calls, returned as the list of their losses, by the first route that applies.  Every route
    runs the same kernels in the same order, so each is bit-identical to the step-by-step loop.

      split          model.row_split is set (train.pixel_split)                          _step per step, a collective in each
      quantise       n >= 1, _plain, no mask, the model's only callbacks are one         _run_ahead, ONE sf_quant_step (the nudge
                     KmeansQuant's and it has a device plan on the bound handle          at optim.defaults["lr"], as the reference)
      bulk           _bulk: nothing on the host looks at the state between two steps     _run_ahead, ONE sf_step
      step by step   otherwise                                                           train_epoch per step

    The reference loop (compress.py:137-170) syncs with the device every iteration for `train_loss.item()`; on the two
    one-call routes the stream never drains and the losses come back in one read."""
    if getattr(model, "row_split", None) is not None:
        return _split_steps(model, optim, grid, img, n, **kwargs)
    mask: Masking = kwargs.get("mask")
    lr_scheduler = kwargs.get("lr_scheduler")
    pbar = kwargs.get("pbar")
    kq = _quant_phase(model, optim) if (_plain(model, optim, **kwargs) and n >= 1 and mask is None) else None
    if kq is not None:
        model.train()
        if kq.bind_handle(grid, img) is None:      # (a handle without the entry points: step by step, the callbacks as ever)
            kq = None
    if kq is not None:
        optim.prepare()
        losses = kq.device_steps(_run_ahead(optim, lr_scheduler, n), want_loss=True)
    elif not _bulk(model, optim, n, **kwargs):
        return [train_epoch(model, optim, grid, img, **kwargs) for _ in range(n)]
    else:
        model.train()
        model.engine(grid, img)
        eng = optim.prepare()
        if mask is not None:
            mask.push_masks_once()
        losses = eng.step(_run_ahead(optim, lr_scheduler, n), want_loss=True)
        if mask is not None:
            mask.count_steps(n)
    if pbar:
        pbar.update(n)
    return losses


# what train_steps_many did, for callers that report it (fit.py logs it per group; tests read it): batched calls, the steps
# they took (per member), and groups that went member by member
MANY_STATS = {"calls": 0, "steps": 0, "fallbacks": 0}
_many_fallback_logged = set()


def train_steps_many(models, optims, grid, imgs, n: int, lr_schedulers=None, masks=None, scopes=None):
    """train_steps(models[b], optims[b], grid, imgs[b], n, lr_scheduler=lr_schedulers[b], mask=masks[b]) for every member b,
    returned as the list of their loss lists.

    When every member meets train_steps' own bulk condition (_bulk: the n steps of a member would be ONE sf_step), the library
    has sf_step_many and the handles pass its checks (one shape, hidden <= 128, fp16 operands, scratch format 16, one chunk,
    the whole picture, one stream: include/siren_fit.h), the n steps of ALL members are one sf_step_many call: every kernel of
    a step is launched once for all of them, and each member ends bit for bit where its own sf_step would.  The host
    bookkeeping per member is train_steps': optim.prepare, mask.push_masks_once, _run_ahead (the member's column of the lrs).
    Otherwise train_steps once per member, in order; why is logged once per reason.

    scopes: one callable per member that returns a context manager, entered around that member's host work (fit.py: the
    member's random state); default: none."""
    B = len(models)
    lr_schedulers = list(lr_schedulers) if lr_schedulers is not None else [None] * B
    masks = list(masks) if masks is not None else [None] * B
    scopes = list(scopes) if scopes is not None else [contextlib.nullcontext] * B
    if not (len(optims) == len(imgs) == len(lr_schedulers) == len(masks) == len(scopes) == B):
        raise ValueError("train_steps_many: one optimiser, picture, scheduler, mask and scope per model")

    def one_by_one(why):
        if why not in _many_fallback_logged:
            _many_fallback_logged.add(why)
            logging.info(f"train_steps_many: member by member ({why})")
        MANY_STATS["fallbacks"] += 1
        out = []
        for b in range(B):
            with scopes[b]():
                out.append(train_steps(models[b], optims[b], grid, imgs[b], n, lr_scheduler=lr_schedulers[b], mask=masks[b]))
        return out

    if B == 0:
        return []
    if B == 1:      # measured (profiles/step_many_bench.json): one fit through the tables is slower than its own eager sf_step
        with scopes[0]():
            return [train_steps(models[0], optims[0], grid, imgs[0], n, lr_scheduler=lr_schedulers[0], mask=masks[0])]
    if any(getattr(m, "row_split", None) is not None for m in models):
        return one_by_one("a fit split by image rows")
    if not all(_bulk(models[b], optims[b], n, mask=masks[b]) for b in range(B)):
        return one_by_one("a member's steps need the host between them, or fewer than two steps")
    if B > _engine.STEP_MANY_MAX:
        return one_by_one(f"more than {_engine.STEP_MANY_MAX} members")
    engines = []
    for b in range(B):
        with scopes[b]():
            models[b].train()
            models[b].engine(grid, imgs[b])
            engines.append(optims[b].prepare())
            if masks[b] is not None:
                masks[b].push_masks_once()
    if not _engine.has_step_many(engines[0].lib):
        return one_by_one("the library has no sf_step_many entry point: rebuild it")
    why = _engine.step_many_refusal(engines)
    if why is not None:
        return one_by_one(why)
    columns = [_run_ahead(optims[b], lr_schedulers[b], n) for b in range(B)]      # member by member, each its own schedule
    lrs = [list(row) for row in zip(*columns)]
    losses = _engine.step_many(engines, lrs, want_loss=True)
    for b in range(B):
        if masks[b] is not None:
            masks[b].count_steps(n)
    MANY_STATS["calls"] += 1
    MANY_STATS["steps"] += n
    return losses


@torch.no_grad()
def eval_epoch(model: Module, grid, img, **kwargs) -> Tuple[torch.Tensor, float, float, float]:
    if getattr(model, "row_split", None) is not None:
        raise NotImplementedError(SPLIT_EVAL_EPOCH_UNSUPPORTED)
    model.eval()
    eng = model.engine(grid, img)
    pred, sse = eng.forward(want_pred=True, want_sse=True)
    test_loss = sse / img.numel()
    test_PSNR = 10 * math.log10(1 / test_loss)
    img_8bit = (img * 255).int()
    pred_8bit = (pred * 255).int()
    mse_8bit = ((img_8bit - pred_8bit) ** 2).float().mean()
    test_PSNR_8bit = 10 * torch.log10(255 ** 2 / mse_8bit)
    return pred, test_loss, test_PSNR, test_PSNR_8bit.item()


def device_eval_wanted(setting) -> bool:
    """train.device_eval (conf/config.yaml): 'auto' -> True, 'off' -> False.  A bare `off` arrives as YAML's false."""
    text = {False: "off", True: "auto", None: "auto"}.get(setting, setting)
    if text not in ("auto", "off"):
        raise ValueError(f"train.device_eval: 'auto' (sf_eval where the handle has it) or 'off', got {setting!r}")
    return text == "auto"


@torch.no_grad()
def eval_metrics(model: Module, grid, img) -> Tuple[float, float, float]:
    """(loss, PSNR, PSNR_8bit) of eval_epoch without its prediction: one sf_eval pass (eng.eval_sums()) whose kernels store
    no picture, no torch arithmetic, no torch allocation, one read.  loss and PSNR are eval_epoch's floats (the same double
    from the same partials in the same order).  PSNR_8bit is 10 log10(255^2 / (sse8 / n)) in Python doubles from the exact
    integer sum, where eval_epoch takes torch's fp32 mean and fp32 log10: the two agree to about 1e-5 dB.
    A library or a handle class without the entry point: eval_epoch(...)[1:]."""
    split = getattr(model, "row_split", None)
    model.eval()
    eng = model.engine(grid, img)             # (as eval_epoch: the pre-pass callbacks of a quantise phase run here)
    if not (callable(getattr(eng, "eval_sums", None)) and _engine.has_eval(eng.lib)):
        return eval_epoch(model, grid, img)[1:]
    if split is not None:                     # this rank's rows; the double and the exact integer sum add up over the ranks
        eng.eval_sums(sync=False)
        sse, sse8 = split.reduce_eval(eng)
        n = split.n_values(img)
    else:
        sse, sse8 = eng.eval_sums()
        n = img.numel()
    test_loss = sse / n
    test_PSNR = 10 * math.log10(1 / test_loss)
    test_PSNR_8bit = 10 * math.log10(255 ** 2 / (sse8 / n)) if sse8 else math.inf
    return test_loss, test_PSNR, test_PSNR_8bit
