"""Recording stand-ins for what a training step touches - engine handle, model, optimiser, mask, scheduler - shared by the host
tests of the step routes (test_step_many_host.py, test_step_routes_host.py).  Every stand-in keeps its own `calls`; given a `log`
(one list shared by the stand-ins of a run) it also appends [name, call, arguments ...] there, so the log is the order of the
calls across all of them.  Nothing here touches a device."""
from types import SimpleNamespace

import torch

from implicit_image.utils import train_helper as th


class _Recorder:
    log, name = None, "?"

    def note(self, what, *args):
        self.calls.append((what, *args) if args else what)
        if self.log is not None:
            self.log.append([self.name, what, *args])


class FakeEngine(_Recorder):
    """A handle.  Pass k (from 1) leaves the SSE 4.8 * k.  The views are accessors without effect and are not logged."""

    def __init__(self, log=None, name="eng", lib=None):
        self.log, self.name, self.calls, self.h = log, name, [], 1
        self.lib = lib if lib is not None else SimpleNamespace(sf_step_many=None)
        self.passes = 0

    def forward_backward(self, sync=True):
        self.note("forward_backward", {"sync": sync})
        self.passes += 1
        return 4.8 * self.passes if sync else None

    def sse_view(self):
        return torch.tensor([4.8 * self.passes], dtype=torch.float64)

    def grad_view(self):
        return torch.zeros(1)

    def adam_step(self, lr):
        self.note("adam_step", lr)

    def step(self, lrs, want_loss=False):
        self.note("step", list(lrs), {"want_loss": want_loss})
        return [1.0 / (k + 1) for k in range(len(lrs))]

    def quant_pass(self, args):
        self.note("quant_pass")

    def quant_nudge(self, args):
        self.note("quant_nudge", args.nudge_lr)


class FakeModel(_Recorder):
    row_split = None
    state_is_live = True

    def __init__(self, eng, log=None, name="model"):
        self.eng, self.calls, self.log, self.name = eng, [], log, name
        self.pre_pass_callbacks, self.post_backward_callbacks = [], []
        self.bound_engine = None

    def named_modules(self):
        return []

    def train(self):
        self.note("train")

    def engine(self, grid, img):
        self.note("engine")
        self.bound_engine = self.eng
        for cb in list(self.pre_pass_callbacks):      # (as EngineBound.engine: the pre-pass callbacks run here)
            cb()
        return self.eng

    def download_grads(self):
        self.note("download_grads")


class FakeOptim(_Recorder, th.EngineAdam):
    """(an EngineAdam to train_steps' isinstance check alone: none of its code runs)"""

    def __init__(self, model, log=None, name="optim", lr=1e-3):
        self.model, self.calls, self.log, self.name = model, [], log, name
        self.param_groups, self.defaults = [{"lr": lr}], {"lr": lr}
        self.state = {"p": {"step": 0}}

    def zero_grad(self, set_to_none=True):
        self.note("zero_grad")

    def prepare(self):
        self.note("prepare")
        return self.model.eng

    def count_steps(self, n):
        self.note("count_steps", n)
        self.state["p"]["step"] += n

    def step(self, closure=None):
        self.note("step", self.param_groups[0]["lr"])
        self.state["p"]["step"] += 1


class FakeMask(_Recorder):
    def __init__(self, optim, steps_need_no_host, log=None, name="mask"):
        self.optimizer, self.steps_need_no_host, self.calls, self.log, self.name = optim, steps_need_no_host, [], log, name
        self.mask_step = 0

    def step(self, scaler=None):
        self.note("step", scaler)
        self.optimizer.step()
        self.mask_step += 1

    def push_masks_once(self):
        self.note("push_masks_once")

    def count_steps(self, n):
        self.note("count_steps", n)
        self.mask_step += n


class FakeSched(_Recorder):
    """StepLR(every, 0.5) as far as a step route can tell: step() counts and halves the optimiser's lr"""

    def __init__(self, optim, every=2, log=None, name="sched"):
        self.optim, self.every, self.calls, self.log, self.name = optim, every, [], log, name
        self.last_epoch = 0

    def step(self):
        self.note("step")
        self.last_epoch += 1
        if self.last_epoch % self.every == 0:
            self.optim.param_groups[0]["lr"] *= 0.5
