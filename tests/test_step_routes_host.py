"""The order of the host's calls on every route that runs n training steps, without a GPU: each route is driven for n = 3 on the
recording stand-ins of tests/_step_fakes.py, and what it called - on engine, model, optimiser, mask and scheduler, in order, with
the arguments - is compared with tests/golden/step_routes_trace.json, beside the returned losses and the counters the routes
keep (the optimiser's state[p]["step"], the scheduler's last_epoch, mask.mask_step).  Every route is promised bit-identical to
train_epoch called n times, so a slip in the order would be silent on the host; the GPU tests compare the results.

    python tests/test_step_routes_host.py        # writes the golden file from the tree it runs in
"""
import json
import os
import sys
from types import SimpleNamespace
from unittest import mock

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "implicit-image-compression_amd")]

from _step_fakes import FakeEngine, FakeMask, FakeModel, FakeOptim, FakeSched  # noqa: E402
from implicit_image import _engine  # noqa: E402
from implicit_image.parallel import RowSplit  # noqa: E402
from implicit_image.pipeline.quant.kmeans import KmeansQuant  # noqa: E402
from implicit_image.utils import train_helper as th  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_routes_trace.json")
N = 3
GRID, IMG = torch.zeros(4, 4, 2), torch.zeros(4, 4, 3)          # 48 values: pass k of a FakeEngine is the loss (float)(0.1 k)


class PlannedQuant(KmeansQuant):
    """A KmeansQuant (train_steps looks for the class) over no layer, whose device plan is a stand-in: the handle's quant_pass /
    quant_nudge and the bulk call are logged."""

    def __init__(self, model, optim, log):
        super().__init__(model, optim, bits=5, skip_ll=())
        self.log = log
        self.args = SimpleNamespace(_keep=(None, None, [], [], []), nudge_lr=None)

    def device_wanted(self):
        return True

    def device_plan(self):
        eng = self.model.bound_engine
        return None if eng is None else (eng, self.args)

    def device_steps(self, lrs, want_loss=True):
        self.log.append(["quant", "device_steps", list(lrs), {"want_loss": want_loss}])
        return [2.0 / (k + 1) for k in range(len(lrs))]


class Rig:
    """one fit's stand-ins on one log"""

    def __init__(self, log, tag="", mask=None, sched=True):
        self.eng = FakeEngine(log, "eng" + tag)
        self.model = FakeModel(self.eng, log, "model" + tag)
        self.optim = FakeOptim(self.model, log, "optim" + tag, lr=2e-3 if tag == "1" else 1e-3)
        self.sched = FakeSched(self.optim, 2, log, "sched" + tag) if sched else None
        self.mask = FakeMask(self.optim, mask, log, "mask" + tag) if mask is not None else None

    def kwargs(self):
        return dict(lr_scheduler=self.sched, mask=self.mask)

    def counters(self):
        return {"optim_step": self.optim.state["p"]["step"], "last_epoch": self.sched.last_epoch if self.sched else None,
                "mask_step": self.mask.mask_step if self.mask else None, "lr": self.optim.param_groups[0]["lr"]}


def one(run, **rig):
    log = []
    r = Rig(log, **rig)
    losses = run(r, log)
    return {"calls": log, "losses": losses, **r.counters()}


def epochs(r, log):
    return [th.train_epoch(r.model, r.optim, GRID, IMG, **r.kwargs()) for _ in range(N)]


def steps(r, log):
    return th.train_steps(r.model, r.optim, GRID, IMG, N, **r.kwargs())


def with_callback(r, log):
    r.model.post_backward_callbacks.append(lambda: log.append(["callback", "post_backward"]))
    return steps(r, log)


def quantise(r, log):
    PlannedQuant(r.model, r.optim, log)
    return steps(r, log)


def split(r, log):
    r.model.row_split = RowSplit(4, rank=0, world=1)
    return steps(r, log)


def split_epoch(r, log):
    r.model.row_split = RowSplit(4, rank=0, world=1)
    return epochs(r, log)


def many(refusal, mask=None):
    log = []
    rigs = [Rig(log, tag, mask=mask) for tag in ("0", "1")]

    def step_many(engines, lrs, want_loss):
        log.append(["_engine", "step_many", [e.name for e in engines], lrs, {"want_loss": want_loss}])
        return [[0.5 / (k + 1) for k in range(len(lrs))] for _ in engines]
    with mock.patch.object(_engine, "step_many_refusal", lambda engines: refusal), \
         mock.patch.object(_engine, "step_many", step_many), mock.patch.dict(th.MANY_STATS):
        losses = th.train_steps_many([r.model for r in rigs], [r.optim for r in rigs], GRID, [IMG, IMG], N,
                                     lr_schedulers=[r.sched for r in rigs], masks=[r.mask for r in rigs])
        stats = dict(th.MANY_STATS)
    return {"calls": log, "losses": losses, "members": [r.counters() for r in rigs], "stats": stats}


def trace():
    with mock.patch.dict(th.MANY_STATS, {"calls": 0, "steps": 0, "fallbacks": 0}):
        return {
            "train_epoch x3": one(epochs),
            "train_epoch x3, mask": one(epochs, mask=False),
            "train_epoch x3, no scheduler": one(epochs, sched=False),
            "train_steps, step by step (post-backward callback)": one(with_callback),
            "train_steps, step by step (mask needs the host)": one(steps, mask=False),
            "train_steps, sf_step": one(steps),
            "train_steps, sf_step, mask": one(steps, mask=True),
            "train_steps, quantise": one(quantise),
            "train_steps, split (world 1)": one(split),
            "train_steps, split (world 1), mask": one(split, mask=True),
            "train_epoch x3, split (world 1)": one(split_epoch),
            "train_steps_many, batched": many(None),
            "train_steps_many, batched, masks": many(None, mask=True),
            "train_steps_many, member by member": many("sf_step_many: member 0: scratch format 12"),
        }


def test_every_route_calls_what_it_called_in_the_same_order():
    want = json.load(open(GOLDEN))
    got = json.loads(json.dumps(trace()))
    assert sorted(got) == sorted(want)
    for route in want:
        assert got[route] == want[route], route


def test_the_routes_agree_with_train_epoch():
    """what the trace itself shows: every single-fit route ends with train_epoch's counters, and the step-by-step ones with its
    losses and its calls"""
    t = trace()
    base = t["train_epoch x3"]
    for route in ("train_steps, step by step (post-backward callback)", "train_steps, sf_step", "train_steps, quantise",
                  "train_steps, split (world 1)"):
        assert {k: t[route][k] for k in ("optim_step", "last_epoch", "lr")} == {k: base[k] for k in ("optim_step", "last_epoch", "lr")}
    assert t["train_epoch x3"]["losses"] == t["train_steps, split (world 1)"]["losses"] == t["train_epoch x3, split (world 1)"]["losses"]
    assert t["train_steps, step by step (mask needs the host)"] == t["train_epoch x3, mask"]
    assert t["train_steps, sf_step, mask"]["mask_step"] == t["train_epoch x3, mask"]["mask_step"] == N
    for b, member in enumerate(t["train_steps_many, batched"]["members"]):
        assert member == t["train_steps_many, member by member"]["members"][b]


def test_a_criterion_or_preconditioner_is_refused_on_every_route():
    r = Rig([])
    for kw, text in ((dict(criterion=torch.nn.functional.l1_loss), "the engine fuses F.mse_loss"),
                     (dict(preconditioner=object()), "preconditioners \\(EKFAC\\) are dead code")):
        with pytest.raises(NotImplementedError, match=text):
            th.train_epoch(r.model, r.optim, GRID, IMG, **kw)
        with pytest.raises(NotImplementedError, match=text):
            th.train_steps(r.model, r.optim, GRID, IMG, N, **kw)
        r.model.row_split = RowSplit(4, rank=0, world=1)
        with pytest.raises(NotImplementedError, match=text):
            th.train_steps(r.model, r.optim, GRID, IMG, N, **kw)
        r.model.row_split = None
    assert r.eng.calls == []


if __name__ == "__main__":
    routes = []
    for route, r in trace().items():                             # one call per line
        calls = ",\n   ".join(json.dumps(c) for c in r.pop("calls"))
        routes.append(f' {json.dumps(route)}: {{\n  "calls": [\n   {calls}],\n  {json.dumps(r)[1:-1]}}}')
    with open(GOLDEN, "w") as fh:
        fh.write("{\n" + ",\n".join(routes) + "\n}\n")
    print("wrote", GOLDEN)
