"""sf_eval without a GPU: the ABI as declared and exported, the null refusal, which route eval_metrics takes, the config key."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

from implicit_image import _engine
from implicit_image.utils import train_helper as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sf_eval", "sf_sse8_ptr")


def test_abi_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
    protos = {"sf_eval": "int sf_eval(sf_handle* h, double* sse_out, uint64_t* sse8_out);",
              "sf_sse8_ptr": "int sf_sse8_ptr(sf_handle* h, uint64_t** dev_ptr);"}
    assert set(NEW) <= set(re.findall(r"^int (sf_\w+)\(", hdr, flags=re.M)) and set(NEW) <= set(_engine.exported_symbols())
    lib = C.CDLL(_engine._LIB_PATH)
    for name in NEW:
        assert protos[name] in hdr and hasattr(lib, name) and _engine.PROTOTYPES[name][0] == "core"
    assert len(_engine.PROTOTYPES["sf_eval"][1]) == 3 and len(_engine.PROTOTYPES["sf_sse8_ptr"][1]) == 2
    assert "#define SF_ABI_VERSION 3 " in hdr                      # detected by presence: the version stays
    assert _engine.has_eval(lib)
    for missing in NEW:
        assert not _engine.has_eval(SimpleNamespace(**{n: None for n in NEW if n != missing}))
    for cls in (_engine.SirenEngine, _engine.FourierEngine, _engine.WaveletEngine):
        assert callable(cls.eval_sums) and callable(cls.sse8_view)


def test_null_handle_is_refused_without_a_gpu():
    lib = _engine.load_library()
    sse, sse8 = C.c_double(), C.c_uint64()
    assert lib.sf_eval(None, C.byref(sse), C.byref(sse8)) == -1 and lib.sf_last_error().decode() == "sf_eval: null argument"
    p = C.c_void_p()
    assert lib.sf_sse8_ptr(None, C.byref(p)) == -1


# ---- which route eval_metrics takes ----------------------------------------------------------------------------------------
class FakeEngine:
    """what eval_epoch and eval_metrics ask of a handle: forward() hands back a fixed prediction, eval_sums() fixed sums"""

    def __init__(self, lib, pred, sums=None, sse=None):
        self.lib, self.pred, self.calls, self.sse = lib, pred, [], sse
        if sums is not None:
            self.eval_sums = lambda sync=True: self.calls.append("eval_sums") or sums

    def forward(self, want_pred=True, want_sse=True):
        self.calls.append("forward")
        return self.pred, float(((self.pred - IMG) ** 2).double().sum()) if self.sse is None else self.sse


class FakeModel:
    def __init__(self, eng):
        self.eng, self.modes = eng, []

    def eval(self):
        self.modes.append("eval")

    def engine(self, grid, img):
        self.modes.append("engine")
        return self.eng


G = torch.Generator().manual_seed(0)
IMG = torch.rand(4, 5, 3, generator=G)
PRED = IMG + 0.1 * torch.randn(4, 5, 3, generator=G)
FULL = SimpleNamespace(sf_eval=None, sf_sse8_ptr=None)


@pytest.mark.parametrize("why", ["old_library_eval", "old_library_ptr", "no_method"])
def test_without_the_entry_point_eval_metrics_is_eval_epoch(why):
    lib = {"old_library_eval": SimpleNamespace(sf_sse8_ptr=None), "old_library_ptr": SimpleNamespace(sf_eval=None), "no_method": FULL}[why]
    eng = FakeEngine(lib, PRED, sums=None if why == "no_method" else (1.0, 1))
    got = th.eval_metrics(FakeModel(eng), None, IMG)
    want = th.eval_epoch(FakeModel(FakeEngine(lib, PRED)), None, IMG)[1:]
    assert got == want and "eval_sums" not in eng.calls and "forward" in eng.calls


def test_with_the_entry_point_one_eval_sums_call_and_the_formulas():
    S = int((((IMG * 255).int() - (PRED * 255).int()).long() ** 2).sum())
    sse = float(((PRED - IMG) ** 2).double().sum())
    eng = FakeEngine(FULL, PRED, sums=(sse, S))
    model = FakeModel(eng)
    loss, psnr, psnr8 = th.eval_metrics(model, None, IMG)
    assert eng.calls == ["eval_sums"] and model.modes == ["eval", "engine"]
    n = IMG.numel()
    _, loss_e, psnr_e, psnr8_e = th.eval_epoch(FakeModel(FakeEngine(FULL, PRED)), None, IMG)
    assert loss == sse / n == loss_e and psnr == 10 * math.log10(1 / loss) == psnr_e
    assert psnr8 == 10 * math.log10(65025 / (S / n))
    assert abs(psnr8 - psnr8_e) <= 1e-4
    # a perfect 8-bit picture: torch's formula gives inf, and so does this one
    assert th.eval_metrics(FakeModel(FakeEngine(FULL, IMG, sums=(sse, 0))), None, IMG)[2] == math.inf
    assert th.eval_epoch(FakeModel(FakeEngine(FULL, IMG, sse=sse)), None, IMG)[3] == math.inf


def test_config_has_the_switch():
    from implicit_image.config import load_config
    assert load_config(os.path.join(ROOT, "conf"), []).train.device_eval == "auto"
    for text, want in (("off", False), ("false", False), ("auto", True), ("true", True)):
        cfg = load_config(os.path.join(ROOT, "conf"), [f"train.device_eval={text}"])
        assert th.device_eval_wanted(cfg.train.device_eval) is want, text
    assert th.device_eval_wanted("auto") and not th.device_eval_wanted("off") and not th.device_eval_wanted(False)
    with pytest.raises(ValueError):
        th.device_eval_wanted("maybe")
