"""The quantise phase on the device without a GPU: the ABI as declared, the restatements of tests/_quant_phase_ref.py (the guess,
the nudge) held against exact arithmetic, and which route KmeansQuant takes."""
import ctypes as C
import os
import re
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _quant_phase_ref as Q
from implicit_image import _engine
from implicit_image.models import registry
from implicit_image.pipeline.quant import KmeansQuant
from implicit_image.utils.train_helper import get_optimizer_lr_scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sf_quant_pass", "sf_quant_nudge", "sf_quant_step")
F32 = np.float32


# ---- header, exports, binding ----------------------------------------------------------------------------------------------
def test_abi_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
    protos = {"sf_quant_pass": "int sf_quant_pass(sf_handle* h, const sf_quant_args* a);",
              "sf_quant_nudge": "int sf_quant_nudge(sf_handle* h, const sf_quant_args* a);",
              "sf_quant_step": "int sf_quant_step(sf_handle* h, const sf_quant_args* a, const float* lr, int32_t n_steps, float* loss_out);"}
    declared = set(re.findall(r"^int (sf_quant_\w+)\(", hdr, flags=re.M))
    assert declared == set(NEW) == {n for n in _engine.exported_symbols() if n.startswith("sf_quant_")}
    lib = C.CDLL(_engine._LIB_PATH)
    for name in NEW:
        assert protos[name] in hdr and hasattr(lib, name) and _engine.PROTOTYPES[name][0] == "core"
    assert [f[0] for f in _engine.sf_quant_layer._fields_] == ["layer", "centers_dev", "centroids_dev", "n_centroids_dev", "labels_dev"]
    assert [f[0] for f in _engine.sf_quant_args._fields_] == ["abi_version", "n_layers", "layers", "K", "iter_limit", "tol", "nudge_lr"]
    assert C.sizeof(_engine.sf_quant_layer) == 40 and C.sizeof(_engine.sf_quant_args) == 32      # as the C structs lay out
    assert len(_engine.PROTOTYPES["sf_quant_step"][1]) == 5
    assert _engine.has_quant_step(lib)
    for missing in NEW:
        assert not _engine.has_quant_step(SimpleNamespace(**{n: None for n in NEW if n != missing}))
    assert _engine.FourierEngine.quant_step is None and _engine.WaveletEngine.quant_step is None
    assert callable(_engine.SirenEngine.quant_pass) and callable(_engine.SirenEngine.quant_nudge)
    names = open(os.path.join(os.path.dirname(_engine._LIB_PATH), "engine.h")).read()
    for k in ("k_kmq_guess", "k_kmq_assign", "k_kmq_update", "k_kmq_finish", "k_kmq_predict", "k_kmq_nudge"):
        assert f'"{k}"' in names and f"K_{k[2:].upper()}" in names


def test_refusals_need_no_gpu():
    """null pointers are refused before the handle is looked at"""
    lib = _engine.load_library()
    a = _engine.sf_quant_args(abi_version=_engine.SF_ABI_VERSION, n_layers=1, K=31, iter_limit=5)
    for fn, call in (("sf_quant_pass", lambda: lib.sf_quant_pass(None, C.byref(a))), ("sf_quant_nudge", lambda: lib.sf_quant_nudge(None, C.byref(a))),
                     ("sf_quant_step", lambda: lib.sf_quant_step(None, C.byref(a), None, 1, None))):
        assert call() == -1 and lib.sf_last_error().decode() == fn + ": null argument"


# ---- the fused multiply-add of the guess -----------------------------------------------------------------------------------
def _round_f32(x: Fraction):
    """x rounded to the nearest float32, ties to even, from exact arithmetic"""
    f = F32(float(x))                                              # within one float32 step of the answer
    cands = sorted({float(np.nextafter(f, F32(-np.inf))), float(f), float(np.nextafter(f, F32(np.inf)))})
    best = min(abs(Fraction(c) - x) for c in cands)
    near = [c for c in cands if abs(Fraction(c) - x) == best]
    if len(near) == 1:
        return F32(near[0])
    return F32(next(c for c in near if (np.array(c, F32).view(np.uint32) & 1) == 0))


def test_fma_restatement_is_rounded_once():
    rng = np.random.default_rng(7)
    a = rng.standard_normal(1500).astype(F32)
    b = rng.integers(0, 511, 1500).astype(F32)
    c = (rng.standard_normal(1500) * np.exp(rng.uniform(-12, 3, 1500))).astype(F32)
    got = Q.fma_f32(a[:1500], b[:1500], c)
    for i in range(1500):
        want = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i] == want, (i, a[i], b[i], c[i])
    # the double-rounding trap itself: the float64 sum lands exactly between two float32 values only through ITS rounding.
    # 64 (1 + 2^-20) (1 - 2^-20) = 64 - 2^-34 beside 2^30 + 128: float64 keeps 2^30 + 192, the midpoint, whose tie goes to
    # the even 2^30 + 256; the exact value lies below it and rounds to 2^30 + 128
    p_a, p_b, cc = F32(64 * (1 + 2.0 ** -20)), F32(1 - 2.0 ** -20), F32(2.0 ** 30 + 128)
    for sign in (1, -1):
        want = _round_f32(Fraction(float(p_a)) * Fraction(float(p_b)) * sign + Fraction(float(cc)) * sign)
        assert Q.fma_f32([p_a], [F32(sign) * p_b], [F32(sign) * cc])[0] == want == F32(sign * (2.0 ** 30 + 128))
        assert F32(float(p_a) * float(sign * p_b) + float(sign * cc)) != want       # (rounding twice gets it wrong)


def test_guess_restatement_equals_torch_linspace_on_the_cpu():
    """(the CPU kernel of torch.linspace uses the same contracted form; the device kernel is held to it on the GPU)"""
    rng = np.random.default_rng(3)
    for K in (3, 15, 31, 255, 511):
        for _ in range(40):
            x, y = np.sort((rng.standard_normal(2) * np.exp(rng.uniform(-8, 2))).astype(F32))
            t = torch.linspace(float(x), float(y), K, dtype=torch.float32).numpy()
            assert np.array_equal(t.view(np.int32), Q.guess_from_ends(x, y, K).view(np.int32)), (K, x, y)
    assert not np.isfinite(Q.guess(np.zeros(9, F32), 31)[[0, -1]]).any()           # no non-zero weight: the empty call
    assert Q.guess_ends(np.array([0.0, -0.0, 0.5, -0.25], F32)) == (F32(-0.25), F32(0.5))
    same = Q.guess(np.array([0.0, 0.25, 0.25], F32), 7)
    assert np.array_equal(same, np.full(7, 0.25, F32))


# ---- the nudge -------------------------------------------------------------------------------------------------------------
def _nudge_case(name):
    rng = np.random.default_rng(11)
    n, C_ = 4096, 256
    cent = np.sort(rng.standard_normal(C_).astype(F32) * F32(0.05))
    labels = rng.integers(0, C_, n)
    g = (rng.standard_normal(n) * np.exp(rng.uniform(-9, -4, n))).astype(F32)
    if name == "empty_bin":
        labels[labels == 17] = 18
    elif name == "one_element_bin":
        labels[labels == 40] = 41
        labels[123] = 40
    elif name == "all_zero":
        g[:] = 0.0
    elif name == "minus_zero":
        g[::5] = -0.0
        g[labels == 9] = -0.0
    return cent, labels, g


@pytest.mark.parametrize("name", ["plain", "empty_bin", "one_element_bin", "all_zero", "minus_zero"])
def test_nudge_restatement_within_the_derived_bound_of_the_exact_sum(name):
    """int64 fixed-point segment sums, one rounding, fp32 c - lr * dw against an exact float64 segmented sum:
    |difference| <= lr * (n_k * 2^-24 * sum|g_i| + two float roundings), computed from the case's own data"""
    lr = 3e-4
    cent, labels, g = _nudge_case(name)
    new, dw, unit = Q.nudge_ref(cent, labels, g, lr)
    exact, bound = Q.nudge_bound(cent, labels, g, lr)
    assert new.dtype == F32 and np.all(np.abs(new.astype(np.float64) - exact) <= bound)
    assert unit == 2.0 ** round(np.log2(unit)) and g.size * float(np.abs(g).max() if g.any() else 1) * unit < 2.0 ** 61
    cnt = np.bincount(labels, minlength=cent.size)
    assert np.array_equal(new[cnt == 0].view(np.int32), cent[cnt == 0].view(np.int32))          # an empty bin keeps its bits
    if name == "empty_bin":
        assert cnt[17] == 0
    if name == "one_element_bin":
        assert cnt[40] == 1 and dw[40] == g[123]                   # one element: the sum is that element
    if name == "all_zero":
        assert np.array_equal(new.view(np.int32), cent.view(np.int32)) and not dw.any() and not np.signbit(dw).any()
    if name == "minus_zero":
        assert dw[9] == 0 and not np.signbit(dw[9]) and new[9] == cent[9]
    # the order of arrival does not matter: any permutation gives the same bits
    perm = np.random.default_rng(5).permutation(g.size)
    again, _, _ = Q.nudge_ref(cent, labels[perm], g[perm], lr)
    assert np.array_equal(again.view(np.int32), new.view(np.int32))
    # a float32 sum in arrival order (what scatter_add_ does) lies within the same bound
    f = np.zeros(cent.size, F32)
    np.add.at(f, labels[perm], g[perm])
    host = (cent - (F32(lr) * f).astype(F32)).astype(F32)
    assert np.all(np.abs(host.astype(np.float64) - exact) <= bound)


# ---- which route KmeansQuant takes -----------------------------------------------------------------------------------------
class FakeEngine:
    """what device_plan asks of a handle"""
    device = "cpu"

    def __init__(self, lib):
        self.lib = lib
        self.calls = []

    def param_offsets(self, layer):
        return 0, 0

    def quant_args(self, layers, centres, centroids, counts, labels, K, **kw):
        self.calls.append((list(layers), K))
        return SimpleNamespace(_keep=(None, centres, centroids, counts, labels), nudge_lr=kw.get("nudge_lr"))

    def quant_step(self, *a, **k):
        raise AssertionError("not called here")


def _quantiser(mlp="siren", hidden=64, bits=8, phase="auto", skip=("layers.0.linear", "layers.3.linear"), lib=None, **kw):
    torch.manual_seed(0)
    model = registry[mlp](depth=4, hidden_size=hidden, first_omega_0=50, hidden_omega_0=30, **kw)
    opt, _ = get_optimizer_lr_scheduler(model, dict(name="adam", lr=3e-4), quantize_mode=True)
    kq = KmeansQuant(model, opt, bits=bits, skip_ll=list(skip), device_phase=phase)
    model._engine = FakeEngine(_engine.load_library() if lib is None else lib)
    return model, kq


def test_plan_on_an_unpadded_siren():
    model, kq = _quantiser()
    plan = kq.device_plan()
    assert plan is not None and plan[0] is model._engine and model._engine.calls == [([1, 2], 255)]
    assert kq.device_plan() is plan and len(model._engine.calls) == 1              # made once per handle
    _, centres, centroids, counts, labels = plan[1]._keep
    assert [c.numel() for c in centres] == [255, 255] and [c.numel() for c in centroids] == [256, 256]
    assert [tuple(l.shape) for l in labels] == [(64, 64), (64, 64)] and labels[0].dtype == torch.int64 and counts[0].dtype == torch.int32
    model, kq = _quantiser(skip=())                                                # skip_ll = []: first and last layer too
    assert kq.device_plan() is not None and model._engine.calls == [([0, 1, 2, 3], 255)]
    model, kq = _quantiser(bits=9)
    assert kq.device_plan() is not None and model._engine.calls == [([1, 2], 511)]


@pytest.mark.parametrize("why", ["padded", "fourier", "off", "env", "env_native", "old_library", "no_method", "bits_1", "bits_10", "unbound"])
def test_every_other_case_keeps_the_host_path(why, monkeypatch):
    kw = {}
    if why == "padded":
        kw = dict(hidden=48)                                       # runs zero-padded to 64
    if why == "fourier":
        kw = dict(mlp="fourier")
    if why == "off":
        kw = dict(phase="off")
    if why == "old_library":
        kw = dict(lib=SimpleNamespace(sf_kmeans_fit=None))
    if why == "bits_1":
        kw = dict(bits=1)
    if why == "bits_10":
        kw = dict(bits=10)
    model, kq = _quantiser(**kw)
    if why == "env":
        monkeypatch.setenv("SIREN_FIT_DEVICE_QUANT", "0")
    if why == "env_native":
        monkeypatch.setenv("SIREN_FIT_NATIVE_KMEANS", "0")
    if why == "no_method":
        model._engine.quant_step = None                            # (what FourierEngine / WaveletEngine say)
    if why == "unbound":
        model._engine = None
    assert kq.device_plan() is None
    if model._engine is not None:
        assert model._engine.calls == []
    # ... and without error: the pre-pass callback of an unbound CPU model is the torch mirror
    if why in ("off", "env", "bits_10") and why != "fourier":
        model._engine = None
        before = model.layers[1].linear.weight.detach().clone()
        kq.kmeans_modify_weights()
        lin = model.layers[1].linear
        assert lin.n_centroids is None and lin.labeled_weight.shape == before.shape
        assert torch.equal(lin.weight.detach(), lin.centroids[lin.labeled_weight])


def test_config_has_the_switch():
    from implicit_image.config import load_config
    cfg = load_config(os.path.join(ROOT, "conf"), [])
    assert cfg.quant.device_phase == "auto"
    from implicit_image.pipeline.quant import Quantize
    for text, want in (("off", "off"), ("auto", "auto")):          # (a bare `off` arrives as YAML's false)
        qcfg = load_config(os.path.join(ROOT, "conf"), [f"quant.device_phase={text}"]).quant
        model = registry["siren"](depth=4, hidden_size=64)
        with Quantize(model, get_optimizer_lr_scheduler(model, dict(name="adam", lr=3e-4))[0], qcfg) as q:
            assert q.compress.device_phase == want
    with pytest.raises(AssertionError):
        KmeansQuant(torch.nn.Linear(2, 2), None, device_phase="maybe")
