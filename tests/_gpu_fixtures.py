"""What the GPU children (tests/_*_child.py) and the in-process GPU tests share: each piece here has at least two callers.
Importing this (or _gpu_child) is all the path setup a child needs."""
import ctypes as C
import hashlib
import os

import numpy as np
import torch

from _gpu_child import ROOT
from oracle import siren_oracle as so

FILL = 0xA5                                    # the sentinel byte behind a Guarded buffer


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def u8_ref(pred):
    """min(max(trunc(pred * 255), 0), 255), written out independently of implicit_image.decode.to_u8"""
    q = torch.trunc(pred.float() * 255.0)
    return torch.minimum(torch.maximum(q, torch.zeros_like(q)), torch.full_like(q, 255.0)).to(torch.uint8)


def u16_ref(pred):
    """min(max(trunc(pred * 65535), 0), 65535) as int32, written out independently of implicit_image.decode.to_u16"""
    q = torch.trunc(pred.float() * 65535.0)
    return torch.minimum(torch.maximum(q, torch.zeros_like(q)), torch.full_like(q, 65535.0)).to(torch.int32)


class Guarded:
    """a device buffer of n samples of 8 or 16 bits followed by `guard` sentinel bytes (torch.full is 4-byte aligned and
    more)"""

    def __init__(self, n, bits, guard):
        self.nbytes = n * bits // 8
        self.bits = bits
        self.buf = torch.full((self.nbytes + guard,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 4 == 0

    def ptr(self):
        return self.buf.data_ptr()

    def samples(self, shape):
        """the samples; 16-bit ones widened to int32 (through int16: every torch build converts that type on the device)"""
        s = self.buf[:self.nbytes]
        return (s if self.bits == 8 else s.view(torch.int16).to(torch.int32) & 0xFFFF).reshape(shape)

    def guard_intact(self):
        return bool((self.buf[self.nbytes:] == FILL).all())


def siren_params(hidden, depth, nout, seed, last_scale, bias_scale):
    """the oracle's SIREN initialisation with the first nout rows of the output layer scaled by last_scale and their
    biases by bias_scale (0: 0.5 + 0.5 * last_scale * (W h) swings to both sides of [0, 1] in every channel)"""
    p = so.siren_init(hidden, depth, seed=seed)
    p[-2], p[-1] = p[-2][:nout] * last_scale, p[-1][:nout] * bias_scale
    return torch.tensor(so.flatten(p))


def fourier_params(hidden, n_linear, map_size, gen):
    """seeded uniform weights of He scale (the ReLU activations stay of order one at every depth), small biases, the output
    layer four times larger so that the sigmoid spreads over many levels"""
    parts = []
    for l in range(n_linear):
        fin = map_size if l == 0 else hidden
        fout = 3 if l == n_linear - 1 else hidden
        scale = (6.0 / fin) ** 0.5 * (4.0 if l == n_linear - 1 else 1.0)
        parts += [((torch.rand(fout * fin, generator=gen) * 2 - 1) * scale), (torch.rand(fout, generator=gen) * 2 - 1) * 0.1]
    return torch.cat(parts).float().contiguous()


def wavelet_params(last_scale, seed, rescale, **kw):
    """[LF | HF] of a seed-`seed` registry model (kernel widths: no padding); with rescale both output layers are scaled by
    last_scale and their biases zeroed, so that the coefficients - and with them the picture - swing to both sides of
    [0, 1]"""
    from implicit_image.models import registry
    torch.manual_seed(seed)
    m = registry["wavelet_siren"](**kw)
    with torch.no_grad():
        if rescale:
            for sub in (m.LF_siren, m.HF_siren):
                sub.layers[-1].linear.weight.mul_(last_scale)
                sub.layers[-1].linear.bias.zero_()
    return torch.cat([p.data.reshape(-1).float() for p in m._param_list()]).contiguous()


def recorder(lib):
    """-> (out, rec): rec(name, rc) puts {rc, msg} of a C ABI call under out[name]"""
    out = {}

    def rec(name, rc):
        out[name] = {"rc": int(rc), "msg": lib.sf_last_error().decode() if rc else ""}
    return out, rec


def launches(eng):
    return int(sum(v["launches"] for v in eng.profile_report().values()))


TRAINING_CALLS = ["sf_forward_backward", "sf_forward", "sf_step", "sf_adam_step", "sf_set_masks", "sf_get_grads", "sf_set_grads",
                  "sf_get_adam_state", "sf_set_adam_state", "sf_kmeans_fit", "sf_feather_attach", "sf_feather_state_ptr",
                  "sf_feather_materialise", "sf_feather_adjoint", "sf_debug_scratch", "sf_state_ptr_grads"]


def refused_training_calls(rec, lib, eng, buf, feather_layers, render_to, set_target):
    """TRAINING_CALLS on a render handle, each recorded under its name; then sf_render into render_to (a WaveletSiren render
    handle refuses that too) unless it is None, and sf_set_target if set_target.  buf: num_params floats on the device"""
    lr = (C.c_float * 1)(1e-3)
    sse = C.c_double()
    step = C.c_int64()
    p, n = C.c_void_p(), C.c_int64()
    li = (C.c_int32 * 4)(64, 64, 64, 3)
    rec("sf_forward_backward", lib.sf_forward_backward(eng.h, C.byref(sse)))
    rec("sf_forward", lib.sf_forward(eng.h, None, None))
    rec("sf_step", lib.sf_step(eng.h, lr, 1, None))
    rec("sf_adam_step", lib.sf_adam_step(eng.h, 1e-3))
    rec("sf_set_masks", lib.sf_set_masks(eng.h, buf.data_ptr()))
    rec("sf_get_grads", lib.sf_get_grads(eng.h, buf.data_ptr()))
    rec("sf_set_grads", lib.sf_set_grads(eng.h, buf.data_ptr()))
    rec("sf_get_adam_state", lib.sf_get_adam_state(eng.h, buf.data_ptr(), buf.data_ptr(), C.byref(step)))
    rec("sf_set_adam_state", lib.sf_set_adam_state(eng.h, buf.data_ptr(), buf.data_ptr(), 0))
    rec("sf_kmeans_fit", lib.sf_kmeans_fit(eng.h, buf.data_ptr(), 16, buf.data_ptr(), 3, 1, 1e-4, buf.data_ptr(), 4, None, None, None))
    rec("sf_feather_attach", lib.sf_feather_attach(eng.h, 8, 8, feather_layers, li, li))
    rec("sf_feather_state_ptr", lib.sf_feather_state_ptr(eng.h, 0, C.byref(p), C.byref(n)))
    rec("sf_feather_materialise", lib.sf_feather_materialise(eng.h))
    rec("sf_feather_adjoint", lib.sf_feather_adjoint(eng.h))
    rec("sf_debug_scratch", lib.sf_debug_scratch(eng.h, 0, C.byref(p), C.byref(n)))
    rec("sf_state_ptr_grads", lib.sf_state_ptr(eng.h, 1, C.byref(p)))
    if render_to is not None:
        rec("sf_render", lib.sf_render(eng.h, render_to, None))
    if set_target:
        rec("sf_set_target", lib.sf_set_target(eng.h, buf.data_ptr()))


def working_calls(rec, lib, eng, buf, offset_layer, set_and_count):
    """what a render handle must keep answering, recorded as ok_<name>; with set_and_count also sf_set_params and
    sf_num_params.  -> [weight offset, bias offset of offset_layer, sf_num_params' answer (0 without set_and_count)]"""
    p, n, w, b = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
    rec("ok_sf_state_ptr_params", lib.sf_state_ptr(eng.h, 0, C.byref(p)))
    if set_and_count:
        rec("ok_sf_set_params", lib.sf_set_params(eng.h, buf.data_ptr()))
    rec("ok_sf_get_params", lib.sf_get_params(eng.h, buf.data_ptr()))
    rec("ok_sf_params_changed", lib.sf_params_changed(eng.h))
    if set_and_count:
        rec("ok_sf_num_params", lib.sf_num_params(eng.h, C.byref(n)))
    rec("ok_sf_param_offset", lib.sf_param_offset(eng.h, offset_layer, C.byref(w), C.byref(b)))
    return [int(w.value), int(b.value), int(n.value)]


def handle_memory(make_engine):
    """-> (device bytes the handle make_engine() returns takes, the handle); in a fresh process, so that nothing else
    allocates in between"""
    torch.cuda.init()
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    eng = make_engine()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    return int(free0 - free1), eng


def siren_engine(H, W, hidden, depth, dtype="f16", params=None, img=None, **kw):
    """a SirenEngine with the oracle's grid, and with parameters / the handle's rows of a target where given"""
    from implicit_image._engine import SirenEngine
    eng = SirenEngine(H, W, hidden, depth, compute_dtype=dtype, **kw)
    gh, gw = so.grid_vectors(H, W)
    eng.set_coords(gh.cuda(), gw.cuda())
    if params is not None:
        eng.set_params(torch.tensor(so.flatten(params)).cuda())
    if img is not None:
        eng.set_target(img[eng.row_begin:eng.row_end].contiguous().cuda())
    return eng
