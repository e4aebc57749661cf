"""ctypes binding of libsiren_fit.so (C ABI: include/siren_fit.h).

PyTorch is used only for device memory, streams and (in parallel.py) torch.distributed; every
arithmetic step of the hot path runs in the HIP library.  Missing library => ImportError-like
RuntimeError at load time (no fallback path exists).
"""
import ctypes as C
import os
from typing import Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SIREN_FIT_LIB: developer override to A/B kernel variants built side by side (same C ABI)
_LIB_PATH = os.environ.get("SIREN_FIT_LIB") or os.path.normpath(os.path.join(_HERE, "..", "csrc", "libsiren_fit.so"))

SF_ABI_VERSION = 3
DTYPES = {"bf16": 0, "f16": 1}


class sf_config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("row_begin", C.c_int32), ("row_end", C.c_int32),
        ("in_features", C.c_int32), ("out_features", C.c_int32), ("hidden", C.c_int32), ("depth", C.c_int32),
        ("first_omega_0", C.c_float), ("hidden_omega_0", C.c_float),
        ("outermost_linear", C.c_int32), ("compute_dtype", C.c_int32),
        ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("device", C.c_int32), ("stream", C.c_void_p), ("chunk_pixels", C.c_int64),
        ("scratch_format", C.c_int32),
    ]


class sf_fourier_config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("in_features", C.c_int32), ("out_features", C.c_int32), ("map_size", C.c_int32), ("hidden", C.c_int32),
        ("n_linear", C.c_int32), ("compute_dtype", C.c_int32),
        ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("device", C.c_int32), ("stream", C.c_void_p), ("chunk_pixels", C.c_int64),
    ]


class sf_wavelet_config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
        ("in_features", C.c_int32), ("out_features", C.c_int32), ("hidden", C.c_int32), ("depth", C.c_int32),
        ("wavelet_levels", C.c_int32), ("first_omega_0", C.c_float), ("hidden_omega_0", C.c_float),
        ("outermost_linear", C.c_int32), ("compute_dtype", C.c_int32),
        ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("device", C.c_int32), ("stream", C.c_void_p), ("chunk_pixels", C.c_int64), ("scratch_format", C.c_int32),
    ]


class sf_wavelet_render_config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("height", C.c_int32), ("max_rows", C.c_int32), ("max_cols", C.c_int32),
        ("hidden", C.c_int32), ("depth", C.c_int32), ("first_omega_0", C.c_float), ("hidden_omega_0", C.c_float),
        ("outermost_linear", C.c_int32), ("compute_dtype", C.c_int32), ("device", C.c_int32),
        ("stream", C.c_void_p), ("chunk_pixels", C.c_int64),
    ]


class sf_mask_layer_stats(C.Structure):
    _fields_ = [("live_before", C.c_int64), ("dead_before", C.c_int64), ("nnz_before", C.c_int64), ("removed", C.c_int64),
                ("live_after", C.c_int64), ("dead_after", C.c_int64), ("nnz_after", C.c_int64), ("prune_rate", C.c_double)]


class sf_mask_update_args(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("n_layers", C.c_int32), ("layers", C.POINTER(C.c_int32)),
                ("prune_rate", C.c_double), ("growth", C.c_int32), ("dense_gradients", C.c_int32),
                ("stats_dev", C.c_void_p)]


class sf_mask_prune_global_args(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("n_layers", C.c_int32), ("layers", C.POINTER(C.c_int32)),
                ("target", C.c_int64), ("prune_rate", C.c_double), ("threshold", C.c_double), ("increment", C.c_double),
                ("tolerance", C.c_double), ("dense_gradients", C.c_int32), ("stats_dev", C.c_void_p)]


class sf_mask_snfs_stats(C.Structure):
    _fields_ = sf_mask_layer_stats._fields_ + [("stat_before", C.c_double), ("budget", C.c_double), ("grown", C.c_int64),
                                               ("stat_after", C.c_double)]


class sf_mask_update_snfs_args(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("n_layers", C.c_int32), ("layers", C.POINTER(C.c_int32)),
                ("prune_rate", C.c_double), ("adjusted_growth", C.c_double), ("growth", C.c_int32), ("statistic", C.c_int32),
                ("dense_gradients", C.c_int32), ("stats_dev", C.c_void_p)]


class sf_quant_layer(C.Structure):
    _fields_ = [("layer", C.c_int32), ("centers_dev", C.c_void_p), ("centroids_dev", C.c_void_p),
                ("n_centroids_dev", C.c_void_p), ("labels_dev", C.c_void_p)]


class sf_quant_args(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("n_layers", C.c_int32), ("layers", C.POINTER(sf_quant_layer)),
                ("K", C.c_int32), ("iter_limit", C.c_int32), ("tol", C.c_float), ("nudge_lr", C.c_float)]


MASK_STATS_WORDS = C.sizeof(sf_mask_layer_stats) // 8      # a statistics row as int64 words (the last one: a double)
MASK_SNFS_STATS_WORDS = C.sizeof(sf_mask_snfs_stats) // 8  # ... of sf_mask_update_snfs (words 7, 8, 9 and 11: doubles)
MASK_GROWTH = {"none": 0, "absolute-gradient": 1, "momentum": 2}
MASK_STATISTIC = {"none": 0, "nonzero": 0, "momentum": 1}

_lib = None

H, F, I32, I64, P = C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.POINTER      # H: sf_handle*, F: device float*
# Every entry point of include/siren_fit.h, once: name -> (group, argtypes, restype).  Every "core" symbol must be there;
# the other groups are bound only when present, so a library built before them still loads (the feature then fails with a
# message naming the rebuild instead of the whole engine failing).
PROTOTYPES = {}


def _declare(group: str, protos: dict, restype=C.c_int):
    PROTOTYPES.update({name: (group, args, restype) for name, args in protos.items()})


_declare("core", {"sf_last_error": []}, C.c_char_p)
_declare("core", {
    "sf_abi_version": [],
    "sf_create": [P(sf_config), P(H)],
    "sf_destroy": [H],
    "sf_fourier_create": [P(sf_fourier_config), P(H)],
    "sf_set_encoding": [H, F],
    "sf_num_params": [H, P(I64)],
    "sf_scratch_format": [H, P(I32)],
    "sf_param_offset": [H, I32, P(I64), P(I64)],
    "sf_set_params": [H, F], "sf_get_params": [H, F], "sf_set_masks": [H, F],
    "sf_get_grads": [H, F], "sf_set_grads": [H, F],
    "sf_get_adam_state": [H, F, F, P(I64)], "sf_set_adam_state": [H, F, F, I64],
    "sf_state_ptr": [H, I32, P(C.c_void_p)],
    "sf_sse_ptr": [H, P(C.c_void_p)],
    "sf_debug_scratch": [H, I32, P(C.c_void_p), P(I64)],
    "sf_debug_throw": [I32],
    "sf_kmeans_fit": [H, F, I64, F, I32, I32, C.c_float, F, I32, C.c_void_p, C.c_void_p, F],
    "sf_params_changed": [H],
    "sf_set_coords": [H, F, F], "sf_set_target": [H, F],
    "sf_forward": [H, F, P(C.c_double)],
    "sf_forward_backward": [H, P(C.c_double)],
    "sf_adam_step": [H, C.c_float],
    "sf_step": [H, P(C.c_float), I32, P(C.c_float)],
    "sf_profile_enable": [H, I32], "sf_profile_reset": [H], "sf_set_graph_replay": [H, I32],
    "sf_profile_num_kernels": [H, P(I32)],
    "sf_profile_get": [H, I32, P(C.c_char_p), P(C.c_double), P(I64), P(C.c_double), P(C.c_double)],
})
_declare("feather", {
    "sf_feather_attach": [H, I64, I64, I32, P(I32), P(I32)],
    "sf_feather_state_ptr": [H, I32, P(C.c_void_p), P(I64)],
    "sf_feather_materialise": [H], "sf_feather_adjoint": [H],
    "sf_feather_render_attach": [H, I64, I64, I32, P(I32), P(I32)],
    "sf_feather_render_load": [H, F],
})
_declare("wavelet", {
    "sf_wavelet_create": [P(sf_wavelet_config), P(H)],
    "sf_wavelet_debug": [H, I32, F, F, F, F, F],
})
# inference-only entry points (csrc/siren_render.hip, wavelet_render.hip, fourier_render.hip)
_declare("render", {"sf_render_create": [P(sf_config), P(H)], "sf_render": [H, C.c_void_p, F]})
# (sf_render at 16 bits per sample.  Not in group "render": has_render / has_fourier_render answer for the 8-bit path of a
# library that has nothing else; RenderEngine.render(bits=16) asks for this symbol itself)
_declare("core", {"sf_render16": [H, C.c_void_p, F]})
_declare("wavelet_render", {
    "sf_wavelet_render_create": [P(sf_wavelet_render_config), P(H)],
    "sf_wavelet_render": [H, I32, I32, I32, I32, C.c_void_p, F],
    "sf_wavelet_render16": [H, I32, I32, I32, I32, C.c_void_p, F],
})
_declare("fourier_render", {"sf_fourier_render_create": [P(sf_fourier_config), P(H)]})
# (the render handle of SIREN 512 / 1024: the RENDER forms of the layer-at-a-time kernels, csrc/siren_wide.hip.  In "core" like
# sf_render16 and sf_mask_update: has_wide_render asks for the three symbols themselves)
_declare("core", {
    "sf_wide_render_create": [P(sf_config), P(H)],
    "sf_wide_render": [H, C.c_void_p, F],
    "sf_wide_render16": [H, C.c_void_p, F],
})
# (the RigL topology update on the device, csrc/siren_mask.hip.  In "core" like sf_render16: has_mask_update asks for the
# symbol itself, Masking routes by it)
_declare("core", {"sf_mask_update": [H, P(sf_mask_update_args)]})
# (the global-magnitude update of masking=Pruning on the device, same file; has_mask_prune_global asks for the symbol itself)
_declare("core", {"sf_mask_prune_global": [H, P(sf_mask_prune_global_args)]})
# (the update of masking=SNFS on the device, same file; has_mask_update_snfs asks for the symbol itself)
_declare("core", {"sf_mask_update_snfs": [H, P(sf_mask_update_snfs_args)]})
# (the quantise phase on the device, csrc/siren_quant.hip; has_quant_step asks for the symbols themselves, KmeansQuant routes by it)
_declare("core", {
    "sf_quant_pass": [H, P(sf_quant_args)],
    "sf_quant_nudge": [H, P(sf_quant_args)],
    "sf_quant_step": [H, P(sf_quant_args), P(C.c_float), I32, P(C.c_float)],
})
# (eval_epoch's three figures on the device, sf_eval in csrc/siren_fit.hip.  In "core" like sf_quant_step: has_eval asks for the
# symbols themselves, train_helper.eval_metrics routes by it)
_declare("core", {
    "sf_eval": [H, P(C.c_double), P(C.c_uint64)],
    "sf_sse8_ptr": [H, P(C.c_void_p)],
})
# (n_steps steps of several fits of one shape in one launch per kernel, sf_step_many in csrc/many_host.hip.  In "core" like
# sf_eval: has_step_many asks for the symbol itself, train_helper.train_steps_many routes by it)
_declare("core", {"sf_step_many": [P(H), I32, P(C.c_float), I32, P(C.c_float)]})
STEP_MANY_MAX = 64      # SF_STEP_MANY_MAX


def load_library():
    """Load libsiren_fit.so once and declare the prototypes of include/siren_fit.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"{_LIB_PATH} not found: build it with `python __graft_entry__.py build` (hipcc "
            "--offload-arch=gfx950). The SIREN engine has no CPU fallback.")
    lib = C.CDLL(_LIB_PATH)
    for name, (group, args, restype) in PROTOTYPES.items():
        if group == "core" and not hasattr(lib, name):
            raise RuntimeError(f"{_LIB_PATH} has no {name} entry point (built before it was added): rebuild it with "
                               "`python __graft_entry__.py build`")
        if group == "core" or hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = restype
    if lib.sf_abi_version() != SF_ABI_VERSION:
        raise RuntimeError("libsiren_fit.so ABI version mismatch")
    _lib = lib
    return lib


def _has(lib, group: str) -> bool:
    return all(hasattr(lib, name) for name, proto in PROTOTYPES.items() if proto[0] == group)


def _render_entry(lib, name: str, bits: int):
    """the entry point `name` (bits = 8) or `name`16 (bits = 16) of a library that has the group; else a ValueError"""
    if bits not in (8, 16):
        raise ValueError(f"render: bits must be 8 or 16, got {bits!r}")
    return getattr(lib, name + ("16" if bits == 16 else ""))


def has_feather(lib) -> bool:
    return _has(lib, "feather")


def has_wavelet(lib) -> bool:
    return _has(lib, "wavelet")


def has_render(lib) -> bool:
    return _has(lib, "render")


def has_wavelet_render(lib) -> bool:
    return _has(lib, "wavelet_render")


def has_fourier_render(lib) -> bool:
    """sf_fourier_render_create, and with it sf_render on FourierNet handles (csrc/fourier_render.hip)"""
    return has_render(lib) and _has(lib, "fourier_render")


def has_wide_render(lib) -> bool:
    """sf_wide_render_create / sf_wide_render / sf_wide_render16: SIREN 512 / 1024 on a render handle"""
    return all(hasattr(lib, n) for n in ("sf_wide_render_create", "sf_wide_render", "sf_wide_render16"))


def has_mask_update(lib) -> bool:
    """sf_mask_update: Masking.update_connections() on the device (csrc/siren_mask.hip)"""
    return hasattr(lib, "sf_mask_update")


def has_mask_prune_global(lib) -> bool:
    """sf_mask_prune_global: the global-magnitude update of masking=Pruning on the device (csrc/siren_mask.hip)"""
    return hasattr(lib, "sf_mask_prune_global")


def has_mask_update_snfs(lib) -> bool:
    """sf_mask_update_snfs: the momentum-growth, momentum-redistribution update of masking=SNFS on the device"""
    return hasattr(lib, "sf_mask_update_snfs")


def has_quant_step(lib) -> bool:
    """sf_quant_pass / sf_quant_nudge / sf_quant_step: the quantise phase on the device (csrc/siren_quant.hip)"""
    return all(hasattr(lib, n) for n in ("sf_quant_pass", "sf_quant_nudge", "sf_quant_step"))


def has_eval(lib) -> bool:
    """sf_eval / sf_sse8_ptr: the sums of an evaluation on the device, no prediction written (csrc/siren_fit.hip)"""
    return all(hasattr(lib, n) for n in ("sf_eval", "sf_sse8_ptr"))


def has_step_many(lib) -> bool:
    """sf_step_many: the training steps of several fits of one shape, one launch per kernel (csrc/many_host.hip)"""
    return hasattr(lib, "sf_step_many")


def _require(lib, has, entry: str, since: str):
    """a library that lacks an optional group: say which entry point is missing and how to get it"""
    if not has(lib):
        raise RuntimeError(f"{_LIB_PATH} has no {entry} (built before {since}): rebuild it with "
                           "`python __graft_entry__.py build`")


def exported_symbols() -> Sequence[str]:
    """Names include/siren_fit.h declares (used by the CPU test that the library exports them all)."""
    hdr = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "siren_fit.h"))
    import re
    txt = open(hdr).read()
    return sorted(set(re.findall(r"\b(sf_[a-z_0-9]+)\s*\(", txt)))


def _check(rc: int):
    if rc != 0:
        raise RuntimeError(f"siren_fit error {rc}: {load_library().sf_last_error().decode()}")


class _DevView:
    """Zero-copy torch view of engine-owned device memory via __cuda_array_interface__."""

    def __init__(self, ptr: int, n: int, typestr: str = "<f4"):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _f32_cuda(t: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("expected a contiguous float32 CUDA tensor")
    if n is not None and t.numel() != n:
        raise ValueError(f"expected {n} elements, got {t.numel()}")
    return t


def step_many(engines, lrs, want_loss: bool = False):
    """sf_step_many on the handles of `engines` (SirenEngine, one shape, one stream): lrs[s][b] is the learning rate of step
    s for member b.  Each member ends where its own step(column b) would, bit for bit.  The losses as a list per member
    (loss[b][s], one read at the end), or None."""
    lib = load_library()
    _require(lib, has_step_many, "sf_step_many entry point", "the batched training step")
    B, n = len(engines), len(lrs)
    if any(len(row) != B for row in lrs):
        raise ValueError(f"step_many: every row of lrs needs {B} learning rates")
    hs = (C.c_void_p * max(B, 1))(*[e.h for e in engines])
    arr = (C.c_float * max(n * B, 1))(*[float(v) for row in lrs for v in row])
    out = (C.c_float * max(n * B, 1))() if want_loss else None
    _check(lib.sf_step_many(hs, B, arr, n, out))
    return [[out[s * B + b] for s in range(n)] for b in range(B)] if want_loss else None


def step_many_refusal(engines):
    """what sf_step_many says to these members, without running anything: a call of zero steps makes every check and
    launches, allocates and changes nothing.  None: it takes them; else the library's message"""
    lib = load_library()
    B = len(engines)
    if any(getattr(e, "h", None) is None for e in engines):
        return "sf_step_many: a member has no engine handle"
    hs = (C.c_void_p * max(B, 1))(*[e.h for e in engines])
    lr = (C.c_float * 1)(0.0)
    return None if lib.sf_step_many(hs, B, lr, 0, None) == 0 else lib.sf_last_error().decode()


class SirenEngine:
    """One per-image fit on one HIP stream (one sf_handle)."""

    STATE = {"params": 0, "grads": 1, "exp_avg": 2, "exp_avg_sq": 3, "masks": 4}
    # the create entry point of this class and, when it belongs to an optional group, what _require says without it; the
    # entry point render() draws with
    _CREATE, _CREATE_NEEDS = "sf_create", None
    _RENDER = "sf_render"

    def __init__(self, height: int, width: int, hidden: int, depth: int, first_omega_0: float = 50.0,
                 hidden_omega_0: float = 30.0, outermost_linear: bool = True, out_features: int = 3,
                 compute_dtype: str = "f16", device: int = 0, row_begin: int = 0, row_end: int = 0,
                 chunk_pixels: int = 0, betas=(0.9, 0.999), eps: float = 1e-8, scratch_format: int = 0):
        cfg = sf_config(height=height, width=width, row_begin=row_begin, row_end=row_end, in_features=2,
                        out_features=out_features, hidden=hidden, depth=depth, first_omega_0=first_omega_0,
                        hidden_omega_0=hidden_omega_0, outermost_linear=int(bool(outermost_linear)), beta1=betas[0],
                        beta2=betas[1], eps=eps, chunk_pixels=chunk_pixels, scratch_format=scratch_format)
        self._open(cfg, device, height, width, hidden, depth, out_features, row_begin, row_end, compute_dtype,
                   who="SirenEngine")

    def _open(self, cfg, device: int, height: int, width: int, hidden: int, depth: int, out_features: int = 3,
              row_begin: int = 0, row_end: int = 0, compute_dtype: str = "f16", who: Optional[str] = None):
        """The one constructor path: library, GPU, device and stream, then the handle (type(self)._CREATE on `cfg`, whose
        abi_version / compute_dtype / device / stream are filled in here), sf_num_params and the attributes every handle has."""
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError(f"{who or type(self).__name__} needs a gfx950 GPU (torch.cuda.is_available() is False); "
                               "no CPU fallback")
        self.device = torch.device("cuda", device)
        with torch.cuda.device(self.device):
            cfg.stream = torch.cuda.current_stream(self.device).cuda_stream
        cfg.abi_version, cfg.compute_dtype, cfg.device = SF_ABI_VERSION, DTYPES[compute_dtype], device
        self.h = C.c_void_p()
        if self._CREATE_NEEDS:
            _require(self.lib, *self._CREATE_NEEDS)
        _check(getattr(self.lib, self._CREATE)(C.byref(cfg), C.byref(self.h)))
        n = C.c_int64()
        _check(self.lib.sf_num_params(self.h, C.byref(n)))
        self.num_params = n.value
        self.height, self.width, self.hidden, self.depth = height, width, hidden, depth
        self.row_begin, self.row_end = row_begin, (row_end if row_end else height)
        self.npix = (self.row_end - self.row_begin) * width
        self.out_features = out_features
        self._target = None
        self._views = {}

    def _outputs(self, shape, want_u8: bool, want_pred: bool, bits: int = 8):
        """(samples, pred, their device pointers) of a render call: `shape` uint8 (bits = 8) or uint16 (bits = 16) / fp32 on
        this device, None where not asked"""
        if not (want_u8 or want_pred):
            raise ValueError("render: ask for bytes, the fp32 prediction, or both")
        u8 = torch.empty(shape, dtype=torch.uint16 if bits == 16 else torch.uint8, device=self.device) if want_u8 else None
        pred = torch.empty(shape, device=self.device) if want_pred else None
        return u8, pred, (u8.data_ptr() if want_u8 else None), (pred.data_ptr() if want_pred else None)

    def _view(self, key: str, fn, *args, n: Optional[int] = None, typestr: str = "<f4") -> torch.Tensor:
        """Cached zero-copy view of engine-owned memory: fn(h, *args, &ptr[, &count]); an entry point that reports no count
        gets `n`"""
        if key not in self._views:
            p, cnt = C.c_void_p(), C.c_int64(n or 0)
            _check(fn(self.h, *args, C.byref(p), *(() if n else (C.byref(cnt),))))
            self._views[key] = torch.as_tensor(_DevView(p.value, cnt.value, typestr), device=self.device)
        return self._views[key]

    def _draw(self, name: str, shape, want_u8: bool, want_pred: bool, bits: int, *window):
        """The one render call: entry point `name` (bits = 16: `name`16), the outputs of `shape`, the call (`window`: the
        arguments between the handle and the outputs), no host sync: (samples or None, pred or None)"""
        fn = _render_entry(self.lib, name, bits)
        u8, pred, u8_p, pred_p = self._outputs(shape, want_u8, want_pred, bits)
        _check(fn(self.h, *window, u8_p, pred_p))
        return u8, pred

    def render(self, want_u8: bool = True, want_pred: bool = False, bits: int = 8):
        """type(self)._RENDER (sf_render) on this handle's rows, no host sync: (rgb8 [rows, W, C] uint8 or None, pred
        [rows, W, C] fp32 or None).  u8 = min(max((int)(pred * 255), 0), 255); pred is bit-identical to forward()'s.
        bits=16: sf_render16, the samples are uint16, min(max((int)(pred * 65535), 0), 65535)."""
        _require(self.lib, has_render, "sf_render entry point", "the render path")
        return self._draw(self._RENDER, (self.row_end - self.row_begin, self.width, self.out_features), want_u8, want_pred, bits)

    @property
    def scratch_format(self) -> int:
        """sf_config.scratch_format in use (what 0 / auto resolved to; an auto handle moves to 16 when a mask is set)"""
        f = C.c_int32()
        _check(self.lib.sf_scratch_format(self.h, C.byref(f)))
        return f.value

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.sf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ---------------------------------------------------------------------------
    def param_offsets(self, layer: int):
        w, b = C.c_int64(), C.c_int64()
        _check(self.lib.sf_param_offset(self.h, layer, C.byref(w), C.byref(b)))
        return w.value, b.value

    def view(self, which: str) -> torch.Tensor:
        """Flat fp32 torch view (no copy) of engine state: params | grads | exp_avg | exp_avg_sq | masks."""
        return self._views[which] if which in self._views else self._view(
            which, self.lib.sf_state_ptr, self.STATE[which], n=self.num_params)

    def grad_view(self) -> torch.Tensor:
        """The engine's own flat fp32 gradient (zero-copy): what pixel-split ranks all-reduce in place."""
        return self.view("grads")

    def sse_view(self) -> torch.Tensor:
        """1-element float64 view of the device scalar the last pass wrote its sum of squared residuals to."""
        return self._view("sse", self.lib.sf_sse_ptr, n=1, typestr="<f8")

    def sse8_view(self) -> torch.Tensor:
        """1-element int64 view of the device word the last eval_sums() wrote its integer sum to."""
        _require(self.lib, has_eval, "sf_sse8_ptr entry point", "the device evaluation")
        return self._view("sse8", self.lib.sf_sse8_ptr, n=1, typestr="<i8")

    def debug_scratch(self, which: str) -> torch.Tensor:
        """uint8 view of an engine scratch tensor of the last pass: phases | deltas | dlast | slabs (tests only)."""
        p, n = C.c_void_p(), C.c_int64()
        _check(self.lib.sf_debug_scratch(self.h, {"phases": 0, "deltas": 1, "dlast": 2, "slabs": 3}[which], C.byref(p), C.byref(n)))
        return torch.as_tensor(_DevView(p.value, n.value, "|u1"), device=self.device)

    def kmeans_fit(self, weight: torch.Tensor, guess: torch.Tensor, iter_limit: int = 5, tol: float = 1e-4,
                   centres_out: Optional[torch.Tensor] = None):
        """sf_kmeans_fit on this handle's stream, no host sync: (centroids [K+1, zero padded], n_centroids [device int32],
        labels [int64, weight's shape], new_weight).  The guess is left as it is; centres_out (float32 [K] on the device)
        receives what the call leaves in centers_dev, the Lloyd centres."""
        w = _f32_cuda(weight.reshape(-1))
        guess = _f32_cuda(guess.reshape(-1))
        centers = guess.clone() if centres_out is None else _f32_cuda(centres_out, guess.numel()).copy_(guess)
        K = centers.numel()
        cent = torch.empty(K + 1, device=self.device)
        ncent = torch.empty(1, dtype=torch.int32, device=self.device)
        labels = torch.empty(w.numel(), dtype=torch.int64, device=self.device)
        new_w = torch.empty_like(w)
        _check(self.lib.sf_kmeans_fit(self.h, w.data_ptr(), w.numel(), centers.data_ptr(), K, iter_limit, tol, cent.data_ptr(), K + 1,
                                      ncent.data_ptr(), labels.data_ptr(), new_w.data_ptr()))
        return cent, ncent, labels.reshape(weight.shape), new_w.reshape(weight.shape)

    def quant_args(self, layers: Sequence[int], centres, centroids, n_centroids, labels, K: int, iter_limit: int = 5,
                   tol: float = 1e-4, nudge_lr: float = 0.0) -> sf_quant_args:
        """the argument struct of quant_pass / quant_nudge / quant_step: `layers` (ascending engine layer indices) with, per
        layer, the caller's device buffers - centres float32 [K], centroids float32 [K + 1], n_centroids int32 [1] (or None),
        labels int64 [the layer's weight count].  The struct keeps the buffers alive."""
        if not (len(layers) == len(centres) == len(centroids) == len(n_centroids) == len(labels)):
            raise ValueError("quant_args: one buffer of each kind per layer")
        rows = (sf_quant_layer * max(len(layers), 1))()
        for j, l in enumerate(layers):
            w, b = self.param_offsets(l)
            lab, nc = labels[j], n_centroids[j]
            if not (lab.is_cuda and lab.dtype == torch.int64 and lab.is_contiguous() and lab.numel() == b - w):
                raise ValueError(f"quant_args: labels of layer {l} must be a contiguous int64 CUDA tensor of {b - w} elements")
            if nc is not None and not (nc.is_cuda and nc.dtype == torch.int32 and nc.numel() >= 1):
                raise ValueError("quant_args: n_centroids must be an int32 CUDA tensor")
            rows[j] = sf_quant_layer(layer=l, centers_dev=_f32_cuda(centres[j], K).data_ptr(),
                                     centroids_dev=_f32_cuda(centroids[j], K + 1).data_ptr(),
                                     n_centroids_dev=None if nc is None else nc.data_ptr(), labels_dev=lab.data_ptr())
        args = sf_quant_args(abi_version=SF_ABI_VERSION, n_layers=len(layers), layers=rows, K=K, iter_limit=iter_limit, tol=tol,
                             nudge_lr=nudge_lr)
        args._keep = (rows, list(centres), list(centroids), list(n_centroids), list(labels))
        return args

    def quant_pass(self, args: sf_quant_args):
        """sf_quant_pass on this handle's stream, no host sync: per listed layer the guess, the Lloyd iterations, the
        centroids and labels into the caller's buffers, the codebook weights into the handle's params"""
        _require(self.lib, has_quant_step, "sf_quant_pass entry point", "the device quantise phase")
        _check(self.lib.sf_quant_pass(self.h, C.byref(args)))

    def quant_nudge(self, args: sf_quant_args):
        """sf_quant_nudge, no host sync: centroids[k] -= nudge_lr * (sum of the handle's grads over the weights labelled k)"""
        _require(self.lib, has_quant_step, "sf_quant_nudge entry point", "the device quantise phase")
        _check(self.lib.sf_quant_nudge(self.h, C.byref(args)))

    def quant_step(self, args: sf_quant_args, lrs: Sequence[float], want_loss: bool = False):
        """sf_quant_step: len(lrs) x (pass, forward_backward, nudge, Adam) in one call; the losses (one read at the end) or None"""
        _require(self.lib, has_quant_step, "sf_quant_step entry point", "the device quantise phase")
        n = len(lrs)
        arr = (C.c_float * max(n, 1))(*lrs)
        out = (C.c_float * max(n, 1))() if want_loss else None
        _check(self.lib.sf_quant_step(self.h, C.byref(args), arr, n, out))
        return list(out)[:n] if want_loss else None

    def mask_update(self, layers: Sequence[int], prune_rate: float, growth: int, dense_gradients: bool,
                    stats: Optional[torch.Tensor] = None):
        """sf_mask_update on this handle's stream, no host sync: one RigL topology update of the weights of `layers`
        (ascending engine layer indices) in the handle's params / grads / moments / masks.  stats: int64
        [len(layers) + 1, MASK_STATS_WORDS] on the device or None - a sf_mask_layer_stats per layer (the last word is the
        bits of the double prune rate) and the status row."""
        self._mask_call("sf_mask_update", sf_mask_update_args, has_mask_update, "the device topology update", layers, stats,
                        prune_rate=float(prune_rate), growth=int(growth), dense_gradients=int(bool(dense_gradients)))

    def mask_prune_global(self, layers: Sequence[int], target: int, prune_rate: float, threshold: float, increment: float,
                          tolerance: float, dense_gradients: bool, stats: Optional[torch.Tensor] = None):
        """sf_mask_prune_global on this handle's stream, no host sync: one global-magnitude topology update of the weights of
        `layers` - the threshold search from `threshold` towards `target` removed weights, the masks |w| > threshold, the
        products.  stats: int64 [len(layers) + 1, MASK_STATS_WORDS] on the device or None - a sf_mask_layer_stats per layer and
        the status row (status, trials, alive, removed, target, 0, 0, the bits of the final threshold)."""
        self._mask_call("sf_mask_prune_global", sf_mask_prune_global_args, has_mask_prune_global,
                        "the device global pruning update", layers, stats, target=int(target), prune_rate=float(prune_rate),
                        threshold=float(threshold), increment=float(increment), tolerance=float(tolerance),
                        dense_gradients=int(bool(dense_gradients)))

    def mask_update_snfs(self, layers: Sequence[int], prune_rate: float, adjusted_growth: float, growth: int, statistic: int,
                         dense_gradients: bool, stats: Optional[torch.Tensor] = None):
        """sf_mask_update_snfs on this handle's stream, no host sync: one SNFS topology update of the weights of `layers` -
        the redistribution statistic, the prune, the regrowth budgets, the growth (MASK_GROWTH), the products.  stats: int64
        [len(layers) + 1, MASK_SNFS_STATS_WORDS] on the device or None - a sf_mask_snfs_stats per layer and the status row
        (status, rounds, removed in all, grown in all, ..., the pool, the norm before, ..., the norm after)."""
        self._mask_call("sf_mask_update_snfs", sf_mask_update_snfs_args, has_mask_update_snfs, "the device SNFS update", layers,
                        stats, words=MASK_SNFS_STATS_WORDS, prune_rate=float(prune_rate), adjusted_growth=float(adjusted_growth),
                        growth=int(growth), statistic=int(statistic), dense_gradients=int(bool(dense_gradients)))

    def _mask_call(self, entry, args_type, has, what, layers, stats, words=MASK_STATS_WORDS, **fields):
        """one topology update entry point: the library has it, `stats` is a statistics table of `words`-word rows for
        `layers`, the call"""
        _require(self.lib, has, f"{entry} entry point", what)
        n = len(layers)
        if stats is not None and not (stats.is_cuda and stats.dtype == torch.int64 and stats.is_contiguous()
                                      and stats.numel() == (n + 1) * words):
            raise ValueError(f"{entry[3:]}: stats must be a contiguous int64 CUDA tensor of {(n + 1) * words} words")
        args = args_type(abi_version=SF_ABI_VERSION, n_layers=n, layers=(C.c_int32 * max(n, 1))(*layers),
                         stats_dev=None if stats is None else stats.data_ptr(), **fields)
        _check(getattr(self.lib, entry)(self.h, C.byref(args)))

    def params_changed(self):
        _check(self.lib.sf_params_changed(self.h))

    def set_params(self, flat: torch.Tensor):
        _check(self.lib.sf_set_params(self.h, _f32_cuda(flat, self.num_params).data_ptr()))

    def get_params(self) -> torch.Tensor:
        out = torch.empty(self.num_params, device=self.device)
        _check(self.lib.sf_get_params(self.h, out.data_ptr()))
        return out

    def get_grads(self) -> torch.Tensor:
        out = torch.empty(self.num_params, device=self.device)
        _check(self.lib.sf_get_grads(self.h, out.data_ptr()))
        return out

    def set_grads(self, flat: torch.Tensor):
        _check(self.lib.sf_set_grads(self.h, _f32_cuda(flat, self.num_params).data_ptr()))

    def set_masks(self, flat: Optional[torch.Tensor]):
        _check(self.lib.sf_set_masks(self.h, None if flat is None else _f32_cuda(flat, self.num_params).data_ptr()))

    def get_adam_state(self):
        m = torch.empty(self.num_params, device=self.device)
        v = torch.empty(self.num_params, device=self.device)
        step = C.c_int64()
        _check(self.lib.sf_get_adam_state(self.h, m.data_ptr(), v.data_ptr(), C.byref(step)))
        return m, v, step.value

    def set_adam_state(self, m: torch.Tensor, v: torch.Tensor, step: int):
        _check(self.lib.sf_set_adam_state(self.h, _f32_cuda(m, self.num_params).data_ptr(),
                                          _f32_cuda(v, self.num_params).data_ptr(), step))

    # ---- data ----------------------------------------------------------------------------
    def set_coords(self, rows: torch.Tensor, cols: torch.Tensor):
        _check(self.lib.sf_set_coords(self.h, _f32_cuda(rows, self.height).data_ptr(),
                                      _f32_cuda(cols, self.width).data_ptr()))

    def set_target(self, img: torch.Tensor):
        self._target = _f32_cuda(img, self.npix * self.out_features)  # keep alive: the engine borrows it
        _check(self.lib.sf_set_target(self.h, self._target.data_ptr()))

    # ---- hot path ------------------------------------------------------------------------
    def forward(self, want_pred: bool = True, want_sse: bool = True):
        pred = torch.empty(self.row_end - self.row_begin, self.width, self.out_features,
                           device=self.device) if want_pred else None
        sse = C.c_double()
        _check(self.lib.sf_forward(self.h, pred.data_ptr() if want_pred else None,
                                   C.byref(sse) if want_sse else None))
        return pred, (sse.value if want_sse else None)

    def eval_sums(self, sync: bool = True):
        """sf_eval: one evaluation pass that writes no prediction.  (sse, sse8): the double forward() reports and the exact
        sum of ((img * 255).int() - (pred * 255).int()) ** 2 over this handle's rows, read with one copy.  sync=False: the
        pass is enqueued and nothing is read - (None, None); the sums are in sse_view() / sse8_view()."""
        _require(self.lib, has_eval, "sf_eval entry point", "the device evaluation")
        sse, sse8 = C.c_double(), C.c_uint64()
        _check(self.lib.sf_eval(self.h, C.byref(sse) if sync else None, C.byref(sse8) if sync else None))
        return (sse.value, sse8.value) if sync else (None, None)

    def forward_backward(self, sync: bool = True) -> Optional[float]:
        sse = C.c_double()
        _check(self.lib.sf_forward_backward(self.h, C.byref(sse) if sync else None))
        return sse.value if sync else None

    def adam_step(self, lr: float):
        _check(self.lib.sf_adam_step(self.h, lr))

    def step(self, lrs: Sequence[float], want_loss: bool = False):
        n = len(lrs)
        arr = (C.c_float * n)(*lrs)
        out = (C.c_float * n)() if want_loss else None
        _check(self.lib.sf_step(self.h, arr, n, out))
        return list(out) if want_loss else None

    # ---- Feathermap (sf_feather_*) ----------------------------------------------------------
    FEATHER = {"params": 0, "grads": 1, "exp_avg": 2, "exp_avg_sq": 3, "V": 4}

    def feather_attach(self, n: int, m: int, logical_out: Sequence[int], logical_in: Sequence[int]):
        _require(self.lib, has_feather, "sf_feather_* entry points", "Feathermap")
        D = len(logical_out)
        outs, ins = (C.c_int32 * D)(*logical_out), (C.c_int32 * D)(*logical_in)
        _check(self.lib.sf_feather_attach(self.h, n, m, D, outs, ins))

    def feather_view(self, which: str) -> torch.Tensor:
        """Flat fp32 view (no copy) of the feather state: params | grads | exp_avg | exp_avg_sq ([V1 | V2 | scalers]),
        or V (the unscaled V[0, P) of the last materialisation)."""
        key = "feather/" + which
        return self._views[key] if key in self._views else self._view(
            key, self.lib.sf_feather_state_ptr, self.FEATHER[which])

    def feather_materialise(self):
        _check(self.lib.sf_feather_materialise(self.h))

    def feather_adjoint(self):
        _check(self.lib.sf_feather_adjoint(self.h))

    @property
    def adam_steps(self) -> int:
        step = C.c_int64()
        _check(self.lib.sf_get_adam_state(self.h, None, None, C.byref(step)))
        return step.value

    @adam_steps.setter
    def adam_steps(self, step: int):
        _check(self.lib.sf_set_adam_state(self.h, None, None, int(step)))

    def set_graph_replay(self, on: bool):
        """step(): replay a captured hipGraph per training step instead of launching kernel by kernel"""
        _check(self.lib.sf_set_graph_replay(self.h, int(on)))

    # ---- measurement -----------------------------------------------------------------------
    def profile(self, on: bool):
        _check(self.lib.sf_profile_enable(self.h, int(on)))

    def profile_reset(self):
        _check(self.lib.sf_profile_reset(self.h))

    def profile_report(self):
        n = C.c_int32()
        _check(self.lib.sf_profile_num_kernels(self.h, C.byref(n)))
        rep = {}
        for i in range(n.value):
            name, ms, cnt, fl, by = C.c_char_p(), C.c_double(), C.c_int64(), C.c_double(), C.c_double()
            _check(self.lib.sf_profile_get(self.h, i, C.byref(name), C.byref(ms), C.byref(cnt), C.byref(fl),
                                           C.byref(by)))
            rep[name.value.decode()] = {"total_ms": ms.value, "launches": cnt.value,
                                        "flops_per_launch": fl.value, "bytes_per_launch": by.value}
        return rep


class RenderEngine(SirenEngine):
    """Inference-only handle (sf_render_create): parameters, forward weight images and the two coordinate vectors - no
    gradient, optimiser state, mask or backward scratch.  set_params / get_params / set_coords / render / the profiling
    calls work; every training call raises with the library's message.  set_coords takes any two vectors (a window of a
    grid is a slice of its linspace vectors); hidden 512 / 1024 is refused (WideRenderEngine is that handle; FourierNet
    has FourierRenderEngine, WaveletSiren has WaveletRenderEngine, a Feathermap fit FeatherRenderEngine)."""

    def __init__(self, height: int, width: int, hidden: int, depth: int, first_omega_0: float = 50.0,
                 hidden_omega_0: float = 30.0, outermost_linear: bool = True, out_features: int = 3,
                 compute_dtype: str = "f16", device: int = 0, row_begin: int = 0, row_end: int = 0, chunk_pixels: int = 0):
        super().__init__(height, width, hidden, depth, first_omega_0, hidden_omega_0, outermost_linear, out_features,
                         compute_dtype, device, row_begin, row_end, chunk_pixels)

    _CREATE, _CREATE_NEEDS = "sf_render_create", (has_render, "sf_render_create entry point", "the render path")


class WideRenderEngine(RenderEngine):
    """Inference-only handle of a SIREN of hidden 512 / 1024 (sf_wide_render_create): parameters, the blocked forward weight
    images, the layer-0 table, the two coordinate vectors and two activation planes of chunk_pixels x hidden 16-bit values
    that the layers use in turn - none of the per-layer phase / activation / delta planes, transposed images, gradient,
    optimiser state or mask of a training handle.  chunk_pixels = 0: 2^18 pixels at 512, 2^17 at 1024.  Everything
    RenderEngine says holds; render() is sf_wide_render / sf_wide_render16, pred bit-identical to SirenEngine.forward()'s."""

    _CREATE = "sf_wide_render_create"
    _CREATE_NEEDS = (has_wide_render, "sf_wide_render_create entry point", "the wide render path")
    _RENDER = "sf_wide_render"


class FeatherRenderEngine(RenderEngine):
    """Inference-only handle of a Feathermap fit (sf_render_create + sf_feather_render_attach): what RenderEngine holds plus
    the feather vector [V1 | V2 | scalers] of feather_elems floats - no gradient, moments, unscaled V or adjoint scratch.
    load_feather materialises W = scaler * (V1 V2) with the training handle's own fixed-order product, so get_params and
    render are bit-identical to a FeatherNet training handle's with the same vector.  n, m: the sides of V1 [n, m] and
    V2 [m, n]; logical_out / logical_in: each Linear's logical size (hidden is the engine width, which may be padded).
    set_params raises with the library's message: the parameters belong to the feather vector."""

    def __init__(self, height: int, width: int, hidden: int, depth: int, n: int, m: int, logical_out: Sequence[int],
                 logical_in: Sequence[int], first_omega_0: float = 50.0, hidden_omega_0: float = 30.0,
                 outermost_linear: bool = True, out_features: int = 3, compute_dtype: str = "f16", device: int = 0,
                 row_begin: int = 0, row_end: int = 0, chunk_pixels: int = 0):
        _require(load_library(), has_feather, "sf_feather_render_* entry points", "the Feathermap render path")
        super().__init__(height, width, hidden, depth, first_omega_0, hidden_omega_0, outermost_linear, out_features,
                         compute_dtype, device, row_begin, row_end, chunk_pixels)
        D = len(logical_out)
        try:
            _check(self.lib.sf_feather_render_attach(self.h, n, m, D, (C.c_int32 * D)(*logical_out),
                                                     (C.c_int32 * D)(*logical_in)))
        except Exception:
            self.close()
            raise
        self.feather_elems = 2 * n * m + 2 * D

    def load_feather(self, flat: torch.Tensor):
        """sf_feather_render_load: [V1 | V2 | scalers] (fp32, on the device, copied), then W; no host sync"""
        _check(self.lib.sf_feather_render_load(self.h, _f32_cuda(flat, self.feather_elems).data_ptr()))


_FOURIER_RENDER = (has_fourier_render, "sf_fourier_render_create entry point", "the FourierNet render path")


class FourierEngine(SirenEngine):
    """FourierNet fit on one HIP stream: an sf_handle made by sf_fourier_create (fourier_kernels.hip).  Every method of
    SirenEngine applies (render() included: sf_render's RENDER form of k_ff_fwd); the frozen encoding goes in through
    set_encoding before the first pass."""

    def __init__(self, height: int, width: int, hidden: int, n_linear: int, map_size: int, out_features: int = 3,
                 device: int = 0, chunk_pixels: int = 0, betas=(0.9, 0.999), eps: float = 1e-8):
        cfg = sf_fourier_config(height=height, width=width, in_features=2, out_features=out_features, map_size=map_size,
                                hidden=hidden, n_linear=n_linear, beta1=betas[0], beta2=betas[1], eps=eps,
                                chunk_pixels=chunk_pixels)
        self._open(cfg, device, height, width, hidden, n_linear, out_features)
        self.map_size = map_size

    _CREATE = "sf_fourier_create"
    mask_update = None          # sf_mask_update refuses a FourierNet handle: Masking keeps such a model on the host path
    mask_prune_global = None    # (sf_mask_prune_global likewise)
    mask_update_snfs = None     # (sf_mask_update_snfs likewise)
    quant_step = None           # sf_quant_step refuses this handle: KmeansQuant keeps such a model on the host path

    def set_encoding(self, B: torch.Tensor):
        """encoding.B [2, map_size/2] (fp32, copied into the engine)"""
        _check(self.lib.sf_set_encoding(self.h, _f32_cuda(B.detach().contiguous(), 2 * (self.map_size // 2)).data_ptr()))

    def render(self, want_u8: bool = True, want_pred: bool = False, bits: int = 8):
        _require(self.lib, *_FOURIER_RENDER)
        return super().render(want_u8, want_pred, bits)


class FourierRenderEngine(FourierEngine):
    """Inference-only FourierNet handle (sf_fourier_render_create, csrc/fourier_render.hip): parameters, the fp16 weight
    images, encoding.B and the two coordinate vectors - none of the activation / gradient planes, slabs, gradient, optimiser
    state, mask or SSE partials of FourierEngine.  set_params / get_params / set_encoding / set_coords / render / the
    profiling calls work; every training call raises with the library's message.  set_coords takes any two vectors (a
    window or a band of a grid is a slice of its linspace vectors)."""

    def __init__(self, height: int, width: int, hidden: int, n_linear: int, map_size: int, out_features: int = 3,
                 device: int = 0, chunk_pixels: int = 0):
        super().__init__(height, width, hidden, n_linear, map_size, out_features, device, chunk_pixels)

    _CREATE, _CREATE_NEEDS = "sf_fourier_render_create", _FOURIER_RENDER


class WaveletEngine(SirenEngine):
    """WaveletSiren fit on one HIP stream: an sf_handle made by sf_wavelet_create (two SIREN sub-networks on the n x n
    coefficient grid, wavelet_kernels.hip for the image).  Every method of SirenEngine applies: the flat vectors are
    [LF | HF], forward() returns the H x H x 3 RGB prediction."""

    def __init__(self, height: int, width: int, hidden: int, depth: int, first_omega_0: float = 50.0,
                 hidden_omega_0: float = 30.0, outermost_linear: bool = True, device: int = 0, chunk_pixels: int = 0,
                 betas=(0.9, 0.999), eps: float = 1e-8, wavelet_levels: int = 1):
        _require(load_library(), has_wavelet, "sf_wavelet_* entry points", "WaveletSiren")      # before the GPU is asked for
        cfg = sf_wavelet_config(height=height, width=width, in_features=2, out_features=3, hidden=hidden, depth=depth,
                                wavelet_levels=wavelet_levels, first_omega_0=first_omega_0, hidden_omega_0=hidden_omega_0,
                                outermost_linear=int(bool(outermost_linear)), beta1=betas[0], beta2=betas[1], eps=eps,
                                chunk_pixels=chunk_pixels, scratch_format=16)
        self._open(cfg, device, height, width, hidden, depth, who="WaveletEngine")
        self.n = (height + 5) // 2

    _CREATE = "sf_wavelet_create"
    mask_update = None          # sf_mask_update refuses a WaveletSiren handle: its topology updates stay on the host
    mask_prune_global = None    # (sf_mask_prune_global likewise)
    mask_update_snfs = None     # (sf_mask_update_snfs likewise)
    quant_step = None           # sf_quant_step refuses this handle: KmeansQuant keeps such a model on the host path

    def set_coords(self, rows: torch.Tensor, cols: torch.Tensor):
        """rows / cols: the linspace(0, 1, n) vectors of the coefficient grid (n = (H + 5) // 2)"""
        _check(self.lib.sf_set_coords(self.h, _f32_cuda(rows, self.n).data_ptr(), _f32_cuda(cols, self.n).data_ptr()))

    def render_window(self, r0: int, r1: int, c0: int, c1: int, want_u8: bool = True, want_pred: bool = False, bits: int = 8):
        """sf_wavelet_render of pixel rows [r0, r1) x columns [c0, c1) on this handle, no host sync:
        (rgb8 [r1 - r0, c1 - c0, 3] uint8 or None, pred fp32 or None); bits=16: sf_wavelet_render16, uint16 samples"""
        return _wavelet_render(self, r0, r1, c0, c1, want_u8, want_pred, bits)

    def debug_compose(self, lf: torch.Tensor, hf: torch.Tensor, img: Optional[torch.Tensor] = None):
        """k_wv_compose on [n, n, 3] sub-network predictions: (RGB [H, H, 3], dL/d(Y, Cb, Cr) [H, H, 3] or None)"""
        nn3, hh3 = self.n * self.n * 3, self.npix * 3
        pred = torch.empty(self.height, self.width, 3, device=self.device)
        g = torch.zeros(self.height, self.width, 3, device=self.device)
        _check(self.lib.sf_wavelet_debug(self.h, 0, _f32_cuda(lf, nn3).data_ptr(), _f32_cuda(hf, nn3).data_ptr(),
                                         None if img is None else _f32_cuda(img, hh3).data_ptr(), pred.data_ptr(),
                                         g.data_ptr()))
        return pred, (g if img is not None else None)

    def debug_adjoint(self, g: torch.Tensor):
        """k_wv_adjoint (unscaled) of dL/d(Y, Cb, Cr) [H, H, 3]: (dL/dp of LF, of HF), [n, n, 3] each"""
        lf = torch.empty(self.n, self.n, 3, device=self.device)
        hf = torch.empty(self.n, self.n, 3, device=self.device)
        _check(self.lib.sf_wavelet_debug(self.h, 1, _f32_cuda(g, self.npix * 3).data_ptr(), None, None, lf.data_ptr(),
                                         hf.data_ptr()))
        return lf, hf


def _wavelet_render(eng, r0: int, r1: int, c0: int, c1: int, want_u8: bool, want_pred: bool, bits: int = 8):
    _require(eng.lib, has_wavelet_render, "sf_wavelet_render entry point", "the WaveletSiren render path")
    return eng._draw("sf_wavelet_render", (max(r1 - r0, 0), max(c1 - c0, 0), 3), want_u8, want_pred, bits, r0, r1, c0, c1)


class WaveletRenderEngine(WaveletEngine):
    """Inference-only WaveletSiren handle (sf_wavelet_render_create, csrc/wavelet_render.hip): the joint parameters [LF | HF],
    two render sub-handles, the two full coefficient-grid vectors and one pair of coefficient buffers sized for a
    max_rows x max_cols pixel window (0 = the whole picture) - no gradient, optimiser state, mask, backward scratch or
    image-space gradient.  set_params / get_params / set_coords (the linspace(0, 1, n) vectors of the FULL coefficient
    grid) / render / the profiling calls work; every training call raises with the library's message."""

    def __init__(self, height: int, hidden: int, depth: int, first_omega_0: float = 50.0, hidden_omega_0: float = 30.0,
                 outermost_linear: bool = True, compute_dtype: str = "f16", max_rows: int = 0, max_cols: int = 0,
                 device: int = 0, chunk_pixels: int = 0):
        _require(load_library(), has_wavelet_render, "sf_wavelet_render_create entry point", "the WaveletSiren render path")
        cfg = sf_wavelet_render_config(height=height, max_rows=max_rows, max_cols=max_cols, hidden=hidden, depth=depth,
                                       first_omega_0=first_omega_0, hidden_omega_0=hidden_omega_0,
                                       outermost_linear=int(bool(outermost_linear)), chunk_pixels=chunk_pixels)
        self._open(cfg, device, height, height, hidden, depth, compute_dtype=compute_dtype)
        self.n = (height + 5) // 2
        self.max_rows, self.max_cols = max_rows or height, max_cols or height

    _CREATE = "sf_wavelet_render_create"

    def render(self, r0: int = 0, r1: Optional[int] = None, c0: int = 0, c1: Optional[int] = None, want_u8: bool = True,
               want_pred: bool = False, bits: int = 8):
        """pixel rows [r0, r1) x columns [c0, c1) of the height x height picture (default: all of it), no host sync:
        (rgb8 [rows, cols, 3] uint8 or None, pred [rows, cols, 3] fp32 or None).  u8 = min(max((int)(pred * 255), 0), 255);
        pred is bit-identical to WaveletEngine.forward()'s for the same pixels.  bits=16: sf_wavelet_render16, uint16
        samples, min(max((int)(pred * 65535), 0), 65535)."""
        return _wavelet_render(self, r0, self.height if r1 is None else r1, c0, self.height if c1 is None else c1,
                               want_u8, want_pred, bits)


class FeatherEngine:
    """A SIREN handle with a feather state (sf_feather_attach), as the optimiser seams see it: view('params' | 'grads' |
    'exp_avg' | 'exp_avg_sq') are the feather vector [V1 | V2 | scalers] and its gradient and Adam moments, so EngineAdam
    binds to them unchanged.  Everything else (forward, step, adam_step, profile, dense views through .base) is the
    SirenEngine's."""

    def __init__(self, base: SirenEngine):
        self.base = base

    def __getattr__(self, name):
        return getattr(self.base, name)

    def view(self, which: str) -> torch.Tensor:
        if which in ("params", "grads", "exp_avg", "exp_avg_sq"):
            return self.base.feather_view(which)
        return self.base.view(which)
