"""`make decode` entry: turn a run directory written by `fit` back into a picture.

    python -m implicit_image.decode decode.dir=outputs/<image>/<experiment>/<tag> [key=value ...]

Loads `model_quantized/` (compressed_weights.data + meta_data.json, through decompress_state_dict: codebook layers come
back dense, fp16 values widened to fp32) when present, else `model.pth`; `decode.source=container|pth` forces one.  The
model shape comes from `decode.json`, which `fit` writes next to them; the same key=value overrides as `fit` replace any
of it, so a container written before that file existed (or by the reference) decodes with `mlp.hidden_size=... mlp.depth=...
img.height=... img.width=...` on the command line.

decode.* keys
  decode.dir        the run directory (required)
  decode.source     container | pth (default: the container when there is one)
  decode.height, decode.width   output size (default: the fitted size); any other size renders the same unit square at
                    that resolution (torch.linspace(0, 1, n) per axis, the reference's get_grid)
  decode.rows=a:b decode.cols=c:d   a window of that grid (the coordinate vectors are sliced on the host)
  decode.band_rows  rows rendered per kernel call (default: as many as keep one band's bytes under 256 MiB)
  decode.out        the PPM to write (default <decode.dir>/decoded.ppm; binary P6, 8 bit, or 16 bit with decode.bits=16)
  decode.bits       8 | 16 (default 8): bits per sample of the file.  16: u16 = min(max(trunc(pred * 65535), 0), 65535) from
                    the render kernels' 16-bit epilogue (sf_render16 / sf_wavelet_render16; the torch path: to_u16), written
                    as P6 with maxval 65535 (big-endian samples, what the loader reads back).  Truncation to 256 levels caps
                    a file at 10 log10(3 * 255^2) = 52.9 dB against its own fp32 prediction; at 16 bits that is 101 dB
  decode.truth      <ppm> or synthetic[:seed]: print loss / PSNR / PSNR_8bit with eval_epoch's formulas (decode.bits=16:
                    and PSNR_16bit, the same formula on 65535 levels)
  decode.device     cuda ordinal (default 0)
  decode.render     auto | kernel | wide | torch (default auto).  auto: what `render_path` answers, below.  torch: the registry
                    model's own forward for any model.  kernel: a render kernel or a ValueError that says why there is
                    none for this model and picture (`kernel_available`), raised before the device is touched; this is
                    how mlp=fourier decodes on its render kernel.  wide: the wide render handle of a plain SIREN whose
                    engine width is 512 or 1024 (depth >= 3), or a ValueError that says what decodes the model instead,
                    raised as early; auto and kernel leave those widths where they were

Four model families decode; `family` looks a run's up once from its shape.  Each has a render kernel at engine width 32 /
64 / 128 / 256 (a Small_Dense width the engine zero-pads, 90 -> 128, runs at the padded width): bytes straight from the last
epilogue, no training state or activation plane on the device.  `_render` does that job for all four: the family's CPU
model builds and fills the handle (models/binding.py); a band is a slice of the coordinate vectors or, for WaveletSiren,
a pixel window.  Without a kernel (a WaveletSiren picture that is not even and square) or under decode.render=torch the
same model runs its own forward on the device, bytes by the same formula in torch; so does a SIREN of width 512 / 1024 -
through a full training handle - unless decode.render=wide asks for its render handle (two activation planes of a chunk and
the forward images; the same `_render`, bands and windows).  The log names the path.

  family          auto runs   kernel runs                           engine class          entry points
  siren           kernel      sf_render                             RenderEngine          render_kernel, load_weights
  siren 512/1024  torch       sf_wide_render (decode.render=wide)   WideRenderEngine      render_kernel, load_weights
  feather         kernel      sf_feather_render_load + sf_render    FeatherRenderEngine   render_feather, load_feather
  fourier         torch       sf_render (RENDER form of k_ff_fwd)   FourierRenderEngine   render_fourier, load_weights
  wavelet_siren   kernel      sf_wavelet_render                     WaveletRenderEngine   render_wavelet, load_weights

feather is SIREN under masking=Feathermap: model.pth holds the feather vector [V1 | V2 | scalers] and there is no container;
the handle forms W = scaler * (V1 V2) by the engine's own fixed-order product: bit for bit the picture `fit` logged the PSNR of.
"""
import json
import logging
import math
import os
import sys
from collections import OrderedDict
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from .config import Cfg, _load_yaml, _parse_scalar, _set_path, _wrap
from .data import get_grid, load_img, read_ppm, write_ppm, write_ppm16
from .models import registry
from .models.fourier import MAP_SIZES as FOURIER_MAPS, engine_takes as fourier_engine_takes
from .models.siren import KERNEL_WIDTHS, Siren, layer_sizes, next_kernel_width
from .models.wavelet_siren import check_image

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
DECODE_JSON = "decode.json"
BAND_BYTES = 256 << 20            # one band's byte output stays under this
ROW_LIMIT = 1 << 40               # a handle decodes (row, col) exactly while rows * width^2 < 2^40 (sf_create)
RENDER_MODES = ("auto", "kernel", "wide", "torch")
WIDE_WIDTHS = tuple(w for w in Siren.WIDTHS if w not in KERNEL_WIDTHS)      # the layer-at-a-time kernels: 512, 1024
SAMPLE_BITS = (8, 16)
SHAPE_KEYS = ("mlp.depth", "mlp.hidden_size")


# ---- decode.json ------------------------------------------------------------------------------------------
def write_decode_json(out_dir: str, cfg, state_dict_keys: Sequence[str]) -> str:
    """What a decoder needs to rebuild the network of a fit: the resolved mlp section, the fitted size, the entropy_coding
    section, the masking that shaped the stored network (name; Small_Dense density) and the state-dict key list."""
    masking = cfg.get("masking") or {}
    rec = {
        "mlp": dict(cfg["mlp"]),
        "img": {"height": int(cfg["img"]["height"]), "width": int(cfg["img"]["width"])},
        "entropy_coding": dict(cfg.get("entropy_coding") or {}),
        "engine": dict(cfg.get("engine") or {}),
        "masking_name": masking.get("name"),
        "small_dense_density": float(masking["density"]) if masking.get("name") == "Small_Dense" else None,
        "state_dict_keys": [str(k) for k in state_dict_keys],
    }
    path = os.path.join(out_dir, DECODE_JSON)
    with open(path, "w") as f:
        json.dump(rec, f, indent=2, sort_keys=True)
    return path


def split_overrides(argv: Sequence[str]) -> Tuple[Dict[str, str], List[str]]:
    """decode.* keys (raw strings: `a:b` ranges are not YAML scalars) and the fit-style overrides"""
    dec, rest = {}, []
    for ov in argv:
        key, eq, val = ov.partition("=")
        if not eq:
            raise ValueError(f"override '{ov}' is not key=value")
        if key.startswith("decode."):
            dec[key[len("decode."):]] = val
        else:
            rest.append(ov)
    return dec, rest


def resolve_shape(run_dir: str, overrides: Sequence[str] = (), conf_dir: Optional[str] = None) -> Cfg:
    """decode.json of the run directory with `key=value` overrides on top (overrides win; `mlp=fourier` /
    `entropy_coding=lzma` select a conf/ group file as in fit).  Without decode.json the overrides must name the network."""
    conf_dir = conf_dir or os.environ.get("IIC_CONF", os.path.join(REPO, "conf"))
    path, given = os.path.join(run_dir, DECODE_JSON), set()
    missing_file = not os.path.exists(path)
    if not missing_file:
        with open(path) as f:
            rec = json.load(f)
    else:
        rec = {"mlp": {"name": "siren", "first_omega_0": 50, "hidden_omega_0": 30, "outermost_linear": True},
               "img": {}, "entropy_coding": {"stream_name": "plain"}, "engine": {}, "masking_name": None,
               "small_dense_density": None, "state_dict_keys": None}
    for ov in overrides:
        key, _, val = ov.partition("=")
        key = key.lstrip("+")
        if "." not in key and os.path.isdir(os.path.join(conf_dir, key)):
            if key in ("mlp", "entropy_coding"):
                rec[key] = _load_yaml(os.path.join(conf_dir, key, f"{val}.yaml"))
            elif key == "masking":
                rec["masking_name"] = None if val == "none" else val
                sec = _load_yaml(os.path.join(conf_dir, key, f"{val}.yaml"))
                rec["small_dense_density"] = float(sec["density"]) if val == "Small_Dense" else None
            continue                                   # other groups (img, optim, quant) say nothing about the stored network
        if key == "masking.density":
            if rec.get("masking_name") == "Small_Dense":
                rec["small_dense_density"] = float(val)
            continue
        given.add(key)
        _set_path(rec, key, _parse_scalar(val))
    if missing_file:
        need = [k for k in SHAPE_KEYS if k not in given]
        if need:
            raise FileNotFoundError(
                f"{path} not found (a run written before `fit` recorded the model shape, or by the "
                f"reference): pass {' '.join(k + '=...' for k in need)} (and mlp=<name>, mlp.first_omega_0=..., "
                "mlp.hidden_omega_0=..., img.height=... img.width=... when they differ from the defaults) on the command line")
    return _wrap(rec)


# ---- weights ----------------------------------------------------------------------------------------------
def _check_source(source: Optional[str]):
    if source not in (None, "", "container", "pth"):
        raise ValueError(f"decode.source must be container or pth, got {source!r}")


def _fp32(sd) -> "OrderedDict[str, torch.Tensor]":
    return OrderedDict((k, v.detach().float().cpu()) for k, v in sd.items())


def read_pth(path: str) -> "OrderedDict[str, torch.Tensor]":
    """model.pth as `fit` saves it (the state dict, or a dict that holds it under 'state_dict'), fp32 on the CPU"""
    blob = torch.load(path, map_location="cpu")
    return _fp32(blob["state_dict"] if isinstance(blob, dict) and "state_dict" in blob else blob)


def load_weights(run_dir: str, shape: Cfg, source: Optional[str] = None) -> Tuple["OrderedDict[str, torch.Tensor]", str]:
    """(fp32 state dict on the CPU, 'container' | 'pth').  The container is preferred when the run has one."""
    from .pipeline import entropy_coding
    if is_feather(shape):
        from .pipeline.feathermap.feathernet import DEPLOY_UNSUPPORTED
        raise NotImplementedError("a masking=Feathermap run saves no deployable weights (model.pth holds the feather vector, not "
                                  f"the network): {DEPLOY_UNSUPPORTED}")
    qdir = os.path.join(run_dir, "model_quantized")
    have_q = os.path.exists(os.path.join(qdir, "meta_data.json")) and os.path.exists(os.path.join(qdir, "compressed_weights.data"))
    pth = os.path.join(run_dir, "model.pth")
    _check_source(source)
    if source == "container" and not have_q:
        raise FileNotFoundError(f"decode.source=container: {qdir} holds no compressed_weights.data / meta_data.json")
    if source == "pth" and not os.path.exists(pth):
        raise FileNotFoundError(f"decode.source=pth: {pth} not found")
    if source == "container" or (not source and have_q):
        ec = dict(shape.get("entropy_coding") or {})
        sd, used = _fp32(entropy_coding.decompress_state_dict(qdir, stream_name=ec.pop("stream_name", "plain"), **ec)), "container"
    elif os.path.exists(pth):
        sd, used = read_pth(pth), "pth"
    else:
        raise FileNotFoundError(f"{run_dir} holds neither model_quantized/ nor model.pth")
    want = shape.get("state_dict_keys")
    if want:   # the dense names the fit recorded (a quantised copy adds centroids / labeled_weight, which come back as weight)
        dense = [k for k in want if "centroids" not in k and "labeled_weight" not in k]
        if sorted(dense) != sorted(sd.keys()):
            raise ValueError(f"{used}: tensors {sorted(sd.keys())} do not match the fit's state dict {sorted(dense)}")
    return sd, used


# ---- Feathermap: the feather vector of model.pth -------------------------------------------------------------
def is_feather(shape: Cfg) -> bool:
    return shape.get("masking_name") == "Feathermap"


def feather_keys(depth: int) -> List[str]:
    """the state-dict keys of a FeatherNet over a SIREN of `depth` layers, in named_parameters() order"""
    return ["_V1", "_V2"] + [f"module.layers.{l}.linear.{kind}_p" for l in range(depth) for kind in ("weight", "bias")]


def load_feather(run_dir: str, shape: Cfg, source: Optional[str] = None) -> "OrderedDict[str, torch.Tensor]":
    """The fp32 CPU state dict of a masking=Feathermap run's model.pth: _V1 [n, m], _V2 [m, n] and one scalar per weight /
    bias tensor, checked against decode.json's key list and against the network of `shape` (n = ceil(sqrt(P))).  A tensor
    that is missing or of another shape raises a ValueError that names it."""
    _check_source(source)
    if source == "container":
        raise FileNotFoundError("decode.source=container: a masking=Feathermap run has no container (fit writes model.pth, the "
                                "feather vector in fp32, and nothing under model_quantized/)")
    pth = os.path.join(run_dir, "model.pth")
    if not os.path.exists(pth):
        raise FileNotFoundError(f"{pth} not found (a masking=Feathermap run is decoded from model.pth)")
    sd = read_pth(pth)
    for k in feather_keys(int(shape.mlp.depth)):
        if k not in sd:
            raise ValueError(f"pth: the feather vector has no tensor {k}")
    want = shape.get("state_dict_keys")
    if want and sorted(want) != sorted(sd.keys()):
        raise ValueError(f"pth: tensors {sorted(sd.keys())} do not match the fit's state dict {sorted(want)}")
    for k in feather_keys(int(shape.mlp.depth))[2:]:
        if sd[k].numel() != 1:
            raise ValueError(f"pth: {k} has shape {tuple(sd[k].shape)}, a scalar was expected")
    feather_geometry(shape, sd)
    return sd


def feather_geometry(shape: Cfg, sd) -> Tuple[int, int, List[int], List[int]]:
    """(n, m, logical_out, logical_in) as sf_feather_render_attach takes them, from a shape alone (no model yet): V1 is
    [n, m], V2 [m, n], and n must be ceil(sqrt(P)) for the P weights and biases of the SIREN of `shape`
    (feathernet.py:186); else a ValueError naming the tensor"""
    mlp = shape.mlp
    outs, ins = layer_sizes(int(mlp.get("input_size", 2)), engine_width(shape), int(mlp.depth), int(mlp.get("output_size", 3)))
    P = sum(o * i + o for o, i in zip(outs, ins))
    n = math.isqrt(P - 1) + 1                      # ceil(sqrt(P)), in integers
    v1, v2 = tuple(sd["_V1"].shape), tuple(sd["_V2"].shape)
    if len(v1) != 2 or v1[0] != n or not 1 <= v1[1] <= n:
        raise ValueError(f"_V1 has shape {v1}: the network of decode.json has {P} weights and biases, so V1 is [{n}, m] with "
                         f"1 <= m <= {n}")
    m = v1[1]
    if v2 != (m, n):
        raise ValueError(f"_V2 has shape {v2}, [{m}, {n}] was expected (the transpose of _V1's {v1})")
    return n, m, outs, ins


def feather_flat(sd, depth: int) -> torch.Tensor:
    """[V1 | V2 | scalers]: the feather vector in FeatherNet.named_parameters() order, flat fp32"""
    return torch.cat([sd[k].reshape(-1) for k in feather_keys(depth)]).float().contiguous()


def feather_model(sd, shape: Cfg):
    """the FeatherNet of `shape` with `sd` loaded, on the CPU: the registry SIREN under compress = (2 m - 1) / n, which
    ceil(compress * n / 2) turns back into m"""
    from .pipeline.feathermap import FeatherNet
    n, m, _, _ = feather_geometry(shape, sd)
    with torch.random.fork_rng(devices=[]):       # the constructors draw an initialisation nobody needs
        net = FeatherNet(registry["siren"](**dict(shape.mlp), **dict(shape.get("engine") or {})), compress=(2 * m - 1) / n)
    assert (net._size_n, net._size_m) == (n, m), ((net._size_n, net._size_m), (n, m))
    net.load_state_dict(sd)
    return net


# ---- bytes ------------------------------------------------------------------------------------------------
def to_u8(pred: torch.Tensor) -> torch.Tensor:
    """min(max(trunc(pred * 255), 0), 255) as uint8: eval_epoch's (pred * 255).int(), clamped to what a file can hold.
    (the product in fp32; the float clamp to [-1, 256] only keeps huge values inside int32 and changes no result)"""
    return (pred.float() * 255).clamp(-1, 256).int().clamp(0, 255).to(torch.uint8)


def to_u16(pred: torch.Tensor) -> torch.Tensor:
    """min(max(trunc(pred * 65535), 0), 65535) as int32: to_u8's statement at 16 bits per sample, the inverse of the loader's
    raw / (2^16 - 1).  (the product in fp32; the float clamp to [-1, 65536] only keeps huge values inside int32 and changes
    no result)"""
    return (pred.float() * 65535).clamp(-1, 65536).int().clamp(0, 65535)


def sample_bits(dec: Dict[str, str]) -> int:
    """decode.bits of the decode.* keys: 8 (default) | 16"""
    raw = dec.get("bits") or "8"
    if raw not in [str(b) for b in SAMPLE_BITS]:
        raise ValueError(f"decode.bits must be one of {', '.join(str(b) for b in SAMPLE_BITS)}, got {raw!r}")
    return int(raw)


def plan_bands(height: int, width: int, channels: int = 3, band_rows: Optional[int] = None,
               band_bytes: int = BAND_BYTES, sample_bytes: int = 1) -> List[Tuple[int, int]]:
    """Row bands [r0, r1) that cover [0, height): each satisfies rows * width^2 < 2^40 (the engine's row decode) and
    rows * width * channels * sample_bytes < band_bytes; band_rows lowers the size further."""
    if height < 1 or width < 1:
        raise ValueError("bad picture size")
    cap = min((ROW_LIMIT - 1) // (width * width), (band_bytes - 1) // (width * channels * sample_bytes))
    if cap < 1:
        raise ValueError(f"width {width}: one row does not fit a band")
    rows = min(height, cap if not band_rows else max(1, min(cap, int(band_rows))))
    return [(r, min(r + rows, height)) for r in range(0, height, rows)]


def _span(spec: Optional[str], n: int, what: str) -> Tuple[int, int]:
    if not spec:
        return 0, n
    a, _, b = spec.partition(":")
    lo, hi = (int(a) if a else 0), (int(b) if b else n)
    if not (0 <= lo < hi <= n):
        raise ValueError(f"decode.{what}={spec}: need 0 <= a < b <= {n}")
    return lo, hi


# ---- the families and the two paths ------------------------------------------------------------------------
def engine_width(shape: Cfg) -> int:
    return int(shape.mlp.hidden_size * math.sqrt(shape.get("small_dense_density") or 1.0))   # siren.py:88


def padded_width(shape: Cfg) -> Optional[int]:
    """the width the engine runs the network at: the logical width, or the next kernel width when it zero-pads (the
    models' own rule, Siren._engine_width); None above 1024"""
    return next_kernel_width(engine_width(shape), Siren.WIDTHS)


class Family(NamedTuple):
    """what `decode` needs to know of a model family; `family` is the one place that tells them apart"""
    available: Callable          # (shape, H, W) -> (is there a render kernel for this model and picture, why)
    auto_kernel: bool            # decode.render=auto runs the kernel when there is one
    load: Callable               # (run_dir, shape, decode.source) -> (fp32 CPU state dict, 'container' | 'pth')
    model: Callable              # (state dict, shape) -> the CPU model, which also builds and fills the render handle
    windowed: bool = False       # a band is a pixel window of an even, square picture, not a slice of coordinate vectors


def _narrow(shape: Cfg) -> Tuple[int, Optional[int], str]:
    """(logical width, the kernel width it renders at or None, the note a why string carries when the two differ)"""
    w, wp = engine_width(shape), padded_width(shape)
    return w, (wp if wp in KERNEL_WIDTHS else None), ("" if wp == w else f" (width {w} zero-padded)")


def _siren_kernel(shape: Cfg, H: int, W: int, what: str = "SIREN", entry: str = "sf_render") -> Tuple[bool, str]:
    w, wp, pad = _narrow(shape)
    if wp is None:
        return False, f"SIREN width {w} is on the wide path: no render kernel"
    return True, f"{what} {wp}x{shape.mlp.depth}{pad}: {entry}"


def _wavelet_kernel(shape: Cfg, H: int, W: int) -> Tuple[bool, str]:
    w, wp, pad = _narrow(shape)
    if wp is None:
        return False, f"WaveletSiren width {w} is above 256: no render kernel"
    if H != W or H < 2 or H % 2:
        return False, f"WaveletSiren needs an even, square picture (got {H}x{W}): no render kernel"
    return True, f"WaveletSiren {wp}x{shape.mlp.depth}{pad}: sf_wavelet_render"


def _fourier_kernel(shape: Cfg, H: int, W: int) -> Tuple[bool, str]:
    m, (w, wp, pad) = shape.mlp, _narrow(shape)
    n_linear, ms = int(m.get("depth", 8)) - 1, int(m.get("map_size", 128))
    fin, fout = m.get("input_size", 2), m.get("output_size", 3)
    if wp is None:
        return False, f"FourierNet width {w} is above 256: no render kernel"
    if not fourier_engine_takes(int(fin), int(fout), ms, n_linear):         # FourierNet's own constructor rule
        return False, (f"FourierNet with map_size {ms}, {n_linear} Linear layers, input_size {fin}, output_size {fout}: the "
                       f"engine takes map_size {' / '.join(map(str, FOURIER_MAPS))}, 2..12 layers, 2 -> 3")
    return True, f"FourierNet {wp}x{n_linear} map {ms}{pad}: sf_render"


def family(shape: Cfg) -> Family:
    """siren, feather (SIREN under masking=Feathermap), fourier or wavelet_siren; any other mlp.name fails at the registry"""
    name = shape.mlp.get("name", "siren")
    if name == "siren" and is_feather(shape):     # model.pth holds the feather vector, not the network
        return Family(lambda *a: _siren_kernel(*a, "Feathermap", "sf_feather_render_load + sf_render"), True,
                      lambda *a: (load_feather(*a), "pth"), feather_model)
    return {"siren": Family(_siren_kernel, True, load_weights, registry_model),
            "fourier": Family(_fourier_kernel, False, load_weights, registry_model),
            "wavelet_siren": Family(_wavelet_kernel, True, load_weights, registry_model, windowed=True),
            }.get(name, Family(lambda *a: (False, f"mlp={name} has no render kernel"), False, load_weights, registry_model))


def kernel_available(shape: Cfg, height: Optional[int] = None, width: Optional[int] = None) -> Tuple[bool, str]:
    """(is there a render kernel for this model and picture, why): what decode.render=kernel asks.  height / width: the
    picture to draw (default: the fitted size), which matters to WaveletSiren only.  No device is touched."""
    img = shape.get("img") or {}
    return family(shape).available(shape, int(height or img.get("height") or 0), int(width or img.get("width") or 0))


def render_path(shape: Cfg, height: Optional[int] = None, width: Optional[int] = None) -> Tuple[str, str]:
    """('kernel' | 'torch', why) of decode.render=auto: the kernel when there is one, unless the family's default has not moved"""
    if not family(shape).auto_kernel:
        return "torch", f"mlp={shape.mlp.get('name', 'siren')} has no render kernel"
    ok, why = kernel_available(shape, height, width)
    return ("kernel" if ok else "torch"), why


def wide_available(shape: Cfg) -> Tuple[bool, str]:
    """(does decode.render=wide draw this model, why / what draws it instead): a plain SIREN whose engine width is 512 or
    1024 with depth >= 3, on the wide render handle.  No device is touched."""
    name = shape.mlp.get("name", "siren")
    if name != "siren" or is_feather(shape):
        what = "Feathermap" if name == "siren" else {"fourier": "FourierNet", "wavelet_siren": "WaveletSiren"}.get(name, f"mlp={name}")
        return False, f"the wide render is SIREN only ({what} decodes under decode.render=auto, kernel or torch)"
    w, wp = engine_width(shape), padded_width(shape)
    if wp in KERNEL_WIDTHS:
        return False, f"SIREN width {w} has the render kernel of the narrow path: use decode.render=kernel"
    if wp not in WIDE_WIDTHS:
        return False, f"SIREN width {w} is above 1024: no engine runs it"
    if int(shape.mlp.depth) < 3:
        return False, f"SIREN width {w} needs depth >= 3 on the wide path (got {shape.mlp.depth})"
    return True, f"SIREN {wp}x{shape.mlp.depth}{'' if wp == w else f' (width {w} zero-padded)'}: sf_wide_render"


def render_mode(dec: Dict[str, str]) -> str:
    """decode.render of the decode.* keys: auto (default) | kernel | wide | torch"""
    mode = dec.get("render") or "auto"
    if mode not in RENDER_MODES:
        raise ValueError(f"decode.render must be one of {', '.join(RENDER_MODES)}, got {mode!r}")
    return mode


def choose_path(shape: Cfg, mode: str, height: int, width: int) -> Tuple[str, str]:
    """('kernel' | 'torch', why) for a decode.render mode; kernel without a render kernel, and wide for anything but a plain
    SIREN of engine width 512 / 1024, raise ValueError"""
    if mode == "torch":
        return "torch", "decode.render=torch"
    if mode == "wide":
        ok, why = wide_available(shape)
        if not ok:
            raise ValueError(f"decode.render=wide: {why}")
        return "kernel", why
    if mode == "auto":
        return render_path(shape, height, width)
    ok, why = kernel_available(shape, height, width)
    if not ok:
        raise ValueError(f"decode.render=kernel: {why}")
    return "kernel", why


def registry_model(sd, shape: Cfg):
    """the registry model of `shape` with `sd` loaded, on the CPU (names, shapes and the padding rule; no engine yet)"""
    m = dict(shape.mlp)
    with torch.random.fork_rng(devices=[]):       # the constructor draws an initialisation nobody needs
        model = registry[m.get("name", "siren")](**m, small_dense_density=shape.get("small_dense_density") or 1.0,
                                                 **dict(shape.get("engine") or {}))
    model.load_state_dict(sd)
    return model


def engine_flat_params(sd, shape: Cfg, num_params: int) -> torch.Tensor:
    """what the model of `shape` hands a handle with num_params slots (zeros in the padding of a wider engine), on the CPU"""
    return registry_model(sd, shape)._flat_for(num_params, torch.device("cpu"))


def flat_params(sd: Dict[str, torch.Tensor], depth: int) -> torch.Tensor:
    """a SIREN state dict in the engine's flat order, by its key names alone"""
    keys = [f"layers.{l}.linear.{kind}" for l in range(depth) for kind in ("weight", "bias")]
    return torch.cat([sd[k].reshape(-1) for k in keys]).float().contiguous()


# ---- the kernel path --------------------------------------------------------------------------------------
def _render(sd, shape: Cfg, rows, cols, band_rows: Optional[int], want_pred: bool, device: int, bits: int,
            side: Optional[int] = None):
    """The whole kernel job of the four renderers: build the CPU model, plan the bands, open ONE render handle through the
    model (sized for the first band), let the model fill it, draw band by band, copy each band to the CPU as it comes, and
    close the handle whatever happens.  rows / cols: the coordinate vectors of the grid; with `side` (a windowed family)
    the pixel spans (a, b) of its side x side picture.  uint8 (bits = 16: int32 values 0..65535, widened from the kernel's
    uint16) [rows, cols, C] on the CPU (and the fp32 prediction when asked)."""
    model = family(shape).model(sd, shape)
    n_cols = cols.numel() if side is None else cols[1] - cols[0]
    bands = (plan_bands(rows.numel(), n_cols, model.cfg["output_size"], band_rows, sample_bytes=bits // 8) if side is None
             else plan_wavelet_bands(side, rows, cols, band_rows, sample_bytes=bits // 8))
    row0, nb = bands[0][0], bands[0][1] - bands[0][0]
    eng = model._new_render_engine(nb, n_cols, device, side)
    cols_d = cols.float().contiguous().to(eng.device) if side is None else None

    def draw(a, b):
        if side is not None:                       # a window of the picture, over the coefficients its rows need
            return eng.render(a, b, cols[0], cols[1], want_u8=True, want_pred=want_pred, bits=bits)
        rb = rows[a:b].float()                     # a slice of `rows`; a shorter (last) band is padded with its final row
        if b - a < nb:
            rb = torch.cat([rb, rb[-1:].expand(nb - (b - a))])
        eng.set_coords(rb.contiguous().to(eng.device), cols_d)
        u8, p = eng.render(want_u8=True, want_pred=want_pred, bits=bits)
        return u8[:b - a], (p[:b - a] if want_pred else None)      # and cut after the render

    try:
        model._load_render_engine(eng)
        size = (bands[-1][1] - row0, n_cols, eng.out_features)
        out = torch.empty(size, dtype=torch.int32 if bits == 16 else torch.uint8)
        pred = torch.empty(size) if want_pred else None
        for a, b in bands:
            u8, p = draw(a, b)
            out[a - row0:b - row0] = u8.cpu().to(out.dtype)
            if want_pred:
                pred[a - row0:b - row0] = p.cpu()
    finally:
        eng.close()
    return out, pred


def render_kernel(sd, shape: Cfg, rows: torch.Tensor, cols: torch.Tensor, band_rows: Optional[int] = None,
                  want_pred: bool = False, device: int = 0, bits: int = 8):
    """uint8 [h, w, C] on the CPU (and the fp32 prediction when asked) of the grid rows x cols, band by band on ONE render
    handle of the family of `shape` (plan_bands is stricter than the height * width < 2^31 a handle needs); bits: _render"""
    return _render(sd, shape, rows, cols, band_rows, want_pred, device, bits)


# (a Feathermap run, sd as load_feather returns it, and mlp=fourier under their own names: `shape` tells, not the caller)
render_feather = render_fourier = render_kernel


# ---- WaveletSiren: which coefficients a window needs, bands, the kernel path -----------------------------------
def _wv_tap(o, H: int):
    """(i0, i1) of wv_tap (csrc/wavelet_kernels.hip) for output index o (int or array), its fp32 arithmetic operation for
    operation"""
    import numpy as np
    n = (H + 5) // 2
    up = np.float32(1.0 / (float(H) / float(n)))
    s = up * (np.asarray(o).astype(np.float32) + np.float32(0.5)) - np.float32(0.5)
    s = np.where(s < 0, np.float32(0), s).astype(np.float32)
    i0 = s.astype(np.int64)
    return i0, i0 + (i0 < n - 1)


def wavelet_coeff_span(o0: int, o1: int, H: int) -> Tuple[int, int]:
    """Coefficient rows (or columns) [lo, hi) that output rows [o0, o1) of an H-row WaveletSiren picture read: for Y rows
    o/2 .. o/2 + 2 (the inverse DWT's gather), for Cb / Cr the two bilinear source rows.  All are monotone in o, so the
    span is the minimum at o0 and the maximum at o1 - 1 (the library's wv_coeff_span, csrc/wavelet_render.hip)."""
    if not (0 <= o0 < o1 <= H) or H < 2 or H % 2:
        raise ValueError(f"need 0 <= o0 < o1 <= H, H even (got [{o0}, {o1}) of {H})")
    a0, _ = _wv_tap(o0, H)
    _, b1 = _wv_tap(o1 - 1, H)
    return min(o0 // 2, int(a0)), max((o1 - 1) // 2 + 2, int(b1)) + 1


def plan_wavelet_bands(H: int, r: Tuple[int, int], c: Tuple[int, int], band_rows: Optional[int] = None,
                       band_bytes: int = BAND_BYTES, sample_bytes: int = 1) -> List[Tuple[int, int]]:
    """Bands [r0, r1) of pixel rows that cover r = [ra, rb): each keeps rows * cols * 3 * sample_bytes < band_bytes and its coefficient
    window within the render sub-handles' row decode, cr * cc^2 < 2^40 (cc: the coefficient columns of the column window
    c); band_rows lowers the size further."""
    cols = c[1] - c[0]
    j0, j1 = wavelet_coeff_span(c[0], c[1], H)
    cc = j1 - j0
    cr_cap = (ROW_LIMIT - 1) // (cc * cc)
    cap = (band_bytes - 1) // (cols * 3 * sample_bytes)
    if cap < 1 or cr_cap < 4:
        raise ValueError(f"{cols} columns: one row does not fit a band")
    cap = min(cap, 2 * (cr_cap - 3))              # rows pixel rows read at most rows / 2 + 3 coefficient rows
    rows = min(r[1] - r[0], cap if not band_rows else max(1, min(cap, int(band_rows))))
    bands = [(a, min(a + rows, r[1])) for a in range(r[0], r[1], rows)]
    for a, b in bands:
        i0, i1 = wavelet_coeff_span(a, b, H)
        assert (i1 - i0) * cc * cc < ROW_LIMIT
    return bands


def render_wavelet(sd, shape: Cfg, H: int, r: Tuple[int, int], c: Tuple[int, int], band_rows: Optional[int] = None,
                   want_pred: bool = False, device: int = 0, bits: int = 8):
    """render_kernel for the window r x c of the H x H picture of a WaveletSiren, on ONE render handle (max_rows = the band
    height, max_cols = the window's): every band runs the two sub-networks over the coefficient window it needs, no more"""
    return _render(sd, shape, r, c, band_rows, want_pred, device, bits, side=H)


def render_torch(sd, shape: Cfg, height: int, width: int, r: Tuple[int, int], c: Tuple[int, int], device: int = 0,
                 bits: int = 8):
    """the family's CPU model, moved to the device: its own forward on the full height x width grid, cut to the window,
    bytes by to_u8 (bits=16: int32 values 0..65535 by to_u16)"""
    dev = torch.device("cuda", device)
    model = family(shape).model(sd, shape).to(dev).eval()
    with torch.no_grad():
        pred = model(get_grid(height, width).to(dev))
    pred = pred[r[0]:r[1], c[0]:c[1]].contiguous()
    return (to_u16 if bits == 16 else to_u8)(pred).cpu(), pred.cpu()


def metrics(pred: torch.Tensor, u8: torch.Tensor, img: torch.Tensor, u16: Optional[torch.Tensor] = None) -> Dict[str, float]:
    """eval_epoch's figures (train_helper.py:41-59) for a prediction and the bytes written for it; with the 16-bit samples
    written for it also PSNR_16bit, the same formula on 65535 levels (the squared differences in int64: 65535^2 does not
    fit int32)"""
    loss = float(((pred.double() - img.double()) ** 2).sum().item() / img.numel())
    mse8 = (((img * 255).int() - u8.int()) ** 2).float().mean()
    res = {"loss": loss, "PSNR": 10 * math.log10(1 / loss), "PSNR_8bit": (10 * torch.log10(255 ** 2 / mse8)).item()}
    if u16 is not None:
        mse16 = (((img * 65535).int().long() - u16.long()) ** 2).double().mean().item()
        res["PSNR_16bit"] = 10 * math.log10(65535 ** 2 / mse16) if mse16 > 0 else math.inf
    return res


def load_truth(spec: str, height: int, width: int) -> torch.Tensor:
    if spec.startswith("synthetic"):
        return load_img(spec, height=height, width=width)
    raw = read_ppm(spec)
    maxval = 65535 if int(raw.max()) > 255 else 255
    return (raw.double() / maxval).float()


def decode(argv: Sequence[str]) -> Dict[str, object]:
    dec, rest = split_overrides(argv)
    mode = render_mode(dec)
    bits = sample_bits(dec)
    run_dir = dec.get("dir")
    if not run_dir:
        raise ValueError("decode.dir=<run directory written by fit> is required")
    shape = resolve_shape(run_dir, rest)
    H = int(dec.get("height") or shape.img.get("height") or 0)
    W = int(dec.get("width") or shape.img.get("width") or 0)
    fam = family(shape)
    if mode in ("kernel", "wide"):                 # no render kernel: refused before a file is read or the device touched
        choose_path(shape, mode, H, W)
    sd, source = fam.load(run_dir, shape, dec.get("source"))
    if H < 1 or W < 1:
        raise ValueError("output size unknown: pass decode.height=... decode.width=... (or img.height / img.width)")
    r, c = _span(dec.get("rows"), H, "rows"), _span(dec.get("cols"), W, "cols")
    device, truth = int(dec.get("device") or 0), dec.get("truth")
    if fam.windowed:
        check_image(H, W)                          # the "even, square" refusal, before anything touches the device
    path, why = choose_path(shape, mode, H, W)
    logging.info(f"decode: weights from {source}; {path} path ({why}); {r[1] - r[0]}x{c[1] - c[0]} of a {H}x{W} grid")
    if path == "kernel":
        band_rows = int(dec["band_rows"]) if dec.get("band_rows") else None
        rows, cols = (r, c) if fam.windowed else (torch.linspace(0, 1, H)[r[0]:r[1]], torch.linspace(0, 1, W)[c[0]:c[1]])
        u8, pred = _render(sd, shape, rows, cols, band_rows, bool(truth), device, bits, side=H if fam.windowed else None)
    else:
        u8, pred = render_torch(sd, shape, H, W, r, c, device=device, bits=bits)
    if u8.shape[-1] != 3:
        raise NotImplementedError(f"PPM holds 3 channels, the model has {u8.shape[-1]}")
    out = dec.get("out") or os.path.join(run_dir, "decoded.ppm")
    (write_ppm16 if bits == 16 else write_ppm)(out, u8)   # (bits = 16: u8 holds the 16-bit samples)
    res = {"out": out, "path": path, "why": why, "source": source, "height": int(u8.shape[0]), "width": int(u8.shape[1])}
    if truth:
        img = load_truth(truth, H, W)[r[0]:r[1], c[0]:c[1]]
        res.update(metrics(pred, to_u8(pred), img, u8) if bits == 16 else metrics(pred, u8, img))
        keys = ("loss", "PSNR", "PSNR_8bit") + (("PSNR_16bit",) if bits == 16 else ())
        logging.info("Decode | " + " | ".join(f"{k}: {res[k]:.4f}" for k in keys))
        print(json.dumps({k: res[k] for k in keys}))
    logging.info(f"decode: wrote {out}")
    return res


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s] %(message)s")
    return decode(list(sys.argv[1:] if argv is None else argv))


if __name__ == "__main__":
    main()
