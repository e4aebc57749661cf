"""SIREN model with the reference's constructor, parameter names and call signature
(reference: implicit_image/models/siren.py:9-134), executed by the gfx950 engine.

The torch module only OWNS NAMES AND SHAPES: once bound (models/binding.py), every
`layers.{i}.linear.{weight,bias}` Parameter (and its .grad) is a zero-copy view of the engine's flat fp32 state.
forward() runs the fused HIP kernels; there is no PyTorch arithmetic fallback.
"""
from typing import Optional

import numpy as np
import torch
from torch import nn

from .binding import EngineBound

KERNEL_WIDTHS = (32, 64, 128, 256)     # fused chain kernels: the widths with a render kernel; all FourierNet / WaveletSiren run


def next_kernel_width(hidden: int, widths) -> Optional[int]:
    """The width the engine runs a network of logical width `hidden` at: the narrowest of `widths` (ascending: the widths
    the kernels are instantiated for) that holds it, None above the last.  The one statement of the zero-padding rule:
    Siren, FourierNet and decode.padded_width call it, each with its own widths."""
    return next((w for w in widths if w >= hidden), None)


def layer_sizes(input_size: int, hidden: int, depth: int, output_size: int):
    """(logical_out, logical_in) of every Linear of a SIREN, for Siren, FeatherNet and decode (from a shape, before a model)"""
    fans = [input_size] + [hidden] * (depth - 1) + [output_size]
    return fans[1:], fans[:-1]


class SineLayer(nn.Module):
    """Linear -> sin(omega_0 * z) (reference siren.py:9-68).  Holds the nn.Linear so that
    `isinstance(m, nn.Linear)` scans (masking, k-means, entropy coding) find it under `.linear`."""

    def __init__(self, in_features: int, out_features: int, has_bias: bool = True, is_first: bool = False,
                 omega_0: float = 30.0, no_activation: bool = False):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.is_first, self.omega_0, self.no_activation = is_first, omega_0, no_activation
        # nn.Linear's default init draws (weight, then bias) come first, as in the reference, so the
        # generator state and the bias values match a reference model built from the same seed
        self.linear = nn.Linear(in_features, out_features, bias=has_bias)
        bound = 1 / in_features if is_first else np.sqrt(6 / in_features) / omega_0
        with torch.no_grad():
            self.linear.weight.uniform_(-bound, bound)
        self.linear.scaler = bound

    def forward(self, x):  # pragma: no cover - the layers never run individually
        raise RuntimeError("SineLayer is executed by the fused engine; call Siren.forward(grid)")


class Siren(EngineBound):
    # hidden widths the kernels are instantiated for (<= 256: fused chain kernels; 512 / 1024: layer-at-a-time
    # kernels); any other width (e.g. Small_Dense's int(hidden * sqrt(density)), reference siren.py:88) runs
    # zero-padded to the next one: padded neurons have zero weights and bias and feed zero weights, so the prediction and
    # every logical gradient are those of the narrow network.  With 16-bit phases they output sin(0) = 0 and their slots
    # stay zero; with phase bytes (formats 8 / 12, what auto picks for a dense fit) a phase decodes to u / 256 + kPhaseEps
    # revolutions (siren_kernels.hip), a padded neuron outputs sin(2 pi / 65536), the weights it feeds get a small gradient
    # and Adam moves those slots of the ENGINE's vector.  Nothing accumulates: the logical parameters are scattered into a
    # zeroed vector before every pass (EngineBound._sync_to_engine) and only logical slots are gathered back
    WIDTHS = KERNEL_WIDTHS + (512, 1024)

    def __init__(self, input_size: int = 2, output_size: int = 3, depth: int = 8, hidden_size: int = 128,
                 first_omega_0: float = 50.0, hidden_omega_0: float = 50.0, outermost_linear: bool = True,
                 simulate_quantization: bool = False, small_dense_density: float = 1.0,
                 compute_dtype: str = "f16", chunk_pixels: int = 0, scratch_format: int = 0, **kwargs):
        super().__init__()
        if simulate_quantization:
            raise NotImplementedError("simulate_quantization (QAT stubs) is outside the accelerated path")
        hidden_size = int(hidden_size * np.sqrt(small_dense_density))   # Small_Dense (reference siren.py:88)
        layers = [SineLayer(input_size, hidden_size, is_first=True, omega_0=first_omega_0)]
        for _ in range(depth - 2):
            layers.append(SineLayer(hidden_size, hidden_size, omega_0=hidden_omega_0))
        layers.append(SineLayer(hidden_size, output_size, omega_0=hidden_omega_0, no_activation=outermost_linear))
        self.layers = nn.Sequential(*layers)
        self.simulate_quantization = simulate_quantization
        self.cfg = dict(input_size=input_size, output_size=output_size, depth=depth, hidden_size=hidden_size,
                        first_omega_0=float(first_omega_0), hidden_omega_0=float(hidden_omega_0),
                        outermost_linear=bool(outermost_linear), compute_dtype=compute_dtype,
                        chunk_pixels=chunk_pixels, scratch_format=int(scratch_format))
        self._engine_width = next_kernel_width(hidden_size, self.WIDTHS)
        if self._engine_width is None:
            raise NotImplementedError(f"hidden_size {hidden_size} > 1024 is not supported by the gfx950 engine")
        if self._engine_width > 256 and depth < 3:
            raise NotImplementedError("hidden_size > 256 needs depth >= 3")
        self._padded = self._engine_width != hidden_size

    def _param_list(self):
        """The engine's parameters in flat order: (weight, bias) of every layer.  Not `self.parameters()`:
        k-means conversion registers extra (frozen) `centroids` / `labeled_weight` parameters on the Linears."""
        out = []
        for layer in self.layers:
            out += [layer.linear.weight, layer.linear.bias]
        return out

    def _handle(self, cls, H: int, w: int, device: int, **more):
        """a handle of class `cls` for H x w pixels: the one mapping from `cfg`, whatever the handle is for"""
        c = self.cfg
        return cls(H, w, hidden=self._engine_width, depth=c["depth"], first_omega_0=c["first_omega_0"],
                   hidden_omega_0=c["hidden_omega_0"], outermost_linear=c["outermost_linear"], out_features=c["output_size"],
                   compute_dtype=c["compute_dtype"], device=device, chunk_pixels=c["chunk_pixels"], **more)

    def _new_engine(self, H: int, w: int, row_begin: int, row_end: int, device: int):
        from .._engine import SirenEngine
        return self._handle(SirenEngine, H, w, device, row_begin=row_begin, row_end=row_end, betas=self._adam[0],
                            eps=self._adam[1], scratch_format=self.cfg["scratch_format"])

    def _new_render_engine(self, rows: int, cols: int, device: int, side=None):
        """the render handle of this model's engine width: the fused chain kernels up to 256, the layer-at-a-time ones above"""
        from .._engine import RenderEngine, WideRenderEngine
        return self._handle(WideRenderEngine if self._engine_width > 256 else RenderEngine, rows, cols, device)

    def _layer_fans(self):
        c = self.cfg
        outs, ins = layer_sizes(c["input_size"], c["hidden_size"], c["depth"], c["output_size"])
        return [(ins[l], outs[l], l > 0, l < c["depth"] - 1) for l in range(c["depth"])]
