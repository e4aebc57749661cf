"""FourierNet with the reference's constructor, parameter names, state_dict keys and random-draw order
(reference: implicit_image/models/fourier.py:8-72), executed by the gfx950 engine (csrc/fourier_kernels.hip).

`encoding.B` is a frozen Parameter handed to the engine once per bind; every `layers.{2k}.{weight,bias}`
(the nn.Linear layers of the Sequential) is, once bound, a zero-copy view of the engine's flat fp32 state,
as in `Siren` (models/binding.py).  forward() runs the fused HIP kernels; there is no PyTorch arithmetic fallback.
"""
import numpy as np
import torch
from torch import nn

from .binding import EngineBound
from .siren import KERNEL_WIDTHS, next_kernel_width

# the reference's Masking puts the frozen encoding.B into its mask_dict and its first update_connections() fails on
# B.grad being None (reference pipeline/masking/funcs/grow.py:87): there is no reference behaviour to reproduce
MASKING_UNSUPPORTED = ("mask-based sparsity (RigL / SNFS / SET / Pruning) is not supported on FourierNet: the reference's "
                       "Masking registers the frozen encoding.B and its first update_connections() fails with "
                       "AttributeError ('NoneType' object has no attribute 'dtype', pipeline/masking/funcs/grow.py:87). "
                       "Use masking=none or masking=Small_Dense")
PIXEL_SPLIT_UNSUPPORTED = "pixel-split (row ranges) is not supported for FourierNet"
MAP_SIZES = (64, 128, 256, 512)   # the encoding sizes k_ff_fwd is instantiated for


def engine_takes(input_size: int, output_size: int, map_size: int, n_linear: int) -> bool:
    """what the engine accepts besides the width: the constructor and decode's availability rule both ask here"""
    return input_size == 2 and output_size == 3 and map_size in MAP_SIZES and 2 <= n_linear <= 12


class Encoding(nn.Module):
    """[sin(2 pi x B), cos(2 pi x B)] (reference fourier.py:8-24); evaluated inside the engine's forward kernel."""

    def __init__(self, input_size: int = 2, map_size: int = 256, map_scale: float = 10.0):
        super().__init__()
        assert map_size % 2 == 0, "Need even map size"
        self.B = nn.Parameter(torch.randn(input_size, map_size // 2) * map_scale, requires_grad=False)

    def forward(self, x):  # pragma: no cover - the encoding never runs on its own
        raise RuntimeError("Encoding is evaluated by the fused engine; call FourierNet.forward(grid)")


class FourierNet(EngineBound):
    # engine widths: Small_Dense's int(hidden * sqrt(density)) runs zero-padded to the next one (padded neurons have zero
    # weights and bias, output relu(0) = 0 and receive exactly zero gradients)
    WIDTHS = KERNEL_WIDTHS
    mask_unsupported = MASKING_UNSUPPORTED
    split_unsupported = PIXEL_SPLIT_UNSUPPORTED
    _WHO = "Siren"                 # (the wording a CPU grid has always been refused with)

    def __init__(self, input_size: int = 2, output_size: int = 3, depth: int = 8, hidden_size: int = 128,
                 map_size: int = 128, map_scale: float = 10.0, small_dense_density: float = 1.0,
                 compute_dtype: str = "f16", chunk_pixels: int = 0, **kwargs):
        super().__init__()
        if compute_dtype != "f16":
            raise NotImplementedError("FourierNet runs fp16 MFMA operands only (engine.compute_dtype=f16)")
        hidden_size = int(hidden_size * np.sqrt(small_dense_density))   # Small_Dense (reference fourier.py:40)
        # the nn.Linear default inits run first, in layer order; the encoding's randn comes after them
        layers = [nn.Linear(map_size, hidden_size), nn.ReLU(inplace=True)]
        for _ in range(depth - 3):
            layers += [nn.Linear(hidden_size, hidden_size), nn.ReLU(inplace=True)]
        layers += [nn.Linear(hidden_size, output_size), nn.Sigmoid()]
        self.encoding = Encoding(input_size, map_size, map_scale)        # registered before `layers` (state_dict order)
        self.layers = nn.Sequential(*layers)
        self.simulate_quantization = False
        n_linear = len(layers) // 2
        self.cfg = dict(input_size=input_size, output_size=output_size, depth=depth, hidden_size=hidden_size,
                        map_size=int(map_size), map_scale=float(map_scale), n_linear=n_linear,
                        compute_dtype=compute_dtype, chunk_pixels=chunk_pixels, scratch_format=16)
        self._engine_width = next_kernel_width(hidden_size, self.WIDTHS)
        if self._engine_width is None:
            raise NotImplementedError(f"hidden_size {hidden_size} > 256 is not supported for FourierNet by the gfx950 engine")
        if not engine_takes(input_size, output_size, map_size, n_linear):
            raise NotImplementedError("FourierNet on the gfx950 engine: input_size 2, output_size 3, map_size 64 / 128 / "
                                      f"256 / 512 and 2..12 Linear layers (got {input_size}, {output_size}, {map_size}, {n_linear})")
        self._padded = self._engine_width != hidden_size
        self._enc_key = None

    # ---- engine binding (models/binding.py; these hooks differ) -----------------------------------
    def set_scratch_format(self, fmt: int):
        """FourierNet has one scratch format (16-bit); nothing to switch."""

    def _param_list(self):
        out = []
        for m in self.layers:
            if isinstance(m, nn.Linear):
                out += [m.weight, m.bias]
        return out

    def _handle(self, cls, H: int, w: int, device: int, **more):
        c = self.cfg
        return cls(H, w, self._engine_width, c["n_linear"], c["map_size"], c["output_size"], device=device,
                   chunk_pixels=c["chunk_pixels"], **more)

    def _new_engine(self, H: int, w: int, row_begin: int, row_end: int, device: int):
        from .._engine import FourierEngine
        self._enc_key = None
        return self._handle(FourierEngine, H, w, device, betas=self._adam[0], eps=self._adam[1])

    def _new_render_engine(self, rows: int, cols: int, device: int, side=None):
        from .._engine import FourierRenderEngine
        return self._handle(FourierRenderEngine, rows, cols, device)

    def _load_render_engine(self, eng):
        super()._load_render_engine(eng)
        eng.set_encoding(self.encoding.B.data.float().contiguous().to(eng.device))

    def engine(self, grid: torch.Tensor, img=None, row_begin: int = 0, row_end: int = 0, full_height=None):
        if row_begin or (row_end and row_end != grid.shape[0]) or (full_height and full_height != grid.shape[0]):
            raise NotImplementedError(PIXEL_SPLIT_UNSUPPORTED)
        eng = super().engine(grid, img)
        B = self.encoding.B
        key = (id(eng), B.data_ptr(), B._version)
        if self._enc_key != key:
            eng.set_encoding(B.data.to(eng.device, torch.float32))
            self._enc_key = key
        return eng

    def _layer_fans(self):
        c = self.cfg
        fans = [c["map_size"]] + [c["hidden_size"]] * (c["n_linear"] - 1) + [c["output_size"]]
        return [(fans[l], fans[l + 1], l > 0, l < c["n_linear"] - 1) for l in range(c["n_linear"])]

    def _copy_extras(self, new):
        new.encoding.B.copy_(self.encoding.B)
