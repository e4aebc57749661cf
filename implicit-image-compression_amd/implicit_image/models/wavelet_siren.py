"""WaveletSiren with the reference's constructor, submodule and parameter names and random-draw order
(reference: implicit_image/models/wavelet_siren.py:12-106), executed by the gfx950 engine (sf_wavelet_create: two SIREN
sub-networks plus csrc/wavelet_kernels.hip for the inverse DWT, the Cb / Cr upsampling and YCbCr -> RGB).

`LF_siren` / `HF_siren` are ordinary Siren modules that only own names and shapes: once bound, every
`{LF,HF}_siren.layers.{i}.linear.{weight,bias}` is a zero-copy view of the engine's flat fp32 state [LF | HF].
forward() runs the HIP kernels; there is no PyTorch arithmetic fallback.
"""
from typing import Optional

import numpy as np
import torch

from ..data import get_grid
from .binding import EngineBound
from .siren import Siren

# the reference's Masking.add_module runs a FLOP-counting forward on a 1x1 grid: 3x3 coefficients, a 2x2 inverse DWT
# against 1x1 upsampled chroma, and a failing torch.cat (it would also fix the cached coefficient size at 3)
MASKING_UNSUPPORTED = ("mask-based sparsity (RigL / SNFS / SET / Pruning) is not supported on WaveletSiren: the reference's "
                       "Masking.add_module counts FLOPs with a 1x1 forward, whose 2x2 inverse DWT and 1x1 Cb / Cr fail "
                       "torch.cat (and would poison the cached LF_h). Use masking=none or masking=Small_Dense")
PIXEL_SPLIT_UNSUPPORTED = "pixel-split (row ranges) is not supported for WaveletSiren: the inverse DWT couples rows"


def coeff_len(h: int) -> int:
    """pywt.dwt_coeff_len(h, 6, "zero"): the db3 coefficient length the reference's DWT probe reports"""
    return (h + 5) // 2


def check_image(h: int, w: int):
    if h != w or h % 2:
        raise NotImplementedError(
            f"WaveletSiren needs an even, square image (got {h}x{w}): in the reference the inverse DWT gives "
            f"{2 * coeff_len(h) - 4}x{2 * coeff_len(w) - 4} and torch.cat with the {h}x{w} Cb / Cr fails")


class WaveletSiren(EngineBound):
    WIDTHS = Siren.WIDTHS          # the sub-networks' (the constructor refuses what the narrow kernel path cannot run)
    mask_unsupported = MASKING_UNSUPPORTED
    split_unsupported = PIXEL_SPLIT_UNSUPPORTED

    def __init__(self, input_size: int = 2, output_size: int = 3, depth: int = 8, hidden_size: int = 64,
                 wavelet_levels: int = 1, first_omega_0: float = 50.0, hidden_omega_0: float = 50.0,
                 outermost_linear: bool = True, simulate_quantization: bool = False, small_dense_density: float = 1.0,
                 compute_dtype: str = "f16", chunk_pixels: int = 0, scratch_format: int = 0, **kwargs):
        super().__init__()
        if compute_dtype != "f16":
            raise NotImplementedError("WaveletSiren runs fp16 MFMA operands only (engine.compute_dtype=f16)")
        if scratch_format not in (0, 16):
            raise NotImplementedError("WaveletSiren runs scratch format 16: format 8 takes its fp8 delta scale from the "
                                      "fused residual, which a WaveletSiren pass does not form")
        if wavelet_levels != 1:
            raise NotImplementedError(f"wavelet_levels={wavelet_levels}: the reference's single-level inverse DWT receives "
                                      f"{3 * wavelet_levels} bands and fails; only wavelet_levels=1 runs")
        if input_size != 2 or output_size != 3:
            raise NotImplementedError("WaveletSiren on the gfx950 engine: input_size 2, output_size 3")
        hidden_size = int(hidden_size * np.sqrt(small_dense_density))   # Small_Dense, once (reference :30)
        self.output_size, self.wavelet_levels, self.wavelet_windows = output_size, wavelet_levels, 3
        # the reference's draw order: every LF tensor, then every HF tensor (:37-60); each inner Siren gets density 1
        self.LF_siren = Siren(input_size, output_size, depth, hidden_size, first_omega_0, hidden_omega_0,
                              outermost_linear, simulate_quantization)
        self.HF_siren = Siren(input_size, output_size * wavelet_levels, depth, hidden_size, first_omega_0,
                              hidden_omega_0, outermost_linear, simulate_quantization)
        self.LF_h = None
        self.simulate_quantization = simulate_quantization
        self.cfg = dict(input_size=input_size, output_size=output_size, depth=depth, hidden_size=hidden_size,
                        wavelet_levels=wavelet_levels, first_omega_0=float(first_omega_0),
                        hidden_omega_0=float(hidden_omega_0), outermost_linear=bool(outermost_linear),
                        compute_dtype=compute_dtype, chunk_pixels=chunk_pixels, scratch_format=16)
        self._engine_width = self.LF_siren._engine_width
        if self._engine_width > 256:
            raise NotImplementedError(f"hidden_size {hidden_size} > 256 is not supported for WaveletSiren by the gfx950 "
                                      "engine (the narrow kernel path only)")
        self._padded = self._engine_width != hidden_size
        self._image_h = None
        self._coeff_grid = None

    # ---- engine binding (models/binding.py; these hooks differ) ------------------------------------------------------
    def set_scratch_format(self, fmt: int):
        """WaveletSiren has one scratch format (16-bit); nothing to switch."""

    def _param_list(self):
        return self.LF_siren._param_list() + self.HF_siren._param_list()

    def _sub_engine_params(self) -> int:
        wp, D = self._engine_width, self.cfg["depth"]
        return 3 * wp + (D - 2) * (wp * wp + wp) + 3 * wp + 3

    def _layer_fans(self):
        """LF's layers, then HF's: the joint [LF | HF] pad index (HF starts _sub_engine_params() slots in)"""
        return self.LF_siren._layer_fans() + self.HF_siren._layer_fans()

    def _new_engine(self, H: int, w: int, row_begin: int, row_end: int, device: int):
        from .._engine import WaveletEngine
        c = self.cfg
        return WaveletEngine(self._image_h, self._image_h, self._engine_width, c["depth"], c["first_omega_0"],
                             c["hidden_omega_0"], c["outermost_linear"], device=device, chunk_pixels=c["chunk_pixels"],
                             betas=self._adam[0], eps=self._adam[1], wavelet_levels=c["wavelet_levels"])

    def _new_render_engine(self, rows: int, cols: int, device: int, side: Optional[int] = None):
        from .._engine import WaveletRenderEngine
        c = self.cfg
        return WaveletRenderEngine(side, self._engine_width, c["depth"], c["first_omega_0"], c["hidden_omega_0"],
                                   c["outermost_linear"], c["compute_dtype"], max_rows=rows, max_cols=cols, device=device,
                                   chunk_pixels=c["chunk_pixels"])

    def _load_render_engine(self, eng):
        super()._load_render_engine(eng)
        lin = torch.linspace(0, 1, eng.n).to(eng.device)      # LF_grid = HF_grid = get_grid(n, n) (wavelet_siren.py:76-80)
        eng.set_coords(lin, lin)

    def shape_probe(self, h: int, w: int):
        """The reference's first forward: a DWT of torch.rand(1, 1, h, w) from the CPU generator fixes the coefficient
        size (wavelet_siren.py:70-74); the draw is repeated so that the generator state matches."""
        if not self.LF_h:
            torch.rand(1, 1, h, w)
            self.LF_h = self.LF_w = coeff_len(h)
            self.HF_h_ll, self.HF_w_ll = [coeff_len(h)], [coeff_len(w)]

    def engine(self, grid: torch.Tensor, img: Optional[torch.Tensor] = None, row_begin: int = 0, row_end: int = 0,
               full_height: Optional[int] = None):
        h, w, _ = grid.shape
        if row_begin or (row_end and row_end != h) or (full_height and full_height != h):
            raise NotImplementedError(PIXEL_SPLIT_UNSUPPORTED)
        check_image(h, w)
        self._check_device(grid)
        self.shape_probe(h, w)
        if self.LF_h != coeff_len(h):   # the reference keeps the first coefficient size (LF_h is cached)
            raise NotImplementedError(f"WaveletSiren was first run on a {2 * self.LF_h - 4}x{2 * self.LF_h - 4} image: the "
                                      "reference caches LF_h and cannot change the image size afterwards")
        self._image_h = h
        n = coeff_len(h)
        if self._coeff_grid is None or self._coeff_grid.device != grid.device or self._coeff_grid.shape[0] != n:
            self._coeff_grid = get_grid(n, n, device=grid.device)   # LF_grid = HF_grid (wavelet_siren.py:76-80)
        return super().engine(self._coeff_grid, img)

    def _copy_extras(self, new):
        new.LF_h = self.LF_h
