"""WaveletSiren for the tests: a torch mirror of the reference's forward (implicit_image/models/wavelet_siren.py:66-106)
in any dtype, and the stand-ins for the two libraries the reference imports that are not installed here.

  pytorch_wavelets   DWTForward (the reference only reads the shapes of its output) and DWTInverse, a conv_transpose2d
                     restatement of the library's zero-mode synthesis (lowlevel.sfb1d / SFB2D); wavelet_idwt.npz (minted
                     by PyWavelets) pins it
  kornia             color.ycbcr.ycbcr_to_rgb (four constants of kornia's source)

These stubs are this project's code: tests/golden/make_golden_wavelet.py installs them to import the real reference.
"""
import sys
import types

import torch
import torch.nn.functional as F
from torch import nn

# pywt.Wavelet("db3").rec_lo / rec_hi (PyWavelets 1.1.1)
REC_LO = (0.33267055295008263, 0.8068915093110925, 0.45987750211849154, -0.13501102001025458, -0.08544127388202666,
          0.03522629188570953)
REC_HI = (0.03522629188570953, 0.08544127388202666, -0.13501102001025458, -0.45987750211849154, 0.8068915093110925,
          -0.33267055295008263)


def coeff_len(h: int) -> int:
    """pywt.dwt_coeff_len(h, 6, "zero")"""
    return (h + 5) // 2


def _sfb1d(lo, hi, g0, g1, dim):
    C, L = lo.shape[1], g0.numel()
    shape = (1, 1, L, 1) if dim == 2 else (1, 1, 1, L)
    s = (2, 1) if dim == 2 else (1, 2)
    pad = (L - 2, 0) if dim == 2 else (0, L - 2)
    g0 = g0.reshape(shape).repeat(C, 1, 1, 1)
    g1 = g1.reshape(shape).repeat(C, 1, 1, 1)
    return (F.conv_transpose2d(lo, g0, stride=s, padding=pad, groups=C)
            + F.conv_transpose2d(hi, g1, stride=s, padding=pad, groups=C))


def idwt(ll, highs, g0=None, g1=None):
    """ll [N, C, n, n], highs [N, C, 3, n, n] (LH, HL, HH) -> [N, C, 2n - 4, 2n - 4]: the column filter along the height
    first, then the row filter along the width (SFB2D.forward)"""
    g0 = torch.tensor(REC_LO, dtype=ll.dtype, device=ll.device) if g0 is None else g0
    g1 = torch.tensor(REC_HI, dtype=ll.dtype, device=ll.device) if g1 is None else g1
    lh, hl, hh = torch.unbind(highs, dim=2)
    lo = _sfb1d(ll, lh, g0, g1, 2)
    hi = _sfb1d(hl, hh, g0, g1, 2)
    return _sfb1d(lo, hi, g0, g1, 3)


def ycbcr_to_rgb(image):
    y, cb, cr = image[..., 0, :, :], image[..., 1, :, :], image[..., 2, :, :]
    cb_s, cr_s = cb - 0.5, cr - 0.5
    r = y + 1.403 * cr_s
    g = y - 0.714 * cr_s - 0.344 * cb_s
    b = y + 1.773 * cb_s
    return torch.stack([r, g, b], -3)


class DWTInverse(nn.Module):
    def __init__(self, wave="db3", mode="zero"):
        super().__init__()
        assert wave == "db3" and mode == "zero"
        self.register_buffer("g0", torch.tensor(REC_LO, dtype=torch.get_default_dtype()))
        self.register_buffer("g1", torch.tensor(REC_HI, dtype=torch.get_default_dtype()))

    def forward(self, coeffs):
        yl, yh = coeffs
        assert len(yh) == 1, "stub: single level"
        return idwt(yl, yh[0], self.g0.to(yl.dtype), self.g1.to(yl.dtype))


class DWTForward(nn.Module):
    """Shapes only: the reference reads Yl.shape and Yh[k].shape of a random probe (wavelet_siren.py:70-74)."""

    def __init__(self, J=1, wave="db3", mode="zero"):
        super().__init__()
        assert wave == "db3" and mode == "zero"
        self.J = J

    def forward(self, x):
        N, C, h, w = x.shape
        yh = []
        for _ in range(self.J):
            h, w = coeff_len(h), coeff_len(w)
            yh.append(torch.zeros(N, C, 3, h, w))
        return torch.zeros(N, C, h, w), yh


def install_stubs():
    """sys.modules entries for pytorch_wavelets and kornia (and for the reference data.py's other imports)"""
    pw = types.ModuleType("pytorch_wavelets")
    pw.DWTInverse, pw.DWTForward = DWTInverse, DWTForward
    sys.modules["pytorch_wavelets"] = pw
    kornia = types.ModuleType("kornia")
    color = types.ModuleType("kornia.color")
    ycbcr = types.ModuleType("kornia.color.ycbcr")
    ycbcr.ycbcr_to_rgb = ycbcr_to_rgb
    color.ycbcr = ycbcr
    kornia.color = color
    sys.modules.update({"kornia": kornia, "kornia.color": color, "kornia.color.ycbcr": ycbcr})
    for name in ("cv2",):
        sys.modules.setdefault(name, types.ModuleType(name))
    try:
        import matplotlib.pyplot  # noqa: F401
    except ImportError:
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules.update({"matplotlib": mpl, "matplotlib.pyplot": mpl.pyplot})


# ---- the mirror ------------------------------------------------------------------------------------------------------
def compose(lf, hf, H, interp_dtype=None):
    """LF / HF predictions [n, n, 3] -> RGB [H, H, 3] (wavelet_siren.py:82-106); interp_dtype: run the upsampling in that
    type (torch forms its source index and weights in the input's type)"""
    n = lf.shape[0]
    y = idwt(lf[..., 0][None, None], hf.permute(2, 0, 1)[None, None])
    x = lf[..., 1:].permute(2, 0, 1)[None]
    cbcr = F.interpolate(x if interp_dtype is None else x.to(interp_dtype), scale_factor=H / n, mode="bilinear",
                         align_corners=False).to(lf.dtype)
    return ycbcr_to_rgb(torch.cat((y, cbcr), 1))[0].permute(1, 2, 0)


def sub_dims(hidden, depth, out=3):
    return [(hidden if l < depth - 1 else out, 2 if l == 0 else hidden) for l in range(depth)]


def split_flat(flat, hidden, depth):
    """joint flat vector [LF | HF] (logical widths) -> two lists [W0, b0, W1, b1, ...]"""
    out, off = [], 0
    for _ in range(2):
        ps = []
        for o, i in sub_dims(hidden, depth):
            ps.append(flat[off:off + o * i].view(o, i)); off += o * i
            ps.append(flat[off:off + o]); off += o
        out.append(ps)
    assert off == flat.numel()
    return out


def model_flat(model):
    return torch.cat([p.detach().reshape(-1).float() for p in model._param_list()])


def forward(flat, hidden, depth, H, first_omega_0=50.0, hidden_omega_0=30.0, dtype=torch.float64):
    from oracle import siren_oracle as so
    n = coeff_len(H)
    grid = so.get_grid(n, n).to(dtype)
    lfp, hfp = split_flat(flat.to(dtype), hidden, depth)
    lf = so.forward(lfp, grid, first_omega_0, hidden_omega_0)
    hf = so.forward(hfp, grid, first_omega_0, hidden_omega_0)
    return lf, hf, compose(lf, hf, H)


def loss_and_grads(flat, hidden, depth, img, first_omega_0=50.0, hidden_omega_0=30.0, dtype=torch.float64):
    """prediction, F.mse_loss and its gradient w.r.t. the joint flat vector (autograd in `dtype`)"""
    p = flat.detach().to(dtype).clone().requires_grad_(True)
    _, _, rgb = forward(p, hidden, depth, img.shape[0], first_omega_0, hidden_omega_0, dtype)
    loss = F.mse_loss(rgb, img.to(dtype))
    g, = torch.autograd.grad(loss, p)
    return rgb.detach(), float(loss.detach()), g
