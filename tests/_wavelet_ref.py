"""WaveletSiren for the tests: a torch mirror of the reference's forward (implicit_image/models/wavelet_siren.py:66-106)
in any dtype, a numerics model of the engine's WaveletSiren pass (engine_model_loss_and_grads), and the stand-ins for
the two libraries the reference imports that are not installed here.

  pytorch_wavelets   DWTForward (the reference only reads the shapes of its output) and DWTInverse, a conv_transpose2d
                     restatement of the library's zero-mode synthesis (lowlevel.sfb1d / SFB2D); wavelet_idwt.npz (minted
                     by PyWavelets) pins it
  kornia             color.ycbcr.ycbcr_to_rgb (four constants of kornia's source)

These stubs are this project's code: tests/golden/make_golden_wavelet.py installs them to import the real reference.
"""
import math
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


def forward(flat, hidden, depth, H, first_omega_0=50.0, hidden_omega_0=30.0, dtype=torch.float64, outermost_linear=True):
    """LF / HF predictions [n, n, 3] and the RGB image [H, H, 3], in `dtype` on flat's device"""
    from oracle import siren_oracle as so
    n = coeff_len(H)
    grid = so.get_grid(n, n).to(device=flat.device, dtype=dtype)
    lfp, hfp = split_flat(flat.to(dtype), hidden, depth)
    lf = so.forward(lfp, grid, first_omega_0, hidden_omega_0, outermost_linear=outermost_linear)
    hf = so.forward(hfp, grid, first_omega_0, hidden_omega_0, outermost_linear=outermost_linear)
    return lf, hf, compose(lf, hf, H)


def loss_and_grads(flat, hidden, depth, img, first_omega_0=50.0, hidden_omega_0=30.0, dtype=torch.float64,
                   outermost_linear=True):
    """prediction, F.mse_loss and its gradient w.r.t. the joint flat vector (autograd in `dtype`, on img's device)"""
    p = flat.detach().to(device=img.device, dtype=dtype).clone().requires_grad_(True)
    _, _, rgb = forward(p, hidden, depth, img.shape[0], first_omega_0, hidden_omega_0, dtype, outermost_linear)
    loss = F.mse_loss(rgb, img.to(dtype))
    g, = torch.autograd.grad(loss, p)
    return rgb.detach(), float(loss.detach()), g


# ---- the numerics model of the engine's pass -------------------------------------------------------------------------
def gpre_of(H):
    """the sub-networks' dL/dout pre-scale (sf_wavelet_create): 2^(ceil(log2(3 H^2)) + 2), from the 3 H^2 values of the
    image (what the loss mean divides by), not from the n^2 coefficients"""
    return 2.0 ** (math.ceil(math.log2(3.0 * H * H)) + 2)


def sub_forward16(params, grid, first_omega_0, hidden_omega_0, outermost_linear=True):
    """The forward of oracle/engine_model.loss_and_grads(fwd="f16", scratch=16), stopped at the output: layer 0 in fp32,
    hidden layers with fp16 operands (omega / 2 pi folded into the weight images, the accumulator is the phase), unorm16
    phases spilled, last layer with weights x 2^8.  A sine output layer (outermost_linear=False) takes its phase as
    fwd_residual does, tt = fp32(o * fp32(omega / 2 pi)), and yields d sin(omega z)/dz = omega cos(2 pi tt) per output.
    Returns (p [N, 3] fp32, dfac [N, 3] fp32 or None, state for sub_backward16)."""
    from oracle import engine_model as em
    depth = len(params) // 2
    x = (grid.reshape(-1, 2) - 0.5) * 2
    W0, b0 = params[0], params[1]
    z = torch.addcmul(torch.addcmul(b0, x[:, 0:1], W0[:, 0]), x[:, 1:2], W0[:, 1])
    t = z * torch.tensor(first_omega_0 / em.TWO_PI, dtype=torch.float32)
    ph0 = t - torch.floor(t)
    hs = torch.tensor(hidden_omega_0 / em.TWO_PI, dtype=torch.float32)
    q = [None]
    a = torch.sin(em.TWO_PI * t.double()).float()
    for l in range(1, depth - 1):
        t = em._rt(a, "f16") @ em._rt(params[2 * l] * hs, "f16").t() + params[2 * l + 1] * hs
        q.append(em._phase_q(t))
        a = torch.sin(em.TWO_PI * t.double()).float()
    L = depth - 1
    out = (em._rt(a, "f16") @ em._rt(params[2 * L] * 256.0, "f16").t() + params[2 * L + 1] * 256.0) * (1.0 / 256.0)
    dfac = None
    if not outermost_linear:
        tt = out * torch.tensor(hidden_omega_0 / em.TWO_PI, dtype=torch.float32)
        out = torch.sin(em.TWO_PI * tt.double()).float()
        dfac = torch.tensor(hidden_omega_0, dtype=torch.float32) * torch.cos(em.TWO_PI * tt.double()).float()
    return out * 0.5 + 0.5, dfac, (x, ph0, q)


def sub_backward16(params, state, dlast, scale, first_omega_0, hidden_omega_0):
    """The backward of oracle/engine_model.loss_and_grads(fwd="f16", scratch=16) from dlast = dL/dz of the last layer
    times `scale` (fp16 values): every delta is an fp16 value at that scale, activations re-derived from the unorm16
    phases (layer 0's from the coordinates), weight images fp16(W omega).  Returns [dW0, db0, dW1, ...] (fp32)."""
    from oracle import engine_model as em
    x, ph0, q = state
    depth = len(params) // 2
    delta = dlast.float() * (1.0 / scale)
    grads = [None] * (2 * depth)
    for l in range(depth - 1, 0, -1):
        ph = ph0 if l - 1 == 0 else q[l - 1] * (1.0 / 65536.0)
        act = em._rt(torch.sin(em.TWO_PI * ph.double()).float(), "f16")
        grads[2 * l] = delta.t() @ act
        grads[2 * l + 1] = delta.sum(0)
        om = first_omega_0 if l - 1 == 0 else hidden_omega_0
        G = delta @ em._rt(params[2 * l] * om, "f16")
        delta = em._rt(G * torch.cos(em.TWO_PI * ph.double()).float() * scale, "f16") * (1.0 / scale)
    xh = em._rt(x, "f16")
    xl = em._rt(x - xh, "f16")
    grads[0] = delta.t() @ xh + delta.t() @ xl
    grads[1] = delta.sum(0)
    return grads


def compose_adjoint(gy, n, H):
    """dL/d(lf, hf) [n, n, 3] each from dL/d(Y, Cb, Cr) [H, H, 3] (fp64): the synthesis adjoint in fp64, the bilinear
    adjoint through torch's fp32 F.interpolate (its fp32 source index and weights, as k_wv_adjoint)"""
    a = torch.zeros(n, n, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(n, n, 3, dtype=torch.float64, requires_grad=True)
    Y = idwt(a[None, None], b.permute(2, 0, 1)[None, None])[0, 0]
    dll, dhf = torch.autograd.grad((Y * gy[..., 0]).sum(), (a, b))
    x = torch.zeros(1, 2, n, n, dtype=torch.float32, requires_grad=True)
    up = F.interpolate(x, scale_factor=H / n, mode="bilinear", align_corners=False)
    dcc, = torch.autograd.grad(up, x, grad_outputs=gy[..., 1:].permute(2, 0, 1)[None].float())
    dlf = torch.cat([dll[..., None], dcc[0].permute(1, 2, 0).double()], -1)
    return dlf, dhf


def engine_model_loss_and_grads(flat, width, depth, img, first_omega_0=50.0, hidden_omega_0=30.0, outermost_linear=True):
    """(pred [H, H, 3], sse, flat gradient) of the engine's WaveletSiren pass on its flat parameter vector (engine
    layout: [LF | HF] at the engine width), with the engine's rounding points:
      1. each sub-network's forward: sub_forward16 (fp16 operands, weights x 2^8, unorm16 hidden phases);
      2. the composition of the two fp32 predictions: inverse DWT in fp64, Cb / Cr upsampled with torch's fp32
         bilinear index and weights;
      3. the adjoint: dL/d(Y, Cb, Cr) = colour-transform adjoint of 2 (rgb - img) / (3 H^2), then compose_adjoint;
      4. dL/dout = fp16(dL/dp * 1/2 * gpre, times dfac for a sine output), rounded once; gpre = gpre_of(H);
      5. each sub-network's backward: sub_backward16 at scale gpre; the gradients are fp32 sums undone by 1 / gpre.
    What separates the engine from it is fp32 summation order (MFMA, the composition) and v_sin / v_cos against libm:
    the occasional fp16 rounding of a phase, an activation or a delta that falls the other way."""
    from oracle import siren_oracle as so
    H = img.shape[0]
    n = coeff_len(H)
    grid = so.get_grid(n, n)
    gpre = gpre_of(H)
    subs = split_flat(flat.detach().cpu().float(), width, depth)
    outs = [sub_forward16(ps, grid, first_omega_0, hidden_omega_0, outermost_linear) for ps in subs]
    lf, hf = (o[0].reshape(n, n, 3) for o in outs)
    y = img.detach().cpu().double()
    rgb = compose(lf.double(), hf.double(), H, interp_dtype=torch.float32)
    e = rgb - y
    sse = float((e * e).sum())
    d = e * (2.0 / (3.0 * H * H))
    gy = torch.stack([d[..., 0] + d[..., 1] + d[..., 2], 1.773 * d[..., 2] - 0.344 * d[..., 1],
                      1.403 * d[..., 0] - 0.714 * d[..., 1]], -1)
    grads = []
    for (p, dfac, state), ps, dp in zip(outs, subs, compose_adjoint(gy, n, H)):
        dz = dp.reshape(-1, 3) * (0.5 * gpre)
        if dfac is not None:
            dz = dz * dfac.double()
        dlast = dz.float().half().float()
        grads += sub_backward16(ps, state, dlast, gpre, first_omega_0, hidden_omega_0)
    return rgb, sse, torch.cat([g.reshape(-1) for g in grads]).double()
