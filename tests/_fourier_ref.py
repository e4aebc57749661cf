"""torch mirror of the reference FourierNet forward (implicit_image/models/fourier.py:21-72) for the tests: prediction
and autograd gradients of a FourierNet's parameters on the CPU, independent of the engine, in fp32 or fp64.

engine_model_loss_and_grads() is the numerics model of csrc/fourier_kernels.hip: the same network with the kernels'
rounding points made explicit and everything between them in fp64 (what tests/test_gpu_parity.py's
oracle/engine_model.py is for SIREN).  What separates the engine from it is fp32 summation order, v_sin / v_cos /
v_exp against libm, and the occasional fp16 rounding that flips because of them."""
import math

import torch
import torch.nn.functional as F


def forward(B, layers, grid, dtype=torch.float32):
    """B [2, M/2]; layers: [(weight, bias), ...]; grid [H, W, 2] -> [H, W, 3], computed in `dtype`"""
    h, w, _ = grid.shape
    x = (2 * math.pi * grid.reshape(-1, 2).to(dtype)) @ B.to(dtype)
    x = torch.cat([torch.sin(x), torch.cos(x)], dim=-1)
    for i, (wt, b) in enumerate(layers):
        x = F.linear(x, wt, b)
        x = torch.relu(x) if i < len(layers) - 1 else torch.sigmoid(x)
    return x.reshape(h, w, -1)


def loss_and_grads(model, grid, img, dtype=torch.float32):
    """(pred, loss, [grad per Linear parameter in _param_list order]) of a FourierNet's current weights, CPU"""
    ps = [p.detach().cpu().to(dtype).clone().requires_grad_(True) for p in model._param_list()]
    B = model.encoding.B.detach().cpu()
    pred = forward(B, list(zip(ps[0::2], ps[1::2])), grid.cpu(), dtype)
    loss = F.mse_loss(pred, img.cpu().to(dtype))
    loss.backward()
    return pred.detach(), loss.item(), [p.grad for p in ps]


# ---- the engine's flat layout: layers.{2l}.weight [out][in] row-major, then layers.{2l}.bias, layer after layer ----
def layer_dims(n_linear, width, map_size, out=3):
    """(in, out) of every Linear layer of a FourierNet run at `width` (the engine width when padded)"""
    return [(map_size if l == 0 else width, out if l == n_linear - 1 else width) for l in range(n_linear)]


def split_flat(flat, dims):
    """flat vector -> [(weight [out, in], bias [out]), ...] (views)"""
    layers, off = [], 0
    for fin, fout in dims:
        w = flat[off:off + fin * fout].reshape(fout, fin)
        off += fin * fout
        layers.append((w, flat[off:off + fout]))
        off += fout
    assert off == flat.numel(), (off, flat.numel())
    return layers


def flat_loss_and_grads(B, flat, dims, grid, img, dtype=torch.float64):
    """(pred [H, W, 3], loss, flat gradient) of the mirror on a flat parameter vector, in `dtype`"""
    p = flat.detach().cpu().to(dtype).clone().requires_grad_(True)
    pred = forward(B.detach().cpu(), split_flat(p, dims), grid.cpu(), dtype)
    loss = F.mse_loss(pred, img.cpu().to(dtype))
    loss.backward()
    return pred.detach(), loss.item(), p.grad


def _f16(x):
    """fp32 value rounded to fp16 (round to nearest even: v_cvt_pk_f16_f32 / the (_Float16) casts), back in fp64.
    The engine rounds its fp32 values; going through fp32 keeps the model's fp64 value on the same fp16 neighbour."""
    return x.float().half().double()


def gpre_of(height, width, out=3):
    """the engine's gradient pre-scale: 2^(ceil(log2(3 H W)) + 2) (sf_fourier_create)"""
    return 2.0 ** (math.ceil(math.log2(out * height * width)) + 2)


def engine_encoding(B, grid):
    """[H W, M] encoding as k_ff_fwd / k_ff_dw<*, true> form it: t = fma(x1, B[1, c], fp32(x0 B[0, c])) in fp32 (the
    phase in revolutions), fr = fract(t) (exact in fp32), sin / cos (2 pi fr), rounded to fp16.  The fma is done in
    fp64 (the product of two fp32 values is exact there) and rounded once to fp32."""
    x = grid.reshape(-1, 2).cpu().float()
    Bf = B.detach().cpu().float()
    p = (x[:, :1] * Bf[0][None, :]).double()                       # fp32 product, rounded
    t = (x[:, 1:].double() * Bf[1][None, :].double() + p).float()   # fma: one rounding
    fr = t.double() - torch.floor(t.double())
    ph = 2 * math.pi * fr
    return _f16(torch.cat([torch.sin(ph), torch.cos(ph)], dim=-1))


def _acc32(x, w, b, kstep=16):
    """x [P, K] @ w[N, K]^T (+ b) as an MFMA chain forms it: the accumulator starts at the fp32 bias (or 0) and is
    rounded to fp32 after every k-step of 16 products.  fp16 x fp16 products and their sum over one k-step are exact in
    fp64, so the only rounding left is the one the hardware does when it adds a k-step to the fp32 accumulator (its
    internal order inside a k-step is not modelled).  Measured against the engine, this halves the model's gradient
    gap at 12 Linear layers and leaves the other shapes where an fp64 accumulator puts them: what remains are fp16
    rounding flips caused by v_sin / v_cos and the MFMA's internal order."""
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float64) if b is None else b.float().double().expand(x.shape[0], -1)
    for k in range(0, x.shape[1], kstep):
        acc = (acc + x[:, k:k + kstep] @ w[:, k:k + kstep].T).float().double()
    return acc


def engine_model_loss_and_grads(B, flat, dims, grid, img):
    """(pred [H, W, 3], sse, flat gradient), fp64, of fourier_kernels.hip with its rounding points:
      - encoding: engine_encoding() (fp32 phase in revolutions, fp16 features);
      - every weight is used as fp16 (k_ff_images, no pre-scale); each layer accumulates from its fp32 bias, in fp32,
        one v_mfma_f32_32x32x16_f16 k-step (16 products, summed exactly here) at a time, in k order (_acc32);
      - each ReLU output is rounded to fp16 once: it is the next layer's operand and the H spill;
      - output: sigmoid, residual r = s - y, dz = 2 r s (1 - s) * gpre / (3 H W) stored as fp16 (the Z plane);
      - backward: acc = W_l^T g_l with fp16 operands, g_{l-1} = fp16(acc) * [fp16(h_{l-1}) > 0];
      - dW_l = g_l h_{l-1}^T (layer 0: g_0 enc^T) and db_l = sum g_l over pixels, then * 1 / gpre (a power of two).
    Pixels are the real ones only: the kernels' padding lanes (clamped coordinates) carry dz = 0, hence g = 0."""
    H, W, _ = grid.shape
    flat = flat.detach().cpu()
    layers = [(_f16(w), b.double()) for w, b in split_flat(flat, dims)]
    gpre = gpre_of(H, W)
    gscale = float(torch.tensor(gpre / (3.0 * H * W), dtype=torch.float32))
    y = img.detach().cpu().reshape(-1, 3).double()
    x = engine_encoding(B, grid)                                    # [P, M]
    hs = [x]
    for w, b in layers[:-1]:
        x = _f16(torch.relu(_acc32(x, w, b)))
        hs.append(x)
    w, b = layers[-1]
    s = torch.sigmoid(_acc32(x, w, b))
    r = s - y
    sse = float((r * r).sum())
    dz = _f16(2.0 * r * s * (1.0 - s) * gscale)                     # [P, 3]
    grads = [None] * len(layers)
    g = dz
    for l in range(len(layers) - 1, -1, -1):
        grads[l] = ((g.T @ hs[l]) / gpre, g.sum(0) / gpre)
        if l == 0:
            break
        g = _f16(_acc32(g, layers[l][0].T, None)) * (hs[l] > 0)
    flat_g = torch.cat([t.reshape(-1) for pair in grads for t in pair])
    return s.reshape(H, W, 3), sse, flat_g
