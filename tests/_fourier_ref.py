"""fp32 torch mirror of the reference FourierNet forward (implicit_image/models/fourier.py:21-72) for the GPU tests:
prediction and autograd gradients of a FourierNet's parameters on the CPU, independent of the engine."""
import math

import torch
import torch.nn.functional as F


def forward(B, layers, grid):
    """B [2, M/2]; layers: [(weight, bias), ...]; grid [H, W, 2] -> [H, W, 3]"""
    h, w, _ = grid.shape
    x = (2 * math.pi * grid.reshape(-1, 2)) @ B
    x = torch.cat([torch.sin(x), torch.cos(x)], dim=-1)
    for i, (wt, b) in enumerate(layers):
        x = F.linear(x, wt, b)
        x = torch.relu(x) if i < len(layers) - 1 else torch.sigmoid(x)
    return x.reshape(h, w, -1)


def loss_and_grads(model, grid, img):
    """(pred, loss, [grad per Linear parameter in _param_list order]) of a FourierNet's current weights, fp32 CPU"""
    ps = [p.detach().cpu().float().clone().requires_grad_(True) for p in model._param_list()]
    B = model.encoding.B.detach().cpu().float()
    pred = forward(B, list(zip(ps[0::2], ps[1::2])), grid.cpu())
    loss = F.mse_loss(pred, img.cpu())
    loss.backward()
    return pred.detach(), loss.item(), [p.grad for p in ps]
