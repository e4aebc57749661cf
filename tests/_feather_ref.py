"""fp32 torch mirror of the reference Feathermap forward (pipeline/feathermap/feathernet.py:260-274, 379-385) on a SIREN,
for the tests: W_k = scaler_k * (V1 @ V2).view(-1)[seg_k], then the oracle's SIREN forward; prediction and autograd
gradients of the feather parameters on the CPU, independent of the engine."""
import torch
import torch.nn.functional as F

from oracle import siren_oracle as so


def shapes(hidden, depth, in_features=2, out_features=3):
    """logical (weight shape, bias shape) of every Linear, in flat order"""
    out = []
    for fin, fout in so.layer_dims(hidden, depth, in_features, out_features):
        out += [(fout, fin), (fout,)]
    return out


def weights(V1, V2, scalers, shp, dtype=torch.float32):
    V = (V1.to(dtype) @ V2.to(dtype)).reshape(-1)
    ws, off = [], 0
    for k, s in enumerate(shp):
        n = int(torch.tensor(s).prod())
        ws.append(scalers[k].to(dtype) * V[off:off + n].reshape(s))
        off += n
    return ws


def loss_and_grads(params, shp, grid, img, first_omega_0=50.0, hidden_omega_0=30.0):
    """params: [V1, V2, scaler_0, ..., scaler_{2D-1}] (named_parameters order) -> (pred, loss, [grad of each])"""
    ps = [p.detach().cpu().float().clone().requires_grad_(True) for p in params]
    ws = weights(ps[0], ps[1], [p.reshape(()) for p in ps[2:]], shp)
    pred = so.forward(ws, grid.cpu(), first_omega_0, hidden_omega_0)
    loss = F.mse_loss(pred, img.cpu())
    loss.backward()
    return pred.detach(), loss.item(), [p.grad for p in ps]
