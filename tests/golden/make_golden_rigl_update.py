#!/usr/bin/env python3
"""Golden vectors for the device topology update (sf_mask_update), minted by running the REAL reference.

    python tests/golden/make_golden_rigl_update.py

RigL as conf/masking/RigL.yaml configures it (ERK 0.5, magnitude pruning at 0.1 under cosine decay, absolute-gradient
growth, dense gradients) on the 64x4 model and the 32x32 formula image, updates every 5 steps: right before the
`update_connections()` calls at steps 5 and 10 the full state (weights, gradients, Adam moments, masks, decay state) is
captured, and the state right after them - the keys of masking_snfs.npz -> masking_rigl.npz.

The device path orders equal keys by index where torch.sort leaves their order open, so the fixture is only usable if no
selection boundary in it falls inside a group of ties: asserted here with tests/_mask_update_ref.py, which must also
reproduce the reference's post-update state bit for bit.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m


class Cfg(dict):
    __getattr__ = dict.get


def flat(ts):
    return np.concatenate([t.detach().numpy().ravel() for t in ts]).astype(np.float32)


def main():
    sys.path.insert(0, REF)
    _stub("omegaconf", DictConfig=dict, OmegaConf=object)
    _stub("torch_optimizer", Shampoo=object)
    from implicit_image.utils import train_helper as th
    spec = importlib.util.spec_from_file_location("ref_siren", f"{REF}/implicit_image/models/siren.py")
    siren = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(siren)
    sys.path.insert(0, os.path.dirname(OUT))
    from golden.make_golden import synthetic_image  # noqa: the same formula image
    from _mask_update_ref import bits_rate, mask_update_ref

    hw = 32
    img = synthetic_image(hw, hw, seed=5)
    gh = torch.linspace(0, 1, hw)
    grid = torch.stack(torch.meshgrid(gh, gh, indexing="ij"), dim=-1)
    mcfg = Cfg(name="RigL", density=0.5, sparse_init="erdos-renyi-kernel", dense_gradients=True,
               growth_mode="absolute-gradient", prune_mode="magnitude", redistribution_mode="none", dense=False,
               prune_rate=0.1, decay_schedule="cosine", end_when=60, interval=5)
    torch.manual_seed(0)
    m = siren.Siren(depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30)
    optim, sched = th.get_optimizer_lr_scheduler(m, Cfg(name="adam", lr=3e-4))
    mask = th.setup_mask(m, optim, mcfg)
    names = [n for n, _ in m.named_parameters() if n in mask.mask_dict]
    slices, off = [], 0
    for n, p in m.named_parameters():
        if n in mask.mask_dict:
            slices.append((off, p.numel()))
        off += p.numel()

    def mask_bits():
        return np.packbits(np.concatenate([mask.mask_dict[n].numpy().ravel().astype(np.uint8) for n in names]))

    def flat_mask():
        return torch.cat([(mask.mask_dict[n] if n in mask.mask_dict else torch.ones_like(p)).reshape(-1).float()
                          for n, p in m.named_parameters()])

    out = {"mask_names": np.array(names), "mask_init": mask_bits()}
    rates = []
    for i in range(13):
        th.train_epoch(m, optim, grid, img, lr_scheduler=sched, mask=mask)
        rates.append(mask.prune_rate)
        if i in (5, 10):
            pre = f"u{i}_"
            out[pre + "w"] = flat(m.parameters())
            out[pre + "g"] = flat([p.grad for p in m.parameters()])
            out[pre + "m"] = flat([optim.state[p]["exp_avg"] for p in m.parameters()])
            out[pre + "v"] = flat([optim.state[p]["exp_avg_sq"] for p in m.parameters()])
            out[pre + "mask"] = mask_bits()
            out[pre + "mask_step"] = mask.mask_step
            out[pre + "rate"] = mask.prune_rate
            out[pre + "adjusted_growth"] = float(mask.adjusted_growth)
            out[pre + "adjustments"] = np.array(mask.adjustments, dtype=np.float64)
            out[pre + "prune_threshold"] = float(mask.prune_threshold)
            out[pre + "total_nonzero"] = mask.stats.total_nonzero
            out[pre + "total_zero"] = mask.stats.total_zero
            state = [torch.tensor(out[pre + k]) for k in "wgmv"] + [flat_mask()]
            mask.update_connections()
            post = f"a{i}_"
            out[post + "w"] = flat(m.parameters())
            out[post + "m"] = flat([optim.state[p]["exp_avg"] for p in m.parameters()])
            out[post + "mask"] = mask_bits()
            out[post + "mask_step"] = mask.mask_step
            out[post + "nnz"] = np.array([int(mask.mask_dict[n].sum().item()) for n in names])
            out[post + "adjusted_growth"] = float(mask.adjusted_growth)
            out[post + "prune_threshold"] = float(mask.prune_threshold)
            out[post + "density"] = mask.stats.total_density
            # the restatement on the captured state: no boundary tied, and the reference's result bit for bit
            rows, tied = mask_update_ref(*state, slices, float(out[pre + "rate"]), 1, True)
            assert not any(any(t) for t in tied), (i, tied)
            assert np.array_equal(state[0].numpy().view(np.int32), out[post + "w"].view(np.int32)), i
            assert np.array_equal(state[2].numpy().view(np.int32), out[post + "m"].view(np.int32)), i
            assert torch.equal(state[4], flat_mask()), i
            assert rows[:-1, 4].tolist() == out[post + "nnz"].tolist() and int(rows[-1, 0]) == 0
            assert [bits_rate(r[7]) for r in rows[:-1]] == [mask.name2prune_rate[n] for n in names]
        elif i <= mcfg.end_when and i % mcfg.interval == 0:
            mask.update_connections()
    out["rates"] = np.array(rates, dtype=np.float64)
    np.savez_compressed(f"{OUT}/masking_rigl.npz", **out)
    print("rigl rates", [round(r, 5) for r in rates[:7]], "nnz", out["a10_nnz"].tolist(), "density", out["a10_density"])


if __name__ == "__main__":
    main()
