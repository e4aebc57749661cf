#!/usr/bin/env python3
"""Golden vectors of the compressed container at quant.bits=9 (the reference's final recipe, slurm_scripts/finals.sh:74),
minted by running the REAL reference code, as tests/golden/make_golden_quant.py does for bits 8:

    python tests/golden/make_golden_quant9.py

The same stubs, the same arithmetic stand-in for torch_scatter.scatter_mean (centroid VALUES stay parity unpinned at that
boundary) and the same trained 64x4 weights (hot_64x4_256.npz, 40 % of layer 1 zeroed).  At bits 9 layers 1
and 2 get more than 256 centroids, so the reference's linear_state_dict writes their labels as torch.uint16
(pipeline/entropy_coding/__init__.py:33-39).
Writes: container_64x4_bits9.npz (plain + lzma byte streams, meta_data.json, the decoded tensors).
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_quant import REF, _TT, _stub, scatter_mean   # noqa: E402  (the stubs, once)

BITS = 9


def main():
    sys.path.insert(0, REF)
    _stub("omegaconf", DictConfig=dict, OmegaConf=object)
    _stub("torch_optimizer", Shampoo=object)
    _stub("torch_scatter", scatter_mean=scatter_mean)
    _stub("torchtyping", TensorType=_TT)
    _stub("zstandard")
    from implicit_image.pipeline.quant.kmeans import KmeansQuant
    from implicit_image.pipeline import entropy_coding
    spec = importlib.util.spec_from_file_location("ref_siren", f"{REF}/implicit_image/models/siren.py")
    siren = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(siren)

    hot = np.load(f"{OUT}/hot_64x4_256.npz")
    torch.manual_seed(0)
    model = siren.Siren(depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30)
    off = 0
    with torch.no_grad():
        for p in model.parameters():
            n = p.numel()
            p.copy_(torch.tensor(hot["final"][off:off + n]).view(p.shape))
            off += n
        g = torch.Generator().manual_seed(11)
        model.layers[1].linear.weight.mul_((torch.rand(64, 64, generator=g) > 0.4).float())
    optim = torch.optim.Adam(model.parameters(), lr=3e-4)
    comp = KmeansQuant(model, optim, bits=BITS, skip_ll=["layers.0.linear", "layers.3.linear"])
    model(torch.rand(3, 3, 2, generator=torch.Generator().manual_seed(1)))      # fires the forward pre-hooks
    comp.update_weights()
    sd_keys = list(model.state_dict().keys())
    half = model.half()
    res = {"state_dict_keys": np.array(sd_keys),
           "n_centroids": np.array([model.layers[l].linear.centroids.numel() for l in (1, 2)])}
    for stream in ("plain", "lzma"):
        with tempfile.TemporaryDirectory() as d:
            nbytes = entropy_coding.compress_state_dict(half, d, stream_name=stream)
            res[f"{stream}_bytes"] = np.frombuffer(open(os.path.join(d, "compressed_weights.data"), "rb").read(), np.uint8)
            res[f"{stream}_meta"] = np.array(open(os.path.join(d, "meta_data.json")).read())
            res[f"{stream}_reported_size"] = nbytes
            if stream == "plain":
                for k, v in entropy_coding.decompress_state_dict(d, stream_name=stream).items():
                    res[f"decoded::{k}"] = v.numpy()
    np.savez_compressed(f"{OUT}/container_64x4_bits9.npz", **res)
    print("container bits 9: plain", res["plain_bytes"].size, "lzma", res["lzma_bytes"].size, "centroids", res["n_centroids"].tolist())


if __name__ == "__main__":
    main()
