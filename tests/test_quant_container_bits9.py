"""The compressed container at quant.bits=9 on the CPU: labels above 255 go out as uint16 (tests/golden/container_64x4_bits9.npz,
minted by the reference's own code: tests/golden/make_golden_quant9.py), and the rule at its edge."""
import json

import numpy as np
import pytest
import torch
from torch import nn

from implicit_image.models import registry
from implicit_image.pipeline import entropy_coding
from implicit_image.pipeline.quant import KmeansQuant


def _quantised_model(golden, bits):
    hot = golden("hot_64x4_256")
    torch.manual_seed(0)
    model = registry["siren"](depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30)
    off = 0
    with torch.no_grad():
        for p in model.parameters():
            n = p.numel()
            p.copy_(torch.tensor(hot["final"][off:off + n]).view(p.shape))
            off += n
        g = torch.Generator().manual_seed(11)
        model.layers[1].linear.weight.mul_((torch.rand(64, 64, generator=g) > 0.4).float())
    optim = torch.optim.Adam(model.parameters(), lr=3e-4)
    comp = KmeansQuant(model, optim, bits=bits, skip_ll=["layers.0.linear", "layers.3.linear"])
    comp.kmeans_modify_weights()
    comp.update_weights()
    return model


@pytest.mark.parametrize("stream", ["plain", "lzma"])
def test_bits9_container_bytes_and_meta_match_reference(golden, tmp_path, stream):
    d = golden("container_64x4_bits9")
    model = _quantised_model(golden, 9)
    counts = [model.layers[l].linear.centroids.numel() for l in (1, 2)]
    assert counts == d["n_centroids"].tolist() and min(counts) > 256               # both layers need more than a byte
    assert list(model.state_dict().keys()) == [str(k) for k in d["state_dict_keys"]]
    codebooks = {l: model.layers[l].linear.centroids.detach().half().numpy() for l in (1, 2)}
    labels = {l: model.layers[l].linear.labeled_weight.detach().numpy() for l in (1, 2)}
    size = entropy_coding.compress_state_dict(model.half(), tmp_path, stream_name=stream)
    data = np.frombuffer(open(tmp_path / "compressed_weights.data", "rb").read(), np.uint8)
    assert np.array_equal(data, d[f"{stream}_bytes"])                               # byte-exact stream
    meta_text = open(tmp_path / "meta_data.json").read()
    assert meta_text == str(d[f"{stream}_meta"])                                    # byte-exact metadata
    assert size == int(d[f"{stream}_reported_size"])
    meta = {m["name"]: m for m in json.loads(meta_text).values()}
    assert [meta[f"layers.{l}.linear.labeled_weight"]["dtype"] for l in (1, 2)] == ["uint16", "uint16"]
    dec = entropy_coding.decompress_state_dict(tmp_path, stream_name=stream)
    for k in dec:
        assert np.array_equal(dec[k].numpy(), d[f"decoded::{k}"])
    for l in (1, 2):                                                                # decompress gives centroids[labels]
        assert labels[l].max() > 255
        assert np.array_equal(dec[f"layers.{l}.linear.weight"].numpy(), codebooks[l][labels[l]].astype(np.float32))


class _OneLayer(nn.Module):
    """a Linear with frozen centroids / labels, as update_weights leaves it"""

    def __init__(self, labels, n_centroids):
        super().__init__()
        self.linear = nn.Linear(labels.shape[1], labels.shape[0])
        self.linear.centroids = nn.Parameter(torch.arange(n_centroids, dtype=torch.float32) / 8, requires_grad=False)
        self.linear.labeled_weight = nn.Parameter(labels, requires_grad=False)


@pytest.mark.parametrize("top,dtype", [(255, "uint8"), (256, "uint16"), (510, "uint16")])
def test_label_width_follows_the_largest_label(tmp_path, top, dtype):
    """255 still fits a byte; 256 does not (the reference writes uint8 there and the label wraps to 0: INTEGRATION.md §4)"""
    labels = (torch.arange(24, dtype=torch.int64) * 7 % (top + 1)).reshape(4, 6)
    labels[1, 2] = top
    model = _OneLayer(labels, top + 1)
    sd = entropy_coding.linear_state_dict(model)
    assert str(sd["linear.labeled_weight"].dtype) == "torch." + dtype and "linear.weight" not in sd
    entropy_coding.compress_state_dict(model, tmp_path, stream_name="plain")
    meta = {m["name"]: m for m in json.load(open(tmp_path / "meta_data.json")).values()}
    assert meta["linear.labeled_weight"]["dtype"] == dtype
    raw = open(tmp_path / "compressed_weights.data", "rb").read()
    width = 1 if dtype == "uint8" else 2
    assert len(raw) == 4 * (4 + top + 1) + 24 * width                               # bias, centroids (fp32), the labels
    stored = np.frombuffer(raw[-24 * width:], "<u%d" % width).reshape(4, 6)         # little-endian in the stream
    assert np.array_equal(stored, labels.numpy())
    dec = entropy_coding.decompress_state_dict(tmp_path, stream_name="plain")
    assert np.array_equal(dec["linear.weight"].numpy(), (labels.float() / 8).numpy())
