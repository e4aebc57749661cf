"""Host side of `make decode` without a GPU: PPM writer, container loading, decode.json, band planner, byte conversion,
and the render symbols of the built library."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE_OV = ["mlp.depth=4", "mlp.hidden_size=64", "mlp.first_omega_0=50", "mlp.hidden_omega_0=30"]


@pytest.mark.parametrize("hw", [(1, 1), (7, 5), (33, 64), (64, 33), (101, 3)])
def test_ppm_round_trip_is_exact(tmp_path, hw):
    from implicit_image.data import read_ppm, write_ppm
    g = torch.Generator().manual_seed(hw[0] * 131 + hw[1])
    x = torch.randint(0, 256, (*hw, 3), generator=g, dtype=torch.uint8)
    write_ppm(str(tmp_path / "x.ppm"), x)
    back = read_ppm(str(tmp_path / "x.ppm"))
    assert tuple(back.shape) == (*hw, 3) and torch.equal(back, x.int())
    write_ppm(str(tmp_path / "y.ppm"), x.numpy())                       # ndarray input
    assert open(tmp_path / "y.ppm", "rb").read() == open(tmp_path / "x.ppm", "rb").read()
    with pytest.raises(ValueError):
        write_ppm(str(tmp_path / "z.ppm"), x.float())


@pytest.mark.parametrize("stream", ["plain", "lzma"])
def test_container_fixture_loads_to_the_reference_state_dict(golden, tmp_path, stream):
    """the reference-minted container bytes -> decode's loading code -> exactly the fixture's decoded tensors"""
    from implicit_image import decode as dec
    d = golden("container_64x4")
    q = tmp_path / "model_quantized"
    q.mkdir()
    (q / "compressed_weights.data").write_bytes(d[f"{stream}_bytes"].tobytes())
    (q / "meta_data.json").write_text(str(d[f"{stream}_meta"]))
    shape = dec.resolve_shape(str(tmp_path), SHAPE_OV + [f"entropy_coding={stream}"])
    sd, used = dec.load_weights(str(tmp_path), shape)
    assert used == "container"
    want = [k[len("decoded::"):] for k in d.files if k.startswith("decoded::")]
    assert sorted(sd.keys()) == sorted(want)
    dense = [str(k) for k in d["state_dict_keys"] if "centroids" not in str(k) and "labeled_weight" not in str(k)]
    assert sorted(sd.keys()) == sorted(dense)
    for k in want:
        assert sd[k].dtype == torch.float32 and np.array_equal(sd[k].numpy(), d[f"decoded::{k}"]), k
    assert dec.flat_params(sd, 4).numel() == 2 * 64 + 64 + 2 * (64 * 64 + 64) + 64 * 3 + 3
    assert dec.render_path(shape)[0] == "kernel"
    with pytest.raises(FileNotFoundError):
        dec.load_weights(str(tmp_path), shape, "pth")


def test_decode_json_round_trip_overrides_and_missing_file(tmp_path):
    from implicit_image import decode as dec
    from implicit_image.config import load_config
    cfg = load_config(os.path.join(ROOT, "conf"), ["mlp.hidden_size=64", "mlp.depth=4", "img.height=48", "img.width=40",
                                                   "masking=Small_Dense", "masking.density=0.25", "entropy_coding=lzma"])
    keys = ["layers.0.linear.weight", "layers.0.linear.bias"]
    path = dec.write_decode_json(str(tmp_path), cfg, keys)
    assert os.path.basename(path) == "decode.json"
    shape = dec.resolve_shape(str(tmp_path))
    assert dict(shape.mlp) == dict(cfg.mlp)
    assert (shape.img.height, shape.img.width) == (48, 40)
    assert shape.entropy_coding.stream_name == "lzma" and shape.small_dense_density == 0.25
    assert shape.state_dict_keys == keys
    assert dec.engine_width(shape) == 32 and dec.render_path(shape)[0] == "kernel"      # int(64 * sqrt(0.25))
    # overrides win
    over = dec.resolve_shape(str(tmp_path), ["mlp.hidden_size=512", "mlp.depth=5", "entropy_coding=plain"])
    assert over.mlp.hidden_size == 512 and over.mlp.depth == 5 and over.mlp.first_omega_0 == cfg.mlp.first_omega_0
    assert over.entropy_coding.stream_name == "plain"
    assert dec.render_path(dec.resolve_shape(str(tmp_path), ["masking=none", "mlp.hidden_size=512"]))[0] == "torch"
    assert dec.render_path(dec.resolve_shape(str(tmp_path), ["mlp=fourier"]))[0] == "torch"
    # a missing file plus overrides works; without them the message names the keys
    empty = tmp_path / "old"
    empty.mkdir()
    old = dec.resolve_shape(str(empty), SHAPE_OV + ["img.height=64", "img.width=64"])
    assert (old.mlp.name, old.mlp.depth, old.mlp.hidden_size, old.img.height) == ("siren", 4, 64, 64)
    with pytest.raises(FileNotFoundError) as e:
        dec.resolve_shape(str(empty), ["mlp.depth=4"])
    assert "mlp.hidden_size" in str(e.value) and "mlp.depth=" not in str(e.value).split("pass ")[1].split("(")[0]
    with pytest.raises(FileNotFoundError) as e:
        dec.resolve_shape(str(empty))
    assert "mlp.depth" in str(e.value) and "mlp.hidden_size" in str(e.value)
    # a Feathermap run says what it cannot do
    cfg_f = load_config(os.path.join(ROOT, "conf"), ["masking=Feathermap", "quant=none"])
    fdir = tmp_path / "feather"
    fdir.mkdir()
    dec.write_decode_json(str(fdir), cfg_f, keys)
    with pytest.raises(NotImplementedError) as e:
        dec.load_weights(str(fdir), dec.resolve_shape(str(fdir)))
    assert "Feathermap" in str(e.value)


@pytest.mark.parametrize("hw", [(1, 1), (64, 64), (4096, 4096), (8192, 8192), (20000, 12345), (32768, 32768), (5, 32768)])
@pytest.mark.parametrize("band_rows", [None, 7])
def test_band_planner(hw, band_rows):
    from implicit_image.decode import BAND_BYTES, plan_bands
    H, W = hw
    bands = plan_bands(H, W, 3, band_rows)
    assert bands[0][0] == 0 and bands[-1][1] == H
    for (a, b), (c, _) in zip(bands, bands[1:] + [(H, H)]):
        assert a < b and b == c                                          # contiguous, disjoint, non-empty
    for a, b in bands:
        assert (b - a) * W * W < 2 ** 40
        assert (b - a) * W * 3 < BAND_BYTES
        if band_rows:
            assert b - a <= band_rows
    if band_rows is None and H * W * 3 < BAND_BYTES and H * W * W < 2 ** 40:
        assert bands == [(0, H)]


def test_byte_conversion_helper():
    from implicit_image.decode import to_u8
    k = torch.arange(0, 256, dtype=torch.float32) / 255
    x = torch.cat([torch.tensor([-3.0, -1e-3, -0.0, 0.0, 0.999999, 1.0, 1.0000001, 1.5, 7.0, 1e12, -1e12, 0.5]), k,
                   torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-1.0))])
    prod = (x * 255.0).double()                                           # the fp32 product, then exact arithmetic
    want = torch.minimum(torch.maximum(torch.trunc(prod), torch.tensor(0.0, dtype=torch.float64)),
                         torch.tensor(255.0, dtype=torch.float64)).to(torch.uint8)
    got = to_u8(x)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    inside = (x >= 0) & (x <= 1)
    assert torch.equal(got[inside].int(), (x[inside] * 255).int())        # eval_epoch's (pred * 255).int() where it applies


def test_render_symbols_are_declared_and_exported():
    from implicit_image import _engine
    syms = _engine.exported_symbols()
    assert "sf_render_create" in syms and "sf_render" in syms
    hdr = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
    assert "int sf_render_create(const sf_config* cfg, sf_handle** out);" in hdr
    assert "int sf_render(sf_handle* h, uint8_t* rgb8_dev, float* pred_dev);" in hdr
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "implicit-image-compression_amd", "csrc"), "libsiren_fit.so"],
                          stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(_engine._LIB_PATH)
    assert hasattr(lib, "sf_render_create") and hasattr(lib, "sf_render")
    assert _engine.has_render(_engine.load_library())
    assert lib.sf_abi_version() == 3
