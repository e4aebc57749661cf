"""Host side of the Feathermap render path, no GPU needed: the two C ABI entry points (header, prototype table, built
library, null-handle refusals), the geometry the decoder hands sf_feather_render_attach, the feather vector read back from a
saved run, and the refusals that stay as they were."""
import ctypes as C
import json
import os
import re
from math import ceil

import pytest
import torch

from implicit_image import _engine
from implicit_image import decode as dec
from implicit_image.config import _wrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
NAMES = ["sf_feather_render_attach", "sf_feather_render_load"]

# hidden, depth, density, P, n, m, engine width
SHAPES = [(32, 2, 0.2, 195, 14, 2, 32), (64, 4, 0.2, 8707, 94, 10, 64), (96, 3, 0.5, 9891, 100, 25, 128),
          (128, 8, 0.2, 99843, 316, 32, 128), (256, 3, 0.1, 67331, 260, 13, 256)]


def mlp_of(hidden, depth):
    return dict(name="siren", depth=depth, hidden_size=hidden, first_omega_0=50, hidden_omega_0=30, outermost_linear=True)


def shape_of(hidden, depth, keys=None, H=64, W=64):
    return _wrap({"mlp": mlp_of(hidden, depth), "img": {"height": H, "width": W}, "engine": {}, "entropy_coding": {},
                  "masking_name": "Feathermap", "small_dense_density": None, "state_dict_keys": keys})


def feather(hidden, depth, density, seed=0):
    from implicit_image.models.siren import Siren
    from implicit_image.pipeline.feathermap import FeatherNet
    torch.manual_seed(seed)
    return FeatherNet(Siren(**{k: v for k, v in mlp_of(hidden, depth).items() if k != "name"}), compress=density)


def save_run(tmp_path, net, hidden, depth, edit=None):
    """a run directory as `fit` leaves it: model.pth and decode.json; edit(sd) changes the saved tensors"""
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    keys = list(sd)
    if edit:
        edit(sd)
    run = str(tmp_path)
    torch.save({"state_dict": sd}, os.path.join(run, "model.pth"))
    cfg = _wrap({"mlp": mlp_of(hidden, depth), "img": {"height": 64, "width": 64}, "entropy_coding": {}, "engine": {},
                 "masking": {"name": "Feathermap", "density": 0.2}})
    dec.write_decode_json(run, cfg, keys)
    return run


def test_symbols_in_header_table_and_library():
    for n in NAMES:
        assert n in _engine.exported_symbols()
        assert _engine.PROTOTYPES[n][0] == "feather" and _engine.PROTOTYPES[n][2] is C.c_int
    assert re.search(r"int sf_feather_render_attach\(sf_handle\* h, int64_t n, int64_t m, int32_t n_layers,\s*"
                     r"const int32_t\* logical_out,\s*const int32_t\* logical_in\);", HEADER)
    assert re.search(r"int sf_feather_render_load\(sf_handle\* h, const float\* feather_dev", HEADER)
    assert re.search(r"#define SF_ABI_VERSION 3\b", HEADER) and _engine.SF_ABI_VERSION == 3
    assert len(re.findall(r"typedef struct (sf_\w*config) \{", HEADER)) == 4          # no new config struct
    lib = _engine.load_library()
    assert _engine.has_feather(lib)
    li = (C.c_int32 * 2)(32, 3)
    assert lib.sf_feather_render_attach(None, 14, 2, 2, li, li) == -1 and lib.sf_last_error()
    assert lib.sf_feather_render_load(None, None) == -1 and lib.sf_last_error()
    assert issubclass(_engine.FeatherRenderEngine, _engine.RenderEngine)
    assert callable(_engine.FeatherRenderEngine.load_feather)


@pytest.mark.parametrize("hidden,depth,density,P,n,m,width", SHAPES)
def test_geometry_of_a_feathernet_state_dict(hidden, depth, density, P, n, m, width):
    net = feather(hidden, depth, density)
    assert (net.get_num_WandB(), net._size_n, net._size_m) == (P, n, m)
    shape = shape_of(hidden, depth)
    sd = net.state_dict()
    assert list(sd) == dec.feather_keys(depth)
    gn, gm, outs, ins = dec.feather_geometry(shape, sd)
    assert (gn, gm) == (n, m)
    assert outs == [hidden] * (depth - 1) + [3] and ins == [2] + [hidden] * (depth - 1)
    assert sum(o * i + o for o, i in zip(outs, ins)) == P
    assert dec.padded_width(shape) == width
    assert dec.render_path(shape) == ("kernel", f"Feathermap {width}x{depth}" + (f" (width {hidden} zero-padded)" if width != hidden else "")
                                      + ": sf_feather_render_load + sf_render")
    c = (2 * m - 1) / n                                  # the compress the torch path rebuilds the net with
    assert ceil(c * n / 2) == m
    again = dec.feather_model(sd, shape)
    assert (again._size_n, again._size_m) == (n, m)
    for (ka, va), (kb, vb) in zip(sd.items(), again.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


def test_load_feather_round_trip_and_flat_order(tmp_path):
    net = feather(64, 4, 0.2)
    run = save_run(tmp_path, net, 64, 4)
    shape = dec.resolve_shape(run)
    assert dec.is_feather(shape)
    sd = dec.load_feather(run, shape)
    assert list(sd) == [k for k, _ in net.named_parameters()]
    for k, v in net.state_dict().items():
        assert sd[k].dtype == torch.float32 and sd[k].device.type == "cpu" and torch.equal(sd[k], v)
    flat = dec.feather_flat(sd, 4)
    assert flat.dtype == torch.float32 and flat.numel() == 2 * 94 * 10 + 8 == net.num_stored()
    assert torch.equal(flat, torch.cat([p.detach().reshape(-1) for _, p in net.named_parameters()]))
    assert dec.feather_geometry(shape, sd) == (94, 10, [64, 64, 64, 3], [2, 64, 64, 64])


def test_load_feather_errors_name_the_tensor(tmp_path):
    net = feather(64, 4, 0.2)
    a, b, c = (tmp_path / x for x in "abc")
    for d in (a, b, c):
        d.mkdir()

    def transpose(sd):
        sd["_V2"] = sd["_V2"].t().contiguous()
    run = save_run(a, net, 64, 4, transpose)
    with pytest.raises(ValueError, match="_V2"):
        dec.load_feather(run, dec.resolve_shape(run))
    run = save_run(b, net, 64, 4, lambda sd: sd.pop("module.layers.2.linear.bias_p"))
    with pytest.raises(ValueError, match=r"module\.layers\.2\.linear\.bias_p"):
        dec.load_feather(run, dec.resolve_shape(run))
    run = save_run(c, net, 64, 4)
    with pytest.raises(FileNotFoundError, match="Feathermap run has no container"):
        dec.load_feather(run, dec.resolve_shape(run), "container")
    with pytest.raises(ValueError, match="_V1"):        # the vector of another network: n is not ceil(sqrt(P))
        dec.feather_geometry(shape_of(32, 2), dec.load_feather(run, dec.resolve_shape(run)))


def test_existing_refusals_stay(tmp_path, monkeypatch):
    run = save_run(tmp_path, feather(64, 4, 0.2), 64, 4)
    with pytest.raises(NotImplementedError, match="saves no deployable weights"):
        dec.load_weights(run, dec.resolve_shape(run))
    # a wide Feathermap run under decode.render=kernel: choose_path's refusal, before a file is read or a device touched
    monkeypatch.setattr(dec, "load_feather", lambda *a, **k: pytest.fail("read a file before refusing"))
    monkeypatch.setattr(dec, "load_weights", lambda *a, **k: pytest.fail("read a file before refusing"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("asked for the device before refusing"))
    with pytest.raises(ValueError, match=r"decode.render=kernel: SIREN width 512 is on the wide path"):
        dec.decode([f"decode.dir={run}", "decode.render=kernel", "mlp.hidden_size=512"])
    assert json.load(open(os.path.join(run, "decode.json")))["masking_name"] == "Feathermap"
