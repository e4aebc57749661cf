"""Feathermap (masking=Feathermap) host side, CPU only: the FeatherNet wrapper against reference-minted fixtures
(tests/golden/make_golden_feather.py), the config group, the fit entry's early refusals and the C ABI symbols."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "implicit-image-compression_amd")
SMALL = dict(depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30, outermost_linear=True)
YAML = dict(depth=8, hidden_size=128, first_omega_0=50, hidden_omega_0=30, outermost_linear=True)


def feather(seed=0, density=0.2, **kw):
    from implicit_image.models.siren import Siren
    from implicit_image.pipeline.feathermap import FeatherNet
    torch.manual_seed(seed)
    return FeatherNet(Siren(**kw), compress=density)


def test_init_is_bit_exact_with_the_reference(golden):
    g = golden("feather_init")
    m = feather(**SMALL)
    sd = m.state_dict()
    assert [k for k in g.files if k.startswith("small/") and k != "small/nm"] == ["small/" + k for k in sd]
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), g["small/" + k]), k
    assert [m._size_n, m._size_m, m.get_num_WandB()] == list(g["small/nm"])


def test_yaml_model_names_shapes_and_draws(golden):
    import hashlib
    g = golden("feather_init")
    m = feather(**YAML)
    sd = m.state_dict()
    assert list(sd) == list(g["yaml_names"])
    assert [n for n, _ in m.named_parameters()] == list(g["yaml_names"])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(g["yaml_shape/" + k]), k
        assert hashlib.sha256(np.ascontiguousarray(v.numpy()).tobytes()).hexdigest() == str(g["yaml_sha/" + k]), k
    assert [m._size_n, m._size_m, m.get_num_WandB()] == list(g["yaml/nm"])


@pytest.mark.parametrize("hidden,depth,P,n,m,stored", [
    (64, 4, 8707, 94, 10, 1888), (128, 8, 99843, 316, 32, 20240), (256, 8, 396291, 630, 63, 79396),
    (512, 8, 1579011, 1257, 126, 316780), (1024, 12, 10502147, 3241, 325, 2106674)])
def test_sizes_at_density_0p2(hidden, depth, P, n, m, stored):
    f = feather(depth=depth, hidden_size=hidden)
    assert (f.get_num_WandB(), f._size_n, f._size_m, f.num_stored()) == (P, n, m, stored)


def test_state_dict_round_trip_and_weight_tensors():
    a, b = feather(seed=0, **SMALL), feather(seed=1, **SMALL)
    b.load_state_dict(a.state_dict())
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    lin = a.module.layers[1].linear
    assert not isinstance(lin.weight, torch.nn.Parameter) and tuple(lin.weight.shape) == (64, 64)
    assert "weight" not in dict(lin.named_parameters()) and "weight_p" in dict(lin.named_parameters())


def test_mirror_matches_the_reference_gradients(golden):
    """the fp32 torch mirror the GPU tests compare against reproduces the reference's forward and autograd gradients"""
    from oracle import siren_oracle as so
    import _feather_ref as fr
    g = golden("feather_grads")
    H, W = 48, 40
    img, grid = so.synthetic_image(H, W, seed=5), so.get_grid(H, W)
    m = feather(**SMALL)
    pred, loss, grads = fr.loss_and_grads(list(m.parameters()), fr.shapes(64, 4), grid, img)
    assert float((pred - torch.tensor(g["small/pred"])).abs().max()) < 1e-5
    assert abs(loss - float(g["small/loss"])) / float(g["small/loss"]) < 1e-5
    for (n, _), gr in zip(m.named_parameters(), grads):
        ref = g[f"small/grad/{n}"]
        assert np.abs(gr.numpy() - ref).max() <= 1e-4 * max(np.abs(ref).max(), 1e-30), n


def test_config_group_composes():
    from implicit_image.config import load_config
    cfg = load_config(os.path.join(ROOT, "conf"), ["masking=Feathermap", "quant=none"])
    assert dict(cfg.masking) == {"name": "Feathermap", "dense": True, "density": 0.2, "print_FLOPs": False}
    assert not cfg.get("quant")


@pytest.mark.parametrize("extra,needle", [(["quant=kmeans"], "deepcopy"), (["quant=none", "mlp=fourier"], "mlp=siren")])
def test_fit_refuses_unsupported_combinations_before_any_device_work(extra, needle, monkeypatch):
    from implicit_image import fit
    from implicit_image.config import load_config
    cfg = load_config(os.path.join(ROOT, "conf"), ["masking=Feathermap"] + extra)
    monkeypatch.setattr(fit, "load_img", lambda **kw: pytest.fail("touched the image before refusing"))
    with pytest.raises(NotImplementedError, match=needle):
        fit.fit_one(cfg, torch.device("cpu"))


def test_deploy_and_deepcopy_raise_with_the_reason():
    import copy
    m = feather(**SMALL)
    with pytest.raises(NotImplementedError, match="deploy"):
        m.deploy()
    with pytest.raises(NotImplementedError, match="deepcopy"):
        copy.deepcopy(m)


def test_feather_symbols_are_declared_exported_and_guarded():
    from implicit_image import _engine
    hdr = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
    names = ["sf_feather_attach", "sf_feather_state_ptr", "sf_feather_materialise", "sf_feather_adjoint"]
    for n in names:
        assert n in _engine.exported_symbols()
        assert re.search(r"#define SF_ABI_VERSION 3\b", hdr)
    lib = os.path.join(PKG, "csrc", "libsiren_fit.so")
    if os.path.exists(lib):
        cdll = ctypes.CDLL(lib)
        assert all(hasattr(cdll, n) for n in names)
    src = open(os.path.join(PKG, "csrc", "feather_host.hip")).read()
    assert '#include "feather_host.hip"' in open(os.path.join(PKG, "csrc", "siren_fit.hip")).read()
    for n in names:   # every entry point is a function-try-block inside extern "C"
        assert re.search(n + r"\([^)]*\)\s*try\s*\{", src), n

    class Stale:   # a library built before the feather entry points: bindings are skipped, attach names the rebuild
        pass
    assert not _engine.has_feather(Stale())
