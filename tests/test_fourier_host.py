"""FourierNet (mlp=fourier) host side, no GPU needed: registry, the reference's init / names / draw order, the yaml load
path, masking rules and the C ABI's validation of sf_fourier_create."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from implicit_image import _engine
from implicit_image.models import registry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registry_has_fourier():
    assert "fourier" in registry and registry["fourier"].__name__ == "FourierNet"


def test_init_is_bit_exact_against_the_reference(golden):
    g = golden("fourier_init")
    torch.manual_seed(0)
    m = registry["fourier"](depth=4, hidden_size=64, map_size=128, map_scale=10.0)
    sd = m.state_dict()
    small = [k[len("small/"):] for k in g.files if k.startswith("small/")]
    assert list(sd) == small == ["encoding.B", "layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias",
                                 "layers.4.weight", "layers.4.bias"]
    for k in small:
        assert np.array_equal(sd[k].numpy(), g["small/" + k]), k
    assert not m.encoding.B.requires_grad
    assert [n for n, p in m.named_parameters() if p.requires_grad] == small[1:]
    torch.manual_seed(0)
    y = registry["fourier"](depth=8, hidden_size=128, map_size=256, map_scale=16.0)
    assert list(y.state_dict()) == [str(n) for n in g["yaml_names"]]
    for k, v in y.state_dict().items():
        assert tuple(v.shape) == tuple(g["yaml_shape/" + k]), k
        assert hashlib.sha256(v.numpy().astype(np.float32).tobytes()).hexdigest() == str(g["yaml_sha/" + k]), k
    assert y.cfg["n_linear"] == 7 and y._engine_width == 128 and not y._padded


def test_yaml_load_path_and_small_dense_width():
    from implicit_image.config import load_config
    cfg = load_config(os.path.join(ROOT, "conf"), ["mlp=fourier", "masking=Small_Dense", "masking.density=0.5"])
    assert dict(cfg.mlp) == {"name": "fourier", "depth": 8, "hidden_size": 128, "map_size": 256, "map_scale": 16}
    m = registry[cfg.mlp.name](**cfg.mlp, small_dense_density=cfg.masking.density, **dict(cfg.engine))
    assert m.cfg["hidden_size"] == 90 and m._engine_width == 128 and m._padded
    assert m.layers[0].weight.shape == (90, 256) and m.encoding.B.shape == (2, 128)
    with pytest.raises(NotImplementedError):
        registry["fourier"](hidden_size=512)
    with pytest.raises(NotImplementedError):
        registry["fourier"](compute_dtype="bf16")


def test_setup_mask_rejects_mask_modes_and_accepts_dense():
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, setup_mask
    m = registry["fourier"](depth=4, hidden_size=64, map_size=128)
    optim, _ = get_optimizer_lr_scheduler(m, dict(name="adam", lr=1e-3))
    rigl = dict(name="RigL", density=0.2, sparse_init="erdos-renyi-kernel", dense_gradients=False, growth_mode="gradient",
                prune_mode="magnitude", redistribution_mode="none", dense=False, prune_rate=0.3, decay_schedule="cosine",
                end_when=100, interval=10)
    with pytest.raises(NotImplementedError, match="encoding.B"):
        setup_mask(m, optim, rigl)
    assert setup_mask(m, optim, dict(name="Small_Dense", dense=True, density=0.5)) is None
    assert setup_mask(m, optim, None) is None


def test_abi_exports_the_fourier_entry_points():
    lib = _engine.load_library()
    assert lib.sf_abi_version() == _engine.SF_ABI_VERSION == 3
    syms = _engine.exported_symbols()
    for s in ("sf_fourier_create", "sf_set_encoding"):
        assert s in syms and hasattr(lib, s)


def _cfg(**kw):
    base = dict(abi_version=_engine.SF_ABI_VERSION, height=16, width=16, in_features=2, out_features=3, map_size=256,
                hidden=128, n_linear=7, compute_dtype=1, beta1=0.9, beta2=0.999, eps=1e-8, device=0, stream=None,
                chunk_pixels=0)
    base.update(kw)
    return _engine.sf_fourier_config(**base)


@pytest.mark.parametrize("bad", [dict(abi_version=2), dict(hidden=96), dict(hidden=512), dict(map_size=100),
                                 dict(map_size=1024), dict(n_linear=1), dict(n_linear=13), dict(out_features=1),
                                 dict(in_features=3), dict(compute_dtype=0), dict(height=0), dict(chunk_pixels=-1)])
def test_fourier_create_rejects_bad_configs_without_a_gpu(bad):
    lib = _engine.load_library()
    h = C.c_void_p()
    assert lib.sf_fourier_create(C.byref(_cfg(**bad)), C.byref(h)) == -1
    assert lib.sf_last_error() and not h.value


def test_set_encoding_and_debug_scratch_need_a_handle():
    lib = _engine.load_library()
    assert lib.sf_set_encoding(None, None) == -1
    assert lib.sf_fourier_create(None, None) == -1
