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


# ---- the torch mirror (tests/_fourier_ref.py) against the reference, and the engine's numerics model against fp64 ----
SMALL = dict(depth=4, hidden_size=64, map_size=128, map_scale=10.0)
YAML = dict(depth=8, hidden_size=128, map_size=256, map_scale=16.0)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _fourier(seed=0, **kw):
    torch.manual_seed(seed)
    return registry["fourier"](**kw)


def _flat(m):
    """flat engine-layout parameters of a host FourierNet (its logical width) and the layer dims"""
    import _fourier_ref as fr
    flat = torch.cat([p.detach().reshape(-1) for p in m._param_list()])
    return flat, fr.layer_dims(m.cfg["n_linear"], m.cfg["hidden_size"], m.cfg["map_size"])


def test_fp32_mirror_reproduces_the_reference_grads_fixture(golden):
    """The mirror the GPU tests use is the reference's arithmetic: on the 48x40 fixture grid it reproduces
    fourier_grads.npz (measured: bit-identical with 8 torch threads; the bars leave room for another thread count's
    summation order)."""
    import _fourier_ref as fr
    from oracle import siren_oracle as so
    g = golden("fourier_grads")
    H, W = 48, 40
    img, grid = so.synthetic_image(H, W, seed=5), so.get_grid(H, W)
    for tag, kw in (("small", SMALL), ("yaml", YAML)):
        m = _fourier(**kw)
        pred, loss, grads = fr.loss_and_grads(m, grid, img)
        assert pred.dtype == torch.float32
        assert (pred - torch.tensor(g[f"{tag}/pred"])).abs().max().item() <= 1e-6, tag
        assert abs(loss - float(g[f"{tag}/loss"])) <= 1e-6 * float(g[f"{tag}/loss"]), tag
        names = [n for n, p in m.named_parameters() if p.requires_grad]
        assert len(names) == len(grads) == 2 * m.cfg["n_linear"]
        for n, gr in zip(names, grads):
            if tag == "small":
                assert _rel(gr, g[f"small/grad/{n}"]) <= 1e-5, n
            else:
                ref = float(g[f"yaml/gradnorm/{n}"])
                assert abs(gr.double().norm().item() - ref) <= 1e-5 * ref, n


def test_engine_model_sits_at_the_fp16_gap_from_fp64(golden):
    """engine_model_loss_and_grads (fourier_kernels.hip's rounding points, fp64 elsewhere) against the fp64 mirror at the
    two fixture models.  Measured: prediction 3.3e-5 / 5.5e-6 max abs, SSE 1.4e-6 / 3.7e-8 relative, per-tensor gradient
    max |err| / max |ref| up to 0.0146 (small, layers.2.weight: the measured engine-vs-reference value of
    test_gpu_fourier.py) / 0.050 (yaml).  Both sides are bounded: a model that lost its fp16 roundings would sit near 0,
    one with a wrong rounding point far above."""
    import _fourier_ref as fr
    from oracle import siren_oracle as so
    H, W = 48, 40
    img, grid = so.synthetic_image(H, W, seed=5), so.get_grid(H, W)
    for tag, kw, gbar in (("small", SMALL, 3e-2), ("yaml", YAML, 0.1)):
        m = _fourier(**kw)
        flat, dims = _flat(m)
        p64, l64, g64 = fr.flat_loss_and_grads(m.encoding.B, flat, dims, grid, img)
        pm, sm, gm = fr.engine_model_loss_and_grads(m.encoding.B, flat, dims, grid, img)
        assert pm.dtype == g64.dtype == gm.dtype == torch.float64
        assert 1e-7 < (pm - p64).abs().max().item() < 1e-4, tag
        assert abs(sm / (3 * H * W) - l64) < 1e-5 * l64, tag
        worst = 0.0
        for (wm, bm), (w64, b64) in zip(fr.split_flat(gm, dims), fr.split_flat(g64, dims)):
            for a, b in ((wm, w64), (bm, b64)):
                e = _rel(a, b)
                assert e < gbar, (tag, e)
                worst = max(worst, e)
        assert worst > 1e-3, (tag, worst)


def test_engine_model_restates_the_fp32_mirror_without_rounding():
    """With every fp16 rounding point turned into the identity, the model is the fp64 mirror: what separates the two is
    the rounding points and nothing else (no stray scale, transpose or mask)."""
    import _fourier_ref as fr
    from oracle import siren_oracle as so
    H, W = 12, 10
    img, grid = so.synthetic_image(H, W, seed=5), so.get_grid(H, W)
    m = _fourier(**SMALL)
    flat, dims = _flat(m)
    p64, l64, g64 = fr.flat_loss_and_grads(m.encoding.B, flat, dims, grid, img)
    keep = fr._f16
    fr._f16 = lambda x: x.double()
    try:
        pm, sm, gm = fr.engine_model_loss_and_grads(m.encoding.B, flat, dims, grid, img)
    finally:
        fr._f16 = keep
    # (left: the fp32 phase t, whose rounding moves features by ~1e-6 at map_scale 10)
    assert (pm - p64).abs().max().item() < 1e-6
    assert abs(sm / (3 * H * W) - l64) < 1e-6 * l64
    assert _rel(gm, g64) < 1e-5


@pytest.fixture(scope="module")
def shapes_fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "fourier_shapes.npz"), allow_pickle=False)


def _shape_kw():
    import _fourier_shapes_child as ch
    return ch.SHAPES


def test_shapes_fixture_covers_the_gpu_matrix(shapes_fixture):
    assert [str(t) for t in shapes_fixture["tags"]] == list(_shape_kw())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "fourier_shapes.npz")) < 256 * 1024


@pytest.mark.parametrize("tag", ["h32_m64_d3", "h45p_m512_d13", "h128_m512_d4", "h256_m256_d4", "h256_m512_d8",
                                 "h198p_m64_d5"])
def test_shapes_init_and_fp32_mirror_match_the_reference(shapes_fixture, tag):
    """Seed-0 init at every shape of the GPU matrix is bit-exact against the reference (sha256 per tensor: the draw
    order at widths 32 / 256, map 64 / 512, 2 and 12 Linear layers, Small_Dense widths 45 and 198); the fp32 mirror
    reproduces the reference's prediction, loss and per-tensor gradient norms there (measured: bit-identical)."""
    import _fourier_ref as fr
    from oracle import siren_oracle as so
    g, kw = shapes_fixture, _shape_kw()[tag]
    m = _fourier(**kw)
    sd = m.state_dict()
    assert list(sd) == [str(n) for n in g[f"{tag}/names"]]
    for k, v in sd.items():
        assert hashlib.sha256(v.numpy().astype(np.float32).tobytes()).hexdigest() == str(g[f"{tag}/sha/{k}"]), (tag, k)
    H, W = 24, 20
    img, grid = so.synthetic_image(H, W, seed=5), so.get_grid(H, W)
    pred, loss, grads = fr.loss_and_grads(m, grid, img)
    assert (pred - torch.tensor(g[f"{tag}/pred"])).abs().max().item() <= 1e-6
    assert abs(loss - float(g[f"{tag}/loss"])) <= 1e-6 * float(g[f"{tag}/loss"])
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    for n, gr in zip(names, grads):
        ref = float(g[f"{tag}/gradnorm/{n}"])
        assert abs(gr.double().norm().item() - ref) <= 1e-5 * ref, (tag, n)
