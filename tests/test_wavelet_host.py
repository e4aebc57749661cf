"""WaveletSiren (mlp=wavelet_siren) host side, no GPU needed: registry, the reference's init / names / draw order, the
library stand-ins and the fp64 mirror against PyWavelets / torch / reference-minted fixtures, the refusals, and the C ABI
of sf_wavelet_create."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from implicit_image import _engine
from implicit_image.models import registry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(depth=4, hidden_size=64, first_omega_0=50.0, hidden_omega_0=30.0)
YAML = dict(depth=8, hidden_size=128, wavelet_levels=1, first_omega_0=50.0, hidden_omega_0=30.0, outermost_linear=True,
            simulate_quantization=False)


def _wavelet(seed=0, **kw):
    torch.manual_seed(seed)
    return registry["wavelet_siren"](**kw)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_registry_has_wavelet_siren():
    assert "wavelet_siren" in registry and registry["wavelet_siren"].__name__ == "WaveletSiren"


def test_init_names_and_draw_order_are_bit_exact_against_the_reference(golden):
    g = golden("wavelet_init")
    m = _wavelet(**SMALL)
    names = [n for n, _ in m.named_parameters()]
    assert names == [str(n) for n in g["small_names"]]
    assert names[0] == "LF_siren.layers.0.linear.weight" and names[-1] == "HF_siren.layers.3.linear.bias"
    assert list(m.state_dict()) == names
    for n, p in m.named_parameters():
        assert np.array_equal(p.detach().numpy(), g["small/" + n]), n
    y = _wavelet(**YAML)
    assert [n for n, _ in y.named_parameters()] == [str(n) for n in g["yaml_names"]]
    for n, p in y.named_parameters():
        assert tuple(p.shape) == tuple(g["yaml_shape/" + n]), n
        assert hashlib.sha256(p.detach().numpy().astype(np.float32).tobytes()).hexdigest() == str(g["yaml_sha/" + n]), n
    assert y._engine_width == 128 and not y._padded and y.cfg["scratch_format"] == 16


def test_first_forward_repeats_the_reference_generator_draw(golden):
    """the reference's first forward draws torch.rand(1, 1, H, W) for its DWT shape probe (wavelet_siren.py:70-71)"""
    m = _wavelet(**SMALL)
    m.shape_probe(64, 64)
    assert m.LF_h == m.LF_w == 34
    assert np.array_equal(torch.rand(8).numpy(), golden("wavelet_init")["draws_after_forward"])
    m.shape_probe(64, 64)   # cached: no second draw
    torch.manual_seed(1)
    a = torch.rand(1)
    torch.manual_seed(1)
    m.shape_probe(64, 64)
    assert torch.equal(torch.rand(1), a)


def test_stub_idwt_and_mirror_match_pywavelets(golden):
    import _wavelet_ref as wr
    g = golden("wavelet_idwt")
    assert np.array_equal(np.float64(wr.REC_LO), g["rec_lo"]) and np.array_equal(np.float64(wr.REC_HI), g["rec_hi"])
    wr.install_stubs()
    from pytorch_wavelets import DWTInverse
    inv = DWTInverse(mode="zero", wave="db3")
    for n in g["ns"]:
        c = [torch.tensor(g[f"n{n}/{k}"]) for k in ("cA", "cH", "cV", "cD")]
        ref = g[f"n{n}/y"]
        assert ref.shape == (2 * n - 4, 2 * n - 4)
        y32 = inv((c[0][None, None], [torch.stack(c[1:], 0)[None, None]]))[0, 0]          # fp32, the reference's dtype
        assert y32.dtype == torch.float32 and _rel(y32, ref) < 1e-5, n
        y64 = wr.idwt(c[0].double()[None, None], torch.stack(c[1:], 0).double()[None, None])[0, 0]
        assert _rel(y64, ref) < (1e-6 if ref.dtype == np.float32 else 1e-12), n
    # band order: pytorch_wavelets' (LH, HL, HH) are pywt's (cH, cV, cD)
    for i, band in enumerate(("cH", "cV", "cD")):
        highs = torch.zeros(1, 1, 3, 6, 6, dtype=torch.float64)
        highs[0, 0, i] = torch.tensor(g[f"band_{band}/in"])
        y = wr.idwt(torch.zeros(1, 1, 6, 6, dtype=torch.float64), highs)[0, 0]
        assert _rel(y, g[f"band_{band}/y"]) < 1e-12, band


def test_bilinear_fixture_is_torch_interpolate_with_the_reference_scale(golden):
    import _wavelet_ref as wr
    g = golden("wavelet_bilinear")
    for H in g["Hs"]:
        H = int(H)
        n = wr.coeff_len(H)
        assert int(np.floor(n * (H / n))) == H
        x = torch.rand(1, 2, n, n, generator=torch.Generator().manual_seed(H))
        rows = g[f"H{H}/rows"]
        y = F.interpolate(x, scale_factor=H / n, mode="bilinear", align_corners=False)[0][:, rows]
        assert np.array_equal(y.numpy(), g[f"H{H}/y"]), H
        y64 = F.interpolate(x.double(), scale_factor=H / n, mode="bilinear", align_corners=False)[0][:, rows]
        # (fp64 against fp32: torch forms the source index and the weights in the input's type; measured 4.8e-6 at H 100)
        assert _rel(y64, g[f"H{H}/y"]) < 2e-5, H


def test_fp64_mirror_reproduces_the_reference_grads_fixture(golden):
    """the mirror the GPU tests use, loaded with the seed-0 init, is the reference's arithmetic (fp32 reference vs fp64)"""
    import _wavelet_ref as wr
    from oracle import siren_oracle as so
    g = golden("wavelet_grads")
    H = 64
    img = so.synthetic_image(H, H, seed=5)
    for tag, kw in (("small", SMALL), ("yaml", YAML)):
        m = _wavelet(**kw)
        flat = wr.model_flat(m)
        pred, loss, grad = wr.loss_and_grads(flat, m.cfg["hidden_size"], m.cfg["depth"], img, 50.0, 30.0)
        assert _rel(pred, g[f"{tag}/pred"]) < 1e-5, tag
        assert abs(loss - float(g[f"{tag}/loss"])) < 1e-5 * float(g[f"{tag}/loss"]), tag
        off = 0
        for n, p in m.named_parameters():
            gr = grad[off:off + p.numel()].view(p.shape)
            off += p.numel()
            if tag == "small":
                assert _rel(gr, g[f"small/grad/{n}"]) < 1e-4, n
            else:
                ref = float(g[f"yaml/gradnorm/{n}"])
                assert abs(gr.norm().item() - ref) < 1e-4 * ref, n


def test_plateau_fixture_holds_the_reference_spread(golden):
    g = golden("wavelet_plateau")
    for name in ("synthetic", "nonsmooth"):
        a, b = float(g[f"{name}/t8/psnr"]), float(g[f"{name}/t2/psnr"])
        assert 20 < a < 60 and abs(a - b) < 0.05, (name, a, b)
        assert g[f"{name}/t8/losses"].shape == (300,)


def test_refusals_raise_with_their_reason():
    with pytest.raises(NotImplementedError, match="wavelet_levels"):
        registry["wavelet_siren"](wavelet_levels=2)
    with pytest.raises(NotImplementedError, match="> 256"):
        registry["wavelet_siren"](hidden_size=512)
    with pytest.raises(NotImplementedError, match="scratch format 16"):
        registry["wavelet_siren"](scratch_format=8)
    with pytest.raises(NotImplementedError, match="fp16"):
        registry["wavelet_siren"](compute_dtype="bf16")
    m = registry["wavelet_siren"](**SMALL)
    from oracle import siren_oracle as so
    for shape in ((64, 48), (63, 63)):
        with pytest.raises(NotImplementedError, match="even, square"):
            m.engine(so.get_grid(*shape))
    with pytest.raises(NotImplementedError, match="pixel-split"):
        m.engine(so.get_grid(64, 64), row_begin=0, row_end=32)
    assert m.LF_h is None   # a refused call draws nothing and caches nothing
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, setup_mask
    optim, _ = get_optimizer_lr_scheduler(m, dict(name="adam", lr=1e-3))
    rigl = dict(name="RigL", density=0.2, sparse_init="erdos-renyi-kernel", dense_gradients=False, growth_mode="gradient",
                prune_mode="magnitude", redistribution_mode="none", dense=False, prune_rate=0.3, decay_schedule="cosine",
                end_when=100, interval=10)
    with pytest.raises(NotImplementedError, match="1x1 forward"):
        setup_mask(m, optim, rigl)
    assert setup_mask(m, optim, dict(name="Small_Dense", dense=True, density=0.5)) is None


@pytest.mark.parametrize("over, reason", [(["masking=Feathermap"], "SIREN engine only"),
                                          (["masking=none", "quant=kmeans"], "quant=KMeans on WaveletSiren"),
                                          (["masking=none", "quant=none", "img.height=64", "img.width=48"], "even, square"),
                                          (["masking=none", "quant=none", "img.height=63", "img.width=63"], "even, square"),
                                          (["masking=RigL", "quant=none", "img.height=64", "img.width=64"], "1x1 forward")])
def test_fit_refuses_before_any_gpu_work(over, reason):
    from implicit_image.config import load_config
    from implicit_image.fit import fit_one
    cfg = load_config(os.path.join(ROOT, "conf"), ["mlp=wavelet_siren"] + over)
    with pytest.raises(NotImplementedError, match=reason):
        fit_one(cfg, torch.device("cpu"))


def test_yaml_load_path_and_small_dense_width():
    from implicit_image.config import load_config
    cfg = load_config(os.path.join(ROOT, "conf"), ["mlp=wavelet_siren", "masking=Small_Dense", "masking.density=0.5"])
    assert dict(cfg.mlp) == {"name": "wavelet_siren", "depth": 8, "hidden_size": 128, "wavelet_levels": 1,
                             "first_omega_0": 50, "hidden_omega_0": 30, "outermost_linear": True,
                             "simulate_quantization": False}
    m = registry[cfg.mlp.name](**cfg.mlp, small_dense_density=cfg.masking.density, **dict(cfg.engine))
    assert m.cfg["hidden_size"] == 90 and m._engine_width == 128 and m._padded
    assert m.LF_siren.layers[0].linear.weight.shape == (90, 2) and m.HF_siren.layers[7].linear.weight.shape == (3, 90)
    idx = m._padded_index(torch.device("cpu"))
    assert idx.numel() == sum(p.numel() for p in m._param_list()) and idx.unique().numel() == idx.numel()
    assert int(idx.max()) < 2 * m._sub_engine_params()


def test_abi_exports_the_wavelet_entry_points():
    lib = _engine.load_library()
    assert lib.sf_abi_version() == _engine.SF_ABI_VERSION == 3
    syms = _engine.exported_symbols()
    for s in ("sf_wavelet_create", "sf_wavelet_debug"):
        assert s in syms and hasattr(lib, s)
    assert _engine.has_wavelet(lib)

    class Stale:   # a library built before WaveletSiren
        sf_create = None
    assert not _engine.has_wavelet(Stale())


def _cfg(**kw):
    base = dict(abi_version=_engine.SF_ABI_VERSION, height=64, width=64, in_features=2, out_features=3, hidden=64, depth=4,
                wavelet_levels=1, first_omega_0=50.0, hidden_omega_0=30.0, outermost_linear=1, compute_dtype=1, beta1=0.9,
                beta2=0.999, eps=1e-8, device=0, stream=None, chunk_pixels=0, scratch_format=0)
    base.update(kw)
    return _engine.sf_wavelet_config(**base)


@pytest.mark.parametrize("bad, word", [(dict(abi_version=2), b"abi"), (dict(hidden=96), b"hidden"),
                                       (dict(hidden=512), b"hidden"), (dict(wavelet_levels=2), b"wavelet_levels"),
                                       (dict(width=48), b"square"), (dict(height=63, width=63), b"even"),
                                       (dict(scratch_format=8), b"format"), (dict(scratch_format=12), b"format"),
                                       (dict(compute_dtype=0), b"fp16"), (dict(out_features=1), b"out_features"),
                                       (dict(depth=1), b"depth"), (dict(chunk_pixels=-1), b"chunk_pixels")])
def test_wavelet_create_rejects_bad_configs_without_a_gpu(bad, word):
    lib = _engine.load_library()
    h = C.c_void_p()
    assert lib.sf_wavelet_create(C.byref(_cfg(**bad)), C.byref(h)) == -1
    assert word in lib.sf_last_error() and not h.value
    assert lib.sf_wavelet_create(None, C.byref(h)) == -1
    assert lib.sf_wavelet_debug(None, 0, None, None, None, None, None) == -1


# ---- wavelet_shapes.npz: every sub-network kernel path the GPU shape matrix runs (tests/_wavelet_shapes_child.py) ----
@pytest.fixture(scope="module")
def shapes_fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "wavelet_shapes.npz"), allow_pickle=False)


def _shapes():
    import _wavelet_shapes_child as ch
    return ch.SHAPES


def _engine_flat(m):
    """a host model's parameters in the engine layout ([LF | HF] at the engine width, padded slots 0)"""
    import _wavelet_ref as wr
    flat = torch.zeros(2 * m._sub_engine_params())
    flat[m._padded_index(torch.device("cpu"))] = wr.model_flat(m)
    return flat


def test_shapes_fixture_covers_the_gpu_matrix(shapes_fixture):
    assert [str(t) for t in shapes_fixture["tags"]] == list(_shapes())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "wavelet_shapes.npz")) < 256 * 1024
    kws = [kw for kw, _ in _shapes().values()]
    assert any(kw.get("outermost_linear") is False for kw in kws)
    assert any(kw.get("first_omega_0", 50.0) != 50.0 or kw.get("hidden_omega_0", 50.0) != 30.0 for kw in kws)


@pytest.mark.parametrize("tag", ["h32_d3_s24", "h64_d2_s10", "h128_d5_sin_s40", "h256_d2_s30", "h256_d6_s64",
                                 "h256_d4_sin_om_s48", "h181p_d4_s48", "h32_d16_s20", "h64_d3_s2", "h64_d3_s4",
                                 "h64_d3_s6"])
def test_shapes_init_and_mirror_match_the_reference(shapes_fixture, tag):
    """Seed-0 init at every shape of the GPU matrix is bit-exact against the reference (sha256 per tensor: widths 32 / 256,
    depths 2 / 16, Small_Dense 181, a sine output layer, omegas 30 / 50).  The mirror, run in fp32 as the reference is,
    reproduces its prediction, loss and gradient norms (measured: bit-identical); in fp64 it is within 4.0e-6 (prediction,
    the sine-output shapes), 1.8e-7 (loss) and 1.1e-6 (gradient norms), which is what the GPU tests compare with."""
    import _wavelet_ref as wr
    from oracle import siren_oracle as so
    g = shapes_fixture
    kw, H = _shapes()[tag]
    m = _wavelet(**kw)
    names = [n for n, _ in m.named_parameters()]
    assert names == [str(n) for n in g[f"{tag}/names"]]
    for (n, p), ref in zip(m.named_parameters(), g[f"{tag}/sha"]):
        assert hashlib.sha256(p.detach().numpy().astype(np.float32).tobytes()).hexdigest() == ref.decode(), (tag, n)
    img = so.synthetic_image(H, H, seed=5)
    c = m.cfg
    for dtype, pbar, lbar, gbar in ((torch.float32, 1e-6, 1e-6, 1e-5), (torch.float64, 1e-5, 1e-6, 5e-6)):
        pred, loss, grad = wr.loss_and_grads(wr.model_flat(m), c["hidden_size"], c["depth"], img, c["first_omega_0"],
                                             c["hidden_omega_0"], dtype, c["outermost_linear"])
        assert (pred.double() - torch.tensor(g[f"{tag}/pred"]).double()).abs().max().item() <= pbar, (tag, dtype)
        assert abs(loss - float(g[f"{tag}/loss"])) <= lbar * float(g[f"{tag}/loss"]), (tag, dtype)
        off = 0
        for (n, p), ref in zip(m.named_parameters(), g[f"{tag}/gradnorm"]):
            gr = grad[off:off + p.numel()]
            off += p.numel()
            assert abs(gr.double().norm().item() - ref) <= gbar * ref, (tag, dtype, n)


def test_mirror_without_outermost_linear_is_not_the_linear_mirror(shapes_fixture):
    """the sine output layer changes the mirror's prediction (the fixture of a sine-output shape is not met by the
    linear-output mirror), so the test above pins outermost_linear=False"""
    import _wavelet_ref as wr
    from oracle import siren_oracle as so
    kw, H = _shapes()["h128_d5_sin_s40"]
    m = _wavelet(**kw)
    pred, _, _ = wr.loss_and_grads(wr.model_flat(m), 128, 5, so.synthetic_image(H, H, seed=5), 50.0, 30.0)
    assert (pred - torch.tensor(shapes_fixture["h128_d5_sin_s40/pred"]).double()).abs().max().item() > 1e-2


def test_engine_model_sub_network_is_engine_model_split_at_dlast():
    """sub_forward16 + sub_backward16, fed the SIREN's own fp16 dL/dout at engine_model's 2^20 scale, are
    oracle/engine_model.loss_and_grads(scratch=16) bit for bit: the WaveletSiren model reuses its rounding points"""
    import _wavelet_ref as wr
    from oracle import engine_model as em
    from oracle import siren_oracle as so
    for hidden, depth in ((64, 4), (32, 2)):
        p = so.siren_init(hidden, depth, seed=0)
        H = 24
        grid, img = so.get_grid(H, H), so.synthetic_image(H, H, seed=5)
        _, sse, grads, pred = em.loss_and_grads(p, grid, img, scratch=16)
        pp, dfac, state = wr.sub_forward16(p, grid, 50.0, 30.0)
        assert dfac is None and torch.equal(pp.reshape(H, H, 3), pred)
        dl = em._rt((pp - img.reshape(-1, 3)) * torch.tensor(1.0 / (3 * H * H), dtype=torch.float32) * 2.0 ** 20, "f16")
        for a, b in zip(grads, wr.sub_backward16(p, state, dl, 2.0 ** 20, 50.0, 30.0)):
            assert torch.equal(a, b)


def test_engine_model_prescale_comes_from_the_image():
    import _wavelet_ref as wr
    assert wr.gpre_of(4096) == 2.0 ** 28 and wr.gpre_of(24) == 2.0 ** 13 and wr.gpre_of(2) == 2.0 ** 6


@pytest.mark.parametrize("tag", ["h32_d3_s24", "h128_d5_sin_s40", "h256_d4_sin_om_s48", "h181p_d4_s48", "h32_d16_s20",
                                 "h64_d3_s2"])
def test_engine_model_sits_at_the_fp16_gap_from_fp64(tag):
    """engine_model_loss_and_grads (the engine's rounding points) against the fp64 mirror on the engine layout.  Measured:
    prediction <= 5.9e-5 max abs with a linear output, 1.2e-3 with a sine output (omega 30 / 50 times the fp16 output
    weights); loss <= 6.3e-5 relative; per-tensor gradient max |err| / max |ref| 1.0e-4 .. 3.7e-3 (h32_d16_s20).  Both
    sides are bounded: a model that lost its fp16 roundings would sit near 0, one with a wrong rounding point or a missing
    dfac far above."""
    import _wavelet_ref as wr
    from oracle import siren_oracle as so
    kw, H = _shapes()[tag]
    m = _wavelet(**kw)
    c, W = m.cfg, m._engine_width
    flat = _engine_flat(m)
    img = so.synthetic_image(H, H, seed=5)
    args = (c["first_omega_0"], c["hidden_omega_0"])
    p64, l64, g64 = wr.loss_and_grads(flat, W, c["depth"], img, *args, outermost_linear=c["outermost_linear"])
    pm, sm, gm = wr.engine_model_loss_and_grads(flat, W, c["depth"], img, *args, c["outermost_linear"])
    assert pm.dtype == gm.dtype == torch.float64
    assert 1e-6 < (pm - p64).abs().max().item() < (2.5e-3 if not c["outermost_linear"] else 1.5e-4), tag
    assert abs(sm / (3 * H * H) - l64) < 1.5e-4 * l64, tag
    worst = 0.0
    for a, b in zip(wr.split_flat(gm, W, c["depth"])[0] + wr.split_flat(gm, W, c["depth"])[1],
                    wr.split_flat(g64, W, c["depth"])[0] + wr.split_flat(g64, W, c["depth"])[1]):
        if b.abs().max() == 0:   # padded-only rows / columns: exactly zero on both sides
            assert a.abs().max() == 0, tag
            continue
        e = _rel(a, b)
        assert e < 8e-3, (tag, e)
        worst = max(worst, e)
    assert worst > 5e-5, (tag, worst)
