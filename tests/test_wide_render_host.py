"""Host side of the wide render handle (sf_wide_render_create / sf_wide_render / sf_wide_render16) and of decode.render=wide,
no GPU needed: the mode and its refusals, what the other modes keep answering at widths 512 / 1024, the three symbols in the
header, the prototype table and a built library, and the creator's width check (which comes before the device is asked for)."""
import ctypes as C
import os

import pytest
import torch

from implicit_image import _engine
from implicit_image import decode as dec
from implicit_image.config import _wrap
from implicit_image.models import registry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
SYMBOLS = ("sf_wide_render_create", "sf_wide_render", "sf_wide_render16")


def shape_of(name, hidden, depth=8, density=None, masking=None, H=64, W=64, **mlp):
    return _wrap({"mlp": dict({"name": name, "hidden_size": hidden, "depth": depth, "first_omega_0": 50, "hidden_omega_0": 30,
                               "outermost_linear": True}, **mlp),
                  "img": {"height": H, "width": W}, "engine": {}, "masking_name": masking or ("Small_Dense" if density else None),
                  "small_dense_density": density})


def test_render_mode_takes_wide():
    assert dec.render_mode({"render": "wide"}) == "wide"
    assert "wide" in dec.RENDER_MODES and dec.render_mode({}) == "auto"
    for bad in ("Wide", "wide_render", "512"):
        with pytest.raises(ValueError, match="decode.render"):
            dec.render_mode({"render": bad})


@pytest.mark.parametrize("hidden,depth,want", [
    (512, 8, "SIREN 512x8: sf_wide_render"), (1024, 8, "SIREN 1024x8: sf_wide_render"), (512, 3, "SIREN 512x3: sf_wide_render"),
    (300, 4, "SIREN 512x4 (width 300 zero-padded): sf_wide_render"), (724, 5, "SIREN 1024x5 (width 724 zero-padded): sf_wide_render"),
    (257, 3, "SIREN 512x3 (width 257 zero-padded): sf_wide_render"),
])
def test_choose_path_wide_answers_the_kernel_path(hidden, depth, want):
    assert dec.choose_path(shape_of("siren", hidden, depth), "wide", 64, 64) == ("kernel", want)


def test_choose_path_wide_for_small_dense_uses_the_engine_width():
    s = shape_of("siren", 1024, 6, density=0.25)                    # int(1024 * sqrt(0.25)) = 512: no padding
    assert dec.engine_width(s) == 512
    assert dec.choose_path(s, "wide", 64, 64) == ("kernel", "SIREN 512x6: sf_wide_render")
    s = shape_of("siren", 512, 6, density=0.5)                      # int(512 * sqrt(0.5)) = 362 -> 512
    assert dec.choose_path(s, "wide", 64, 64) == ("kernel", "SIREN 512x6 (width 362 zero-padded): sf_wide_render")


@pytest.mark.parametrize("shape,word", [
    (shape_of("siren", 256), "decode.render=kernel"), (shape_of("siren", 32), "decode.render=kernel"),
    (shape_of("siren", 200, 4), "decode.render=kernel"), (shape_of("siren", 512, 8, density=0.25), "decode.render=kernel"),
    (shape_of("siren", 512, 2), "depth >= 3"),
    (shape_of("siren", 512, masking="Feathermap"), "SIREN only"), (shape_of("siren", 128, masking="Feathermap"), "SIREN only"),
    (shape_of("fourier", 128, map_size=256), "SIREN only"), (shape_of("fourier", 512, map_size=256), "SIREN only"),
    (shape_of("wavelet_siren", 128), "SIREN only"), (shape_of("wavelet_siren", 512), "SIREN only"),
])
def test_choose_path_wide_refuses_everything_else(shape, word):
    with pytest.raises(ValueError, match="^decode.render=wide: ") as e:
        dec.choose_path(shape, "wide", 64, 64)
    assert word in str(e.value), str(e.value)
    ok, why = dec.wide_available(shape)
    assert not ok and str(e.value) == f"decode.render=wide: {why}"


def test_wide_names_the_family_it_refuses():
    for shape, name in ((shape_of("siren", 512, masking="Feathermap"), "Feathermap"), (shape_of("fourier", 128), "FourierNet"),
                        (shape_of("wavelet_siren", 128), "WaveletSiren")):
        assert name in dec.wide_available(shape)[1]


@pytest.mark.parametrize("hidden", [512, 1024, 300, 724])
def test_auto_and_kernel_are_unchanged_at_the_wide_widths(hidden):
    s = shape_of("siren", hidden)
    assert dec.choose_path(s, "auto", 64, 64)[0] == "torch"
    assert dec.render_path(s)[0] == "torch"
    ok, why = dec.kernel_available(s)
    assert not ok and "wide path" in why
    with pytest.raises(ValueError, match=f"decode.render=kernel: SIREN width {hidden} is on the wide path"):
        dec.choose_path(s, "kernel", 64, 64)
    assert dec.choose_path(s, "torch", 64, 64) == ("torch", "decode.render=torch")


def test_wide_mode_refuses_before_a_file_is_read_or_the_device_touched(tmp_path):
    """the run directory holds no weights and this machine may have no GPU - neither is reached"""
    over = [f"decode.dir={tmp_path}", "decode.render=wide", "img.height=64", "img.width=64"]
    with pytest.raises(ValueError, match="decode.render=wide: SIREN width 64 .*decode.render=kernel"):
        dec.decode(over + ["mlp.hidden_size=64", "mlp.depth=4"])
    with pytest.raises(ValueError, match="decode.render=wide: the wide render is SIREN only"):
        dec.decode(over + ["mlp=fourier", "mlp.hidden_size=64", "mlp.depth=4"])
    with pytest.raises(ValueError, match="decode.render=wide: the wide render is SIREN only"):
        dec.decode(over + ["mlp=wavelet_siren", "mlp.hidden_size=64", "mlp.depth=4"])
    with pytest.raises(ValueError, match="decode.render=wide: the wide render is SIREN only"):
        dec.decode(over + ["masking=Feathermap", "mlp.hidden_size=512", "mlp.depth=4"])
    # a shape the mode takes gets past the refusal and fails on the empty directory instead
    with pytest.raises(FileNotFoundError):
        dec.decode(over + ["mlp.hidden_size=512", "mlp.depth=4"])


def test_header_table_and_classes_declare_the_entry_points():
    assert "int sf_wide_render_create(const sf_config* cfg, sf_handle** out);" in HEADER
    assert "int sf_wide_render(sf_handle* h, uint8_t* rgb8_dev, float* pred_dev);" in HEADER
    assert "int sf_wide_render16(sf_handle* h, uint16_t* rgb16_dev, float* pred_dev);" in HEADER
    assert set(SYMBOLS) <= set(_engine.exported_symbols())
    assert sorted(_engine.PROTOTYPES) == list(_engine.exported_symbols())
    assert [C.POINTER(_engine.sf_config), C.POINTER(C.c_void_p)] == _engine.PROTOTYPES["sf_wide_render_create"][1]
    for name in SYMBOLS[1:]:
        assert _engine.PROTOTYPES[name][1] == [C.c_void_p, C.c_void_p, C.c_void_p] and _engine.PROTOTYPES[name][2] is C.c_int
    assert issubclass(_engine.WideRenderEngine, _engine.RenderEngine)
    assert _engine.WideRenderEngine._CREATE == "sf_wide_render_create"
    assert _engine.WideRenderEngine._CREATE_NEEDS[0] is _engine.has_wide_render
    assert _engine.RenderEngine._CREATE == "sf_render_create"            # the narrow handle keeps its creator
    assert _engine.SF_ABI_VERSION == 3


def test_has_wide_render_needs_all_three_symbols():
    def fake(names):
        return type("Lib", (), {n: None for n in names})()
    assert _engine.has_wide_render(fake(SYMBOLS))
    for n in SYMBOLS:
        assert not _engine.has_wide_render(fake([m for m in SYMBOLS if m != n])), n


def test_built_library_exports_them_and_checks_the_width_first():
    """sf_wide_render_create's width check comes before the device is asked for, so it answers on a machine without a GPU;
    so do the null checks of the two render calls.  sf_render_create keeps its own refusal at hidden 512."""
    lib = _engine.load_library()
    for n in SYMBOLS:
        assert hasattr(lib, n), n
    assert _engine.has_wide_render(lib)
    h = C.c_void_p(1)
    for hidden, depth in ((256, 8), (64, 4), (100, 4), (2048, 4), (512, 2)):
        cfg = _engine.sf_config(_engine.SF_ABI_VERSION, 64, 64, 0, 0, 2, 3, hidden, depth, 50.0, 30.0, 1, 1, 0.9, 0.999, 1e-8, 0,
                                None, 0, 0)
        assert lib.sf_wide_render_create(C.byref(cfg), C.byref(h)) == -1, (hidden, depth)
        msg = lib.sf_last_error().decode()
        assert "sf_wide_render_create" in msg and "sf_render_create" in msg and "512 / 1024" in msg, msg
        assert not h.value
        h = C.c_void_p(1)
    assert lib.sf_wide_render_create(None, C.byref(h)) == -1
    cfg = _engine.sf_config(99, 64, 64, 0, 0, 2, 3, 512, 4, 50.0, 30.0, 1, 1, 0.9, 0.999, 1e-8, 0, None, 0, 0)
    assert lib.sf_wide_render_create(C.byref(cfg), C.byref(h)) == -1 and b"abi_version" in lib.sf_last_error()
    cfg.abi_version, cfg.out_features = _engine.SF_ABI_VERSION, 4
    assert lib.sf_wide_render_create(C.byref(cfg), C.byref(h)) == -1 and b"out_features" in lib.sf_last_error()
    assert lib.sf_wide_render(None, None, None) == -1 and lib.sf_wide_render16(None, None, None) == -1
    cfg.out_features = 3
    assert lib.sf_render_create(C.byref(cfg), C.byref(h)) == -1 and b"wide path" in lib.sf_last_error()


def test_siren_model_picks_the_render_engine_by_its_engine_width():
    """_new_render_engine hands the model's own mapping to WideRenderEngine above 256 and to RenderEngine up to it"""
    seen = []

    def record(cls):
        return type("Rec" + cls.__name__, (), {"__init__": lambda self, *a, **k: seen.append((cls.__name__, a, k))})

    real = _engine.RenderEngine, _engine.WideRenderEngine
    _engine.RenderEngine, _engine.WideRenderEngine = record(real[0]), record(real[1])
    try:
        for hidden, depth, cls, width in ((512, 3, "WideRenderEngine", 512), (300, 4, "WideRenderEngine", 512),
                                          (724, 3, "WideRenderEngine", 1024), (256, 3, "RenderEngine", 256), (90, 3, "RenderEngine", 128)):
            with torch.random.fork_rng(devices=[]):
                m = registry["siren"](depth=depth, hidden_size=hidden, first_omega_0=50, hidden_omega_0=30)
            m._new_render_engine(7, 9, 0)
            name, args, kw = seen.pop()
            assert (name, args[:2], kw["hidden"], kw["depth"], kw["chunk_pixels"]) == (cls, (7, 9), width, depth, 0), (hidden, name, kw)
    finally:
        _engine.RenderEngine, _engine.WideRenderEngine = real
