"""Host side of the ctypes binding, no GPU needed: the one prototype table against the header, the group checks derived
from it, the four config structs against their C declarations, and the one width rule as the models and the decoder see it."""
import ctypes as C
import os
import re

import pytest

from implicit_image import _engine
from implicit_image import decode as dec
from implicit_image.config import _wrap
from implicit_image.models import registry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
GROUPS = {"feather": _engine.has_feather, "wavelet": _engine.has_wavelet, "render": _engine.has_render,
          "wavelet_render": _engine.has_wavelet_render, "fourier_render": _engine.has_fourier_render}
CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "void*": C.c_void_p}


def names_of(group):
    return [n for n, proto in _engine.PROTOTYPES.items() if proto[0] == group]


def test_table_and_header_name_the_same_entry_points():
    assert sorted(_engine.PROTOTYPES) == list(_engine.exported_symbols())
    assert {proto[0] for proto in _engine.PROTOTYPES.values()} == {"core"} | set(GROUPS)
    assert _engine.PROTOTYPES["sf_last_error"][2] is C.c_char_p
    assert all(proto[2] is C.c_int for n, proto in _engine.PROTOTYPES.items() if n != "sf_last_error")


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_group_check_needs_every_symbol_of_the_group(group):
    """a fake library with every entry point of the table: the group's has_* is true; take any one of the group's away and
    it is false (has_fourier_render also needs the render group)"""
    def fake(without=()):
        return type("Lib", (), {n: None for n in _engine.PROTOTYPES if n not in without})()

    has, names = GROUPS[group], names_of(group)
    assert names and has(fake())
    for n in names + (names_of("render") if group == "fourier_render" else []):
        assert not has(fake(without=(n,))), n
    other = [n for g in GROUPS if g != group and not (group == "fourier_render" and g == "render") for n in names_of(g)]
    assert has(fake(without=other))                      # and of nothing else


def header_fields(struct):
    """[(name, C type)] of `typedef struct <struct> { ... } <struct>;`, comments dropped, `int32_t height, width;` split"""
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s;" % (struct, struct), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(int32_t|int64_t|float|void\s*\*)\s*(.+)", decl, re.S)
        assert m, f"{struct}: cannot read `{decl}`"
        out += [(name.strip(), re.sub(r"\s", "", m.group(1))) for name in m.group(2).split(",")]
    return out


def test_header_declares_four_config_structs():
    assert sorted(re.findall(r"typedef struct (sf_\w*config) \{", HEADER)) == [
        "sf_config", "sf_fourier_config", "sf_wavelet_config", "sf_wavelet_render_config"]


@pytest.mark.parametrize("struct", ["sf_config", "sf_fourier_config", "sf_wavelet_config", "sf_wavelet_render_config"])
def test_config_struct_matches_the_header(struct):
    want = [(name, CTYPES[ctype]) for name, ctype in header_fields(struct)]
    assert len(want) >= 13
    assert [(f[0], f[1]) for f in getattr(_engine, struct)._fields_] == want


def test_header_parser_splits_joint_declarations():
    names = [n for n, _ in header_fields("sf_config")]
    assert names[:5] == ["abi_version", "height", "width", "row_begin", "row_end"]
    assert ("stream", "void*") in header_fields("sf_config") and ("chunk_pixels", "int64_t") in header_fields("sf_config")


def test_one_width_rule_for_models_and_decoder():
    """decode.padded_width and the models' _engine_width agree for every hidden width 1..1024 at density 1; above its own
    limit each refuses as it always has (the decoder answers None, the models raise)"""
    def padded(h, name="siren"):
        return dec.padded_width(_wrap({"mlp": {"name": name, "hidden_size": h}, "small_dense_density": None}))

    for h in range(1, 1025):
        want = next(w for w in (32, 64, 128, 256, 512, 1024) if w >= h)       # the rule, written out
        assert padded(h) == want
        assert registry["siren"](depth=2 if h <= 256 else 3, hidden_size=h)._engine_width == want, h
        if h <= 256:
            assert registry["fourier"](depth=3, hidden_size=h, map_size=64)._engine_width == want, h
            assert registry["wavelet_siren"](depth=2, hidden_size=h)._engine_width == want, h
    assert padded(1025) is None
    with pytest.raises(NotImplementedError, match="hidden_size 1025 > 1024 is not supported by the gfx950 engine"):
        registry["siren"](depth=3, hidden_size=1025)
    with pytest.raises(NotImplementedError, match="hidden_size 257 > 256 is not supported for FourierNet"):
        registry["fourier"](depth=3, hidden_size=257, map_size=64)
    with pytest.raises(NotImplementedError, match="hidden_size 257 > 256 is not supported for WaveletSiren"):
        registry["wavelet_siren"](depth=3, hidden_size=257)
