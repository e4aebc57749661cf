"""Host side of decode.bits=16 without a GPU: to_u16, the 16-bit PPM writer, the decode.bits key, band planning at two bytes
per sample, PSNR_16bit, and the two 16-bit render entry points in the binding table and the header."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def u16_ref(x):
    """min(max((int)(x * 65535.0f), 0), 65535) for an fp32 array, written out in numpy independently of decode.to_u16: the
    product rounded to fp32, truncated toward zero in exact integer arithmetic; NaN -> 0 does not occur in these inputs"""
    prod = (np.asarray(x, dtype=F32) * F32(65535.0)).astype(F32)
    out = np.empty(prod.shape, dtype=np.int64)
    for i, v in np.ndenumerate(prod):
        v = float(v)
        out[i] = 65535 if v >= 65535.0 else (0 if v <= 0.0 else int(math.floor(v)))
    return out


def edge_values():
    vals = [-3.0, -0.0, 0.0, 0.5, float(np.nextafter(F32(1.0), F32(0.0))), 1.0, 1.0 + 2.0 ** -20, 7.0, float("inf"),
            float("-inf"), 1e30, -1e30]
    for k in (1, 2, 255, 256, 257, 32767, 32768, 40000, 65534, 65535):
        q = F32(k) / F32(65535.0)
        vals += [float(np.nextafter(q, F32(-1.0))), float(q), float(np.nextafter(q, F32(2.0)))]
    return np.array(vals, dtype=F32)


def test_to_u16_edge_values_and_random():
    from implicit_image.decode import to_u16
    rng = np.random.default_rng(16)
    x = np.concatenate([edge_values(), rng.uniform(-0.1, 1.1, 4096).astype(F32)])
    got = to_u16(torch.from_numpy(x))
    assert got.dtype == torch.int32 and tuple(got.shape) == x.shape
    want = u16_ref(x)
    assert np.array_equal(got.numpy().astype(np.int64), want), np.nonzero(got.numpy() != want)[0][:8]
    assert int(got.min()) == 0 and int(got.max()) == 65535
    # both sides of a level: some neighbour of k / 65535 falls on k - 1 and some on k
    assert len(set(want[12:12 + 30].tolist())) > 10
    assert to_u16(torch.tensor([0.25], dtype=torch.float64)).dtype == torch.int32       # (computed in fp32 whatever comes in)


@pytest.mark.parametrize("hw", [(1, 1), (7, 5), (33, 64)])
def test_write_ppm16_round_trip_header_and_byte_order(tmp_path, hw):
    from implicit_image.data import read_ppm, write_ppm16
    g = torch.Generator().manual_seed(hw[0] * 131 + hw[1])
    x = torch.randint(0, 65536, (*hw, 3), generator=g, dtype=torch.int32)
    x[0, 0, 0], x[-1, -1, -1] = 0x1234, 65535
    path = str(tmp_path / "x.ppm")
    write_ppm16(path, x)
    back = read_ppm(path)
    assert tuple(back.shape) == (*hw, 3) and torch.equal(back, x)
    raw = open(path, "rb").read()
    header = b"P6\n%d %d\n65535\n" % (hw[1], hw[0])
    assert raw.startswith(header) and len(raw) == len(header) + hw[0] * hw[1] * 3 * 2
    assert raw[len(header):len(header) + 2] == b"\x12\x34"                               # big-endian: high byte first
    assert raw[-2:] == b"\xff\xff"
    for other in (x.numpy(), x.to(torch.int64), x.to(torch.uint16), x.numpy().astype(np.uint16)):
        write_ppm16(str(tmp_path / "y.ppm"), other)
        assert open(tmp_path / "y.ppm", "rb").read() == raw


def test_write_ppm16_refuses_floats_shapes_and_values(tmp_path):
    from implicit_image.data import write_ppm16
    path = str(tmp_path / "z.ppm")
    x = torch.zeros(4, 5, 3, dtype=torch.int32)
    for bad in (x.float(), x.numpy().astype(np.float64), x[..., :2], x[0], x.reshape(4, 5, 3, 1), x - 1, x + 65536):
        with pytest.raises(ValueError):
            write_ppm16(path, bad)
    assert not os.path.exists(path)


def test_decode_bits_is_checked_before_anything_is_read(tmp_path):
    from implicit_image import decode as dec
    missing = str(tmp_path / "no_such_run")
    for bad in ("12", "0", "32", "sixteen", "16.0"):
        with pytest.raises(ValueError, match="decode.bits"):
            dec.decode([f"decode.dir={missing}", f"decode.bits={bad}"])
    assert not os.path.exists(missing)
    assert dec.sample_bits({}) == 8 and dec.sample_bits({"bits": "8"}) == 8 and dec.sample_bits({"bits": "16"}) == 16
    with pytest.raises(FileNotFoundError):                  # a good value gets as far as the missing run directory
        dec.decode([f"decode.dir={missing}", "decode.bits=16"])
    with pytest.raises(ValueError, match="decode.render"):  # render_mode still answers first, the same way
        dec.decode([f"decode.dir={missing}", "decode.render=gpu", "decode.bits=12"])


@pytest.mark.parametrize("hw", [(64, 64), (1000, 700), (30000, 20000), (5, 1 << 19)])
def test_plan_bands_at_two_bytes_per_sample(hw):
    from implicit_image.decode import BAND_BYTES, ROW_LIMIT, plan_bands
    H, W = hw
    for kw in ({}, {"band_rows": 7}, {"band_bytes": 1 << 23}):
        bands = plan_bands(H, W, 3, sample_bytes=2, **kw)
        assert bands[0][0] == 0 and bands[-1][1] == H
        assert all(a[1] == b[0] for a, b in zip(bands, bands[1:])) and all(a < b for a, b in bands)
        for a, b in bands:
            assert (b - a) * W * W < ROW_LIMIT and (b - a) * W * 3 * 2 < kw.get("band_bytes", BAND_BYTES)
        # the default is one byte per sample: existing calls and results do not change
        assert plan_bands(H, W, 3, **kw) == plan_bands(H, W, 3, sample_bytes=1, **kw)
    assert inspect.signature(plan_bands).parameters["sample_bytes"].default == 1
    # where the byte limit binds, two bytes per sample halve the band; where ROW_LIMIT binds, nothing changes
    one, two = plan_bands(H, W, 3), plan_bands(H, W, 3, sample_bytes=2)
    cap1, cap2 = (BAND_BYTES - 1) // (W * 3), (BAND_BYTES - 1) // (W * 6)
    row_cap = (ROW_LIMIT - 1) // (W * W)
    assert one[0][1] == min(H, cap1, row_cap) and two[0][1] == min(H, cap2, row_cap)


def test_plan_wavelet_bands_at_two_bytes_per_sample():
    from implicit_image.decode import BAND_BYTES, plan_wavelet_bands
    H = 20000
    for r, c in (((0, H), (0, H)), ((3, 19999), (1, 12346))):
        one, two = plan_wavelet_bands(H, r, c), plan_wavelet_bands(H, r, c, sample_bytes=2)
        assert one == plan_wavelet_bands(H, r, c, sample_bytes=1)
        for bands, nb in ((one, 1), (two, 2)):
            assert bands[0][0] == r[0] and bands[-1][1] == r[1] and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
            assert all((b - a) * (c[1] - c[0]) * 3 * nb < BAND_BYTES for a, b in bands)
        assert len(two) > len(one)
    assert plan_wavelet_bands(64, (0, 64), (0, 64), sample_bytes=2) == [(0, 64)]


def test_metrics_with_16_bits():
    from implicit_image.decode import metrics, to_u8, to_u16
    img = torch.ones(8, 8, 3)
    pred = torch.zeros(8, 8, 3) + 1e-3
    base = metrics(pred, to_u8(pred), img)
    assert sorted(base) == ["PSNR", "PSNR_8bit", "loss"]                                 # the default key set is today's
    m = metrics(pred, to_u8(pred), img, torch.zeros(8, 8, 3, dtype=torch.int32))         # all 65535 against all 0
    assert sorted(m) == ["PSNR", "PSNR_16bit", "PSNR_8bit", "loss"]
    assert {k: m[k] for k in base} == base
    assert m["PSNR_16bit"] == pytest.approx(0.0, abs=1e-9)                               # 10 log10(65535^2 / 65535^2): no overflow
    g = torch.Generator().manual_seed(3)
    img, pred = torch.rand(16, 16, 3, generator=g), torch.rand(16, 16, 3, generator=g)
    want = np.mean(((img.numpy() * F32(65535)).astype(np.int64) - to_u16(pred).numpy().astype(np.int64)).astype(np.float64) ** 2)
    assert metrics(pred, to_u8(pred), img, to_u16(pred))["PSNR_16bit"] == pytest.approx(10 * math.log10(65535.0 ** 2 / want), rel=1e-12)
    assert metrics(pred, to_u8(pred), img, (img * 65535).int())["PSNR_16bit"] == math.inf   # samples that equal the truth's
    # truncation leaves an error uniform in [0, 1) LSB: about 10 log10(3 * top^2) against the fp32 prediction itself
    x = torch.rand(256, 256, 3, generator=g)
    mse16 = ((x.double() * 65535 - to_u16(x).double()) ** 2).mean().item()
    assert abs(10 * math.log10(65535 ** 2 / mse16) - 10 * math.log10(3 * 65535 ** 2)) < 0.1


def test_binding_table_and_header_have_the_16_bit_entry_points():
    import ctypes as C
    from implicit_image import _engine
    hdr = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
    P = _engine.PROTOTYPES
    # (sf_render16 sits with the symbols every library has: the existing host tests want has_render / has_fourier_render true
    # for a library that has the 8-bit names only, and false when any name of the group is missing)
    assert P["sf_render16"][0] == "core" and P["sf_wavelet_render16"][0] == "wavelet_render"
    assert _engine.has_render(type("Old", (), {"sf_render_create": None, "sf_render": None})())
    assert P["sf_render16"][1] == P["sf_render"][1] and P["sf_wavelet_render16"][1] == P["sf_wavelet_render"][1]
    assert P["sf_render16"][2] is C.c_int and P["sf_wavelet_render16"][2] is C.c_int
    assert "int sf_render16(sf_handle* h, uint16_t* rgb16_dev, float* pred_dev);" in hdr
    assert "int sf_wavelet_render16(sf_handle* h, int32_t row0, int32_t row1, int32_t col0, int32_t col1, uint16_t* rgb16_dev," in hdr
    assert {"sf_render16", "sf_wavelet_render16"} <= set(_engine.exported_symbols())
    for cls in (_engine.RenderEngine, _engine.FourierRenderEngine, _engine.WaveletRenderEngine, _engine.SirenEngine):
        assert inspect.signature(cls.render).parameters["bits"].default == 8
    with pytest.raises(ValueError, match="bits"):
        _engine._render_entry(object(), "sf_render", 12)
