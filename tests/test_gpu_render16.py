"""16 bits per sample on the render kernels (sf_render16 / sf_wavelet_render16, decode.bits=16) on an MI355X.
u16 = min(max((int)(pred * 65535.0f), 0), 65535), the product in fp32 and truncated toward zero.  Every comparison is exact
(torch.equal on values widened to int32).  One case of tests/_render16_child.py per child process."""
import json

import pytest

from _gpu_child import run_case

pytestmark = pytest.mark.gpu
CHILD = "_render16_child.py"
CHECKS = ("equals_to_u16", "equals_formula", "alone_equal", "pred_bit_identical", "guard_intact", "u8_after_equal",
          "u8_guard_intact", "finite")


def check_rows(rows):
    """what every model asserts of every (shape, picture, handle): the samples equal decode.to_u16 of the kernel's own pred
    and an independently written formula; samples written alone equal samples written with pred; pred is bit-identical to
    the 8-bit call's; 64 sentinel bytes behind the output are untouched; the 8-bit call afterwards still gives to_u8(pred)"""
    bad = [c for c in rows if c["rc"] != [0, 0, 0, 0] or not all(c[k] for k in CHECKS) or not c.get("pred_is_forward", True)]
    assert not bad, bad[:3]


def test_siren_samples_on_every_kernel_form(tmp_path):
    """k_fwd<32> (32x2), k_fwd<256> (256x2), k_fwd_pipe (256x3) x out_features 1 / 2 / 3 x outermost_linear x 1x1, 5x7 (35
    pixels: a ragged block, an odd sample count at out_features 1 and 3), 33x31, 64x64 x chunk_pixels 0 / 256, on a render
    handle and on a training handle.  The output layer is scaled by 40 with a zero bias: a linear output swings over about
    [-1.5, 3] (the fp64 oracle's range for these seeds), so both clamps are hit and a thousand pixels spread over more
    levels than a byte has."""
    rows = run_case(CHILD, "siren", tmp_path=tmp_path, timeout=600)["cases"]
    assert len(rows) == 3 * 3 * 2 * 4 * 2 * 2
    check_rows(rows)
    assert all("pred_is_forward" in c for c in rows if c["handle"] == "train")
    for c in rows:
        if c["linear"] and c["H"] * c["W"] >= 1000:
            assert c["lo"] > 0 and c["hi"] > 0 and c["levels"] > 256, c      # clamps on both sides; more than a byte's levels


def test_fourier_samples(tmp_path):
    """hidden 32 and 256, map 64, 3 Linear layers, the same pictures and chunkings, render and training handle"""
    rows = run_case(CHILD, "fourier", tmp_path=tmp_path, timeout=300)["cases"]
    assert len(rows) == 2 * 4 * 2 * 2
    check_rows(rows)
    assert all(c["levels"] > 256 for c in rows if c["H"] * c["W"] >= 1000)


def test_wavelet_samples_full_picture_and_windows(tmp_path):
    """32x2 and 256x3 at H = 6, 10, 64: the full picture and windows with odd origins and sizes, one pixel, an odd pixel
    count that is no multiple of 64, on a render handle and on a training handle; pred equals that region of sf_forward's"""
    rows = run_case(CHILD, "wavelet", tmp_path=tmp_path, timeout=300)["cases"]
    assert len(rows) == 2 * (3 + 4 + 5) * 2
    check_rows(rows)
    assert all("pred_is_forward" in c for c in rows)
    assert any(c["lo"] > 0 and c["hi"] > 0 for c in rows)


def test_argument_errors_are_answered_before_any_launch(tmp_path):
    """return codes (SF_ERR_INVALID -1, SF_ERR_STATE -4) and messages; nothing is launched by a refused call"""
    r = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=180)
    print(json.dumps(r, indent=1))

    def refused(name, rc, *words):
        assert r[name]["rc"] == rc and all(w in r[name]["msg"] for w in words), (name, r[name])
    refused("r16_before_coords", -4, "sf_set_coords")
    refused("r16_both_null", -1, "sf_render16", "rgb16_dev", "both NULL")
    refused("r16_odd_base", -1, "sf_render16", "4-byte aligned")
    refused("r16_two_byte_base", -1, "sf_render16", "4-byte aligned")
    refused("r16_null_handle", -1, "null")
    refused("r16_wide_handle", -1, "sf_render16", "32 .. 256")
    refused("r16_fourier_before_coords", -4, "sf_set_coords")
    refused("r16_fourier_before_encoding", -4, "sf_set_encoding")
    refused("r16_wavelet_render_handle", -1, "sf_render16", "sf_wavelet_render16")
    refused("r16_wavelet_train_handle", -1, "sf_render16")
    refused("w16_siren_handle", -1, "sf_wavelet_render16", "not a WaveletSiren handle")
    refused("w16_fourier_handle", -1, "sf_wavelet_render16", "not a WaveletSiren handle")
    refused("w16_before_coords", -4, "sf_set_coords")
    refused("w16_both_null", -1, "sf_wavelet_render16", "rgb16_dev", "both NULL")
    refused("w16_odd_base", -1, "sf_wavelet_render16", "4-byte aligned")
    refused("w16_two_byte_base", -1, "sf_wavelet_render16", "4-byte aligned")
    for name in ("w16_empty", "w16_reversed", "w16_negative", "w16_beyond", "w16_beyond_cols"):
        refused(name, -1, "sf_wavelet_render16", "row0 < row1")
    refused("w16_larger_than_max_rows", -1, "sf_wavelet_render16", "max_rows")
    refused("w16_null_handle", -1, "null")
    assert r["launches_siren"] == 0 and r["launches_fourier"] == 0 and r["launches_wavelet"] == 0
    assert r["ok_r16"]["rc"] == 0 and r["ok_w16"]["rc"] == 0
    # one launch on the existing record, charged 2 bytes per sample: 4096 pixels x 3 x 2
    assert r["k_render_launches"] == 1 and r["k_render_bytes_per_launch"] == 4096 * 3 * 2
    assert "bits must be 8 or 16" in r["binding_bits_12"]
    assert r["binding_itemsize"] == 2 and r["binding_shape"] == [8, 8, 3] and "int16" in r["binding_dtype"]


def test_fit_then_decode_16_bits_end_to_end(tmp_path):
    """fit (SIREN 64x4, FourierNet 64x4 map 128, WaveletSiren 64x4; synthetic 64x64, 30-40 steps) -> decode.bits=16: the
    file is P6 / 65535 and read_ppm of it equals the 16-bit conversion of the fitted model's own forward on the grid;
    decode.render=torch decode.bits=16 writes the same file; with decode.truth PSNR_16bit is there and finite;
    decode.bits=8 is a run without the key, file and figures."""
    r = run_case(CHILD, "e2e", tmp_path=tmp_path, timeout=900)
    print(json.dumps(r, indent=1))
    assert sorted(r) == ["fourier", "siren", "wavelet_siren"]
    for name, c in r.items():
        assert c["path"] == c["want_path"] and c["torch_path"] == "torch", (name, c)
        assert c["header_ok"] and c["ppm_equals_model"] and c["ppm_equals_to_u16"] and c["torch_file_identical"], (name, c)
        assert c["levels"] > 256, (name, c)
        assert c["psnr16_finite"] and c["psnr16"] == pytest.approx(c["psnr16_formula"], rel=1e-9), (name, c)
        assert c["keys16"] == ["PSNR", "PSNR_16bit", "PSNR_8bit", "loss"] and c["keys8"] == ["PSNR", "PSNR_8bit", "loss"], (name, c)
        assert c["bits8_file_identical"] and c["bits8_figures_identical"] and c["plain_is_8bit"], (name, c)
