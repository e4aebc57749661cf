"""The inference-only WaveletSiren path (sf_wavelet_render_create / sf_wavelet_render, csrc/wavelet_render.hip) and `decode`
of WaveletSiren / zero-padded fits on an MI355X.  One case of tests/_wavelet_render_child.py per child process.  No
tolerance unless one is named."""
import json

import pytest

from _gpu_child import run_case
from _gpu_fixtures import TRAINING_CALLS

pytestmark = pytest.mark.gpu
CHILD = "_wavelet_render_child.py"


@pytest.fixture(scope="module")
def bitid(tmp_path_factory):
    return run_case(CHILD, "bitid", tmp_path=tmp_path_factory.mktemp("wv_bitid"), timeout=600)["cases"]


def test_render_pred_is_bit_identical_to_the_training_forward(bitid):
    """widths 32 / 64 / 128 / 256, depths 2 / 3 / 4 / 5 / 8 / 16 (k_fwd<32 | 64 | 128 | 256> and k_fwd_pipe), linear and sine
    output, omegas 30 / 50, pictures 2, 4, 6, 10, 64, 100, 250 squared, coefficient grids of 3 and 11 chunks; at the
    initialisation and with both output layers scaled by 400: torch.equal(full-window pred of a render handle, sf_forward's
    pred of a training handle), and the same for sf_wavelet_render on the training handle itself.  All values finite."""
    assert len(bitid) == 13 * 2
    for c in bitid:
        print({k: c[k] for k in ("hidden", "depth", "H", "chunk", "linear", "scale", "pred_equal", "pred_equal_train_handle",
                                 "below0", "above1")})
    bad = [c for c in bitid if not (c["pred_equal"] and c["pred_equal_train_handle"] and c["finite"])]
    assert not bad, bad[:4]


def test_render_bytes_equal_the_conversion_of_the_kernels_own_prediction(bitid):
    """rgb8 == decode.to_u8(pred) of the kernel's own pred (and an independent statement of the same formula), exactly; the
    bytes depend neither on whether pred is written nor on the kind of handle; the scaled cases are clamped at both ends."""
    bad = [c for c in bitid if not (c["u8_equal"] and c["u8_ref_equal"] and c["u8_only_equal"] and c["u8_train_equal"])]
    assert not bad, bad[:4]
    for c in bitid:
        if c["scale"] > 1:
            assert c["below0"] > 0 and c["above1"] > 0, c
            assert c["clamped0"] == c["below0"] and c["clamped255"] == c["above1"], c


def test_ragged_outputs_and_the_guard_region(tmp_path):
    """byte counts that are no multiple of 4 (a 5 x 7 window of a 10 x 10 picture: 105 bytes; 1 x 1: 3 bytes), windows whose
    first pixel is no multiple of 64, on both kinds of handle, with and without pred: bytes and pred equal that region of
    the training forward, and the 256 bytes behind the output stay untouched."""
    r = run_case(CHILD, "ragged", tmp_path=tmp_path, timeout=300)["cases"]
    assert any(c["nbytes"] % 4 for c in r) and any(c["nbytes"] == 105 for c in r) and any(c["nbytes"] == 3 for c in r)
    for c in r:
        for k in ("render_pred", "render_nopred", "train_pred", "train_nopred"):
            v = c[k]
            assert v["rc"] == 0 and v["bytes_equal"] and v["guard_intact"] and v["pred_equal"], (c["H"], c["win"], k, v)


def test_windows_and_bands_equal_the_full_render(tmp_path):
    """128 x 128 (64x4) and 250 x 250 (256x3, k_fwd_pipe): rows 32:96 x cols 16:80, the four corners, 1 x 1 windows; every
    single-row and single-column window of a 10 x 10 picture: pred and bytes equal that region of the full render, on a
    render handle and on a training handle.  decode's band loop with band_rows=7 equals one band (full picture and a
    window); a handle created with max_rows = 7 draws 7 rows and refuses 8 with SF_ERR_INVALID."""
    r = run_case(CHILD, "windows", tmp_path=tmp_path, timeout=400)
    assert len(r["windows"]) == 9 + 9 + 20
    bad = [w for w in r["windows"] if not (w["pred_equal"] and w["u8_equal"] and w["train_pred_equal"] and w["train_u8_equal"])]
    assert not bad, bad[:4]
    assert r["band_equal"] and r["band_pred_equal"] and r["band_window_equal"]
    assert r["rows7_rc"] == 0
    assert r["rows8_rc"] == -1 and "max_rows" in r["rows8_msg"]
    assert r["distinct_levels_128"] > 16 and r["distinct_levels_250"] > 16          # pictures, not constants


def test_render_against_the_reference_predictions(tmp_path):
    """tests/golden/wavelet_grads.npz (minted by the reference: the seed-0 64x4 and yaml models on 64 x 64):
    max |render pred - reference pred| < 1.5e-4, the bound tests/test_gpu_wavelet.py holds the training forward to
    (measured there 6.6e-5 / 7.1e-5); the byte picture differs from to_u8(reference pred) by at most one level."""
    r = run_case(CHILD, "reference", tmp_path=tmp_path, timeout=180)
    print(r)
    for tag in ("small", "yaml"):
        assert r[tag]["max_abs"] < 1.5e-4, r
        assert r[tag]["max_levels"] <= 1, r


def test_refusals(tmp_path):
    """every training call (TRAINING_CALLS) plus sf_render and sf_set_target on a WaveletSiren render handle:
    SF_ERR_INVALID and 'render handle' in the message; sf_wavelet_render's own argument checks; nothing is launched by a
    refused call (the handle's profile counts no launch); the calls that must keep working return 0"""
    r = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=180)
    for name in TRAINING_CALLS + ["sf_render", "sf_set_target"]:
        assert r[name]["rc"] == -1, (name, r[name])
        assert "render handle" in r[name]["msg"], (name, r[name])
    assert r["before_set_coords"]["rc"] == -4 and r["before_set_coords"]["msg"]
    for name in ("wr_both_null", "wr_misaligned", "wr_empty", "wr_reversed", "wr_negative", "wr_beyond", "wr_beyond_cols",
                 "wr_siren_handle", "wr_fourier_handle"):
        assert r[name]["rc"] == -1 and r[name]["msg"], (name, r[name])
    assert r["launches_after_refusals"] == 0
    for name, v in r.items():
        if name.startswith("ok_"):
            assert v["rc"] == 0, (name, v)
    P0 = (2 * 64 + 64) + 2 * (64 * 64 + 64) + (3 * 64 + 3)
    assert r["param_offset_hf_layer1"] == [P0 + 192, P0 + 192 + 64 * 64, 2 * P0]
    assert r["k_wv_render_launches"] == 1 and r["k_render_launches"] == 2
    for name, word in (("create_odd", "even, square"), ("create_hidden", "hidden"), ("create_bf16", "fp16"),
                       ("create_depth", "depth"), ("create_max_rows", "max_rows"), ("create_abi", "abi_version")):
        assert r[name]["rc"] == -1 and word in r[name]["msg"] and r[name]["handle_null"], (name, r[name])


def test_render_handle_memory(tmp_path):
    """yaml model 128x8 at 2048 x 2048 (n = 1026), full window, each handle in a fresh process: the render handle takes less
    than 64 MiB (the allowance of test_gpu_render.py::test_render_handle_memory) + 24 B x n^2 (the two coefficient buffers);
    the training handle takes at least the two sub-networks' phase + delta scratch more, counted as twice what
    sf_debug_scratch reports for a plain SIREN training handle of 128x8, scratch format 16, on a 1026 x 1026 grid."""
    tr = run_case(CHILD, "mem", "train", tmp_path=tmp_path, timeout=240)
    rn = run_case(CHILD, "mem", "render", tmp_path=tmp_path, timeout=240)
    scratch = 2 * sum(tr["sub_scratch"].values())
    print({"train": tr, "render": rn, "two_sub_scratch": scratch})
    assert rn["n"] == 1026
    assert 0 < rn["taken"] < (64 << 20) + 24 * rn["n"] ** 2
    assert scratch > (1 << 30)
    assert tr["taken"] - rn["taken"] >= scratch


def test_fit_then_decode_end_to_end(tmp_path):
    """fit_one (mlp=wavelet_siren 64x4 on 64 x 64, masking none and Small_Dense 0.5 - width 45 zero-padded to 64 -
    quant=none, 40 steps) -> decode: the kernel path from model.pth; the PPM equals to_u8(model(grid)) of the fitted model
    byte for byte; PSNR_8bit as printed equals decode.metrics on those bytes; decode.height=128 decode.width=128 equals a
    fresh registry model with the state dict on the 128 x 128 grid; a window in bands of 7 rows equals that region.  A SIREN
    fit whose Small_Dense width is 181 (hidden 256, density 0.5) decodes on the kernel path to its own model's bytes."""
    r = run_case(CHILD, "e2e", tmp_path=tmp_path, timeout=900)
    print(json.dumps(r, indent=1))
    for tag in ("none", "small_dense"):
        c = r[tag]
        assert c["path"] == "kernel" and c["source"] == "pth"
        assert c["ppm_equal"]
        assert c["psnr8_decode"] == c["psnr8_metrics_on_bytes"]
        assert c["big_path"] == "kernel" and c["big_shape"] == [128, 128] and c["big_equal"]
        assert c["window_equal"]
    assert r["none"]["logical_width"] == 64 and r["small_dense"]["logical_width"] == 45 and r["small_dense"]["engine_width"] == 64
    s = r["siren181"]
    assert s["logical_width"] == 181 and s["path"] == "kernel" and s["source"] == "pth" and s["ppm_equal"]
