"""The inference-only render path (sf_render_create / sf_render, csrc/siren_render.hip) and `decode` on an MI355X.
One case of tests/_render_child.py per child process."""
import json

import pytest

from _gpu_child import run_case
from _gpu_fixtures import TRAINING_CALLS

pytestmark = pytest.mark.gpu
CHILD = "_render_child.py"


@pytest.fixture(scope="module")
def bitid(tmp_path_factory):
    return run_case(CHILD, "bitid", tmp_path=tmp_path_factory.mktemp("bitid"), timeout=600)["cases"]


def test_render_pred_is_bit_identical_to_the_training_forward(bitid):
    """(hidden, depth) in {(32,3), (64,4), (128,6), (256,8), (256,2)} x {67x45, 256x256, 1031x517 in 64 Ki-pixel chunks} x
    outermost_linear True / False x out_features 3 / 1 x fp16 / bf16 operands, at the SIREN initialisation and with a
    scaled output layer: torch.equal(sf_render's pred on a render handle, sf_forward's pred on a training handle).  No
    tolerance; the same holds for sf_render on the training handle itself."""
    assert len(bitid) == 5 * 3 * 2 * 2 * 2 * 2
    bad = [c for c in bitid if not (c["pred_equal"] and c["pred_equal_train_handle"] and c["finite"])]
    assert not bad, bad[:4]


def test_render_bytes_equal_the_conversion_of_the_kernels_own_prediction(bitid):
    """rgb8 == min(max(trunc(pred * 255), 0), 255) of the kernel's fp32 output, exactly; the bytes do not depend on whether
    pred is also written, nor on the kind of handle.  Both clamps are exercised: with a linear output layer scaled by 400
    (zero output bias) every case has predictions below 0 and above 1.  A sine output layer gives 0.5 + 0.5 sin(.), which
    cannot leave [0, 1], so for those cases the test asserts that range instead."""
    bad = [c for c in bitid if not (c["u8_equal"] and c["u8_only_equal"] and c["u8_train_equal"])]
    assert not bad, bad[:4]
    for c in bitid:
        if c["linear"] and c["scale"] > 1:
            assert c["below0"] > 0 and c["above1"] > 0, c
        if not c["linear"]:
            assert c["pmin"] >= 0.0 and c["pmax"] <= 1.0, c


def test_render_of_the_container_fixture_against_the_fp64_oracle(tmp_path):
    """tests/golden/container_64x4.npz rendered at 64x64: max |pred - oracle.forward| < 5e-4 (smoke()'s bound for this
    shape), and the byte image differs from the oracle's by at most one level anywhere."""
    r = run_case(CHILD, "oracle", tmp_path=tmp_path, timeout=120)
    print(r)
    assert r["max_abs"] < 5e-4
    assert r["max_levels"] <= 1


def test_windows_and_bands_equal_the_full_render(tmp_path):
    """rows=32:96 cols=16:80 of a 128x128 grid == that region of the full 128x128 render; band_rows=7 == one band"""
    r = run_case(CHILD, "windows", tmp_path=tmp_path, timeout=180)
    print(r)
    assert r["window_equal"] and r["window_pred_equal"]
    assert r["band_equal"] and r["band_pred_equal"]
    assert r["distinct_levels"] > 16          # a picture, not a constant


def test_render_handle_refuses_training_calls_and_the_wide_path(tmp_path):
    """argument checks that return SF_ERR_INVALID (-1) with a message; nothing is launched"""
    r = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=120)
    for name in TRAINING_CALLS:
        assert r[name]["rc"] == -1, (name, r[name])
        assert "render handle" in r[name]["msg"], (name, r[name])
    assert r["sf_render_both_null"]["rc"] == -1 and r["sf_render_both_null"]["msg"]
    for name, v in r.items():
        if name.startswith("ok_"):
            assert v["rc"] == 0, (name, v)
    assert r["wide_create"]["rc"] == -1 and "wide path" in r["wide_create"]["msg"] and r["wide_handle_null"]


def test_render_handle_memory(tmp_path):
    """256x8 at 2048x2048, each handle in a fresh process: the render handle takes less device memory than the training
    handle by at least Pbuf + Dbuf + Dlast (sizes as sf_debug_scratch reports them), and its own footprint (it allocates
    no output buffer) is under 64 MiB."""
    tr = run_case(CHILD, "mem", "train", tmp_path=tmp_path, timeout=180)
    rn = run_case(CHILD, "mem", "render", tmp_path=tmp_path, timeout=180)
    scratch = sum(tr["scratch"].values())
    print({"train": tr, "render": rn, "scratch": scratch})
    assert scratch > (1 << 30)                # the 8-bit scratch of 4 Mi pixels x 7 layers x 256 is several GiB
    assert tr["taken"] - rn["taken"] >= scratch
    assert 0 < rn["taken"] < (64 << 20)


def test_fit_then_decode_end_to_end(tmp_path):
    """fit_one (SIREN 64x4, synthetic 64x64, quant=kmeans, entropy_coding=plain; masking none and RigL) -> decode: the PPM
    equals the byte image of the existing engine forward for decompress_state_dict's weights, and the PSNR_8bit decode
    prints equals eval_epoch's formula applied to those clamped bytes exactly.  When no prediction lies outside [0, 1]
    the clamp changes nothing and the figure is also eval_epoch's own ('Quant PSNR 8bit' of the fit, which evaluates the
    quantised model before the fp16 container: compared to 0.5 dB only, the weights differ by the fp16 rounding).
    Fallback: mlp=fourier from model.pth gives a 64x64 file equal to the torch conversion of the model's own forward."""
    r = run_case(CHILD, "e2e", tmp_path=tmp_path, timeout=900)
    print(json.dumps(r, indent=1))
    for tag in ("none", "rigl"):
        c = r[tag]
        assert c["has_decode_json"] and c["path"] == "kernel" and c["source"] == "container"
        assert c["ppm_equal"]
        assert c["psnr8_decode"] == c["psnr8_formula_on_bytes"]          # asserting: the formula on the clamped bytes
        if c["outside_01"] == 0:
            assert abs(c["psnr8_decode"] - c["psnr8_fit"]) < 0.5
    f = r["fourier"]
    assert f["path"] == "torch" and f["source"] == "pth" and f["shape"] == [64, 64, 3] and f["ppm_equal"]
