"""The inference-only Feathermap path on an MI355X: sf_feather_render_attach / sf_feather_render_load on a render handle
(csrc/feather_host.hip, k_fth_mat<true>), FeatherRenderEngine, and `decode` of a masking=Feathermap run.  One case of
tests/_feather_render_child.py per child process."""
import json

import pytest

import _feather_render_child as child  # (the shape lists only: nothing touches the device at import)
from _gpu_child import run_case

pytestmark = pytest.mark.gpu
CHILD = "_feather_render_child.py"
# tests/test_gpu_handle_memory.py's figures: hipMalloc hands out device memory in 2 MiB blocks, and what a create .. destroy
# cycle may leave behind that is not the handle's stands at 0 there (not yet measured), so the slack is one granule
GRANULE = 2 << 20
SLACK = GRANULE


@pytest.mark.parametrize("which", range(len(child.SHAPES)), ids=[f"{s[0]}x{s[1]}" for s in child.SHAPES])
def test_render_handle_is_bit_identical_to_the_training_handle(which, tmp_path):
    """Seeded FeatherNet init on a 37x41 grid (1517 pixels: a ragged last 32-pixel block, six chunks at chunk_pixels=256).
    A training handle (sf_feather_attach, materialised, sf_forward) and a FeatherRenderEngine given the same feather vector:
    get_params is torch.equal over every engine slot and the padding is exactly 0; the fp32 prediction is torch.equal; the
    bytes are decode.to_u8(pred) and the 16-bit samples decode.to_u16(pred).  The five shapes: m below one 16-deep k slice
    (2, 10, 13), a ragged second slice (25), an exact multiple (32); rows_used < n (93 of 94, 99 of 100, 259 of 260); n no
    multiple of the 64 tile; strided logical rows (96 in 128); k_fwd and, at 256x3, k_fwd_pipe.  One load is one
    k_feather_mat launch, under the existing profile line.

    Against float64 (64x4, 96x3, 128x8): max |W - scaler * (V1 V2)| <= 1e-6 max |W|, the bar tests/test_gpu_feather.py holds
    the training handle's product to."""
    hidden, depth, density, P, n, m, width = child.SHAPES[which]
    cases = run_case(CHILD, "bitid", str(which), tmp_path=tmp_path, timeout=120)["cases"]
    print(json.dumps(cases, indent=1))
    assert [c["chunk"] for c in cases] == ([0, 256] if which == child.CHUNKED else [0])
    for c in cases:
        assert c["finite"] and c["levels"] > 16                 # a picture, not a constant
        assert c["num_params"][0] == c["num_params"][1] == c["num_params"][2]
        assert c["feather_elems"] == [2 * n * m + 2 * depth] * 2
        assert c["w_equal"] and c["w_nonzero"] > 0.9 * P
        assert c["padding_max"] == 0.0 and (c["padding_slots"] > 0) == (width != hidden)
        assert c["pred_equal"], c
        assert c["u8_equal"] and c["u16_equal"], c
        assert c["mat_launches"] == 1 and c["render_launches"] == 2 * (6 if c["chunk"] else 1)
        if which in child.FP64 and c["chunk"] == 0:
            assert c["fp64_rel"] <= 1e-6, c["fp64_rel"]
        else:
            assert "fp64_rel" not in c


def test_second_load_replaces_the_network(tmp_path):
    """two seeded 64x4 networks, one handle: after the second load_feather the picture is the second network's (a stale
    weight image would give the first's)"""
    r = run_case(CHILD, "reload", tmp_path=tmp_path, timeout=120)
    print(r)
    assert r["networks_differ"] and r["first_equal"] and r["second_equal"]


def test_refusals_and_what_keeps_working(tmp_path):
    """Status and message of every refusal of the two entry points: attach on a training handle (names sf_feather_attach), on
    a FourierNet render handle, twice, with a wrong depth, n^2 < P, m > n and sizes that do not fit: -1; load before attach
    and sf_render / sf_render16 after attach but before the first load: -4; sf_set_params / sf_params_changed after attach:
    -1; none of them launches anything.  sf_feather_attach and sf_feather_materialise still refuse the render handle.  After
    a load the handle renders and answers as any render handle; a plain RenderEngine in the same process still takes
    set_params and renders."""
    r = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=120)
    print(json.dumps(r, indent=1))
    inv = {"attach_training_handle": "sf_feather_attach", "attach_fourier_render": "SIREN render handles",
           "attach_twice": "already has a feather state", "attach_wrong_layers": "n_layers must equal the handle's depth",
           "attach_small_n": "n^2 >= the parameter count", "attach_m_above_n": "1 <= m <= n <= 46340",
           "attach_bad_sizes": "logical layer sizes do not fit the handle",
           "set_params_after_attach": "feather vector", "params_changed_after_attach": "feather vector",
           # what exists keeps its refusals: the training entry points on a render handle, attached or not
           "training_attach_on_render_handle": "render handle", "materialise_on_render_handle": "render handle"}
    for name, needle in inv.items():
        assert r[name]["rc"] == -1 and needle in r[name]["msg"], (name, r[name])
    for name in ("attach_wrong_layers", "attach_small_n", "attach_m_above_n", "attach_bad_sizes", "attach_twice"):
        assert r[name]["msg"].startswith("sf_feather_render_attach: "), r[name]
    state = {"load_before_attach": "sf_feather_render_attach", "load_training_handle": "sf_feather_render_attach",
             "render_before_load": "sf_feather_render_load", "render16_before_load": "sf_feather_render_load"}
    for name, needle in state.items():
        assert r[name]["rc"] == -4 and needle in r[name]["msg"], (name, r[name])
    assert r["launches_before_load"] == 0                       # every refusal came before the device
    for name, v in r.items():
        if name.startswith("ok_"):
            assert v["rc"] == 0, (name, v)
    assert "siren_fit error -1" in r["binding_set_params"] and "feather vector" in r["binding_set_params"]
    assert "n^2 >= the parameter count" in r["binding_bad_size"]
    assert r["binding_feather_elems"] == 1888
    assert r["plain_levels"] > 16                               # a plain RenderEngine still takes set_params and renders


def test_fit_then_decode(tmp_path):
    """`python -m implicit_image.fit masking=Feathermap quant=none` (64x4, 64x64, 50 steps), then `python -m
    implicit_image.decode decode.dir=<run> decode.truth=synthetic`: decoded.ppm is to_u8 of the prediction of a FeatherNet
    reloaded from model.pth; decode.metrics on that prediction equals the printed figures exactly (the same function on
    bit-identical input); the PSNR agrees with result.json within 1e-3 dB (the engine's fp32-square / double-sum SSE against
    a float64 sum over the same residuals: a relative difference of the loss of order 1e-6, under 1e-5 dB).  A window, a
    banded decode, decode.bits=16 and decode.render=torch of the same run give the same samples."""
    r = run_case(CHILD, "e2e", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["keys"][:2] == ["_V1", "_V2"] and len(r["keys"]) == 2 + 8
    assert "model.pth" in r["files"] and "decode.json" in r["files"] and "model_quantized" not in r["files"]
    assert r["ppm_equal"] and r["levels"] > 16
    assert r["printed"] == {k: r["metrics_on_reloaded"][k] for k in ("loss", "PSNR", "PSNR_8bit")}
    assert abs(r["printed"]["PSNR"] - r["result_psnr"]) <= 1e-3, (r["printed"]["PSNR"], r["result_psnr"])
    assert r["window_equal"] and r["window_size"] == [16, 36]
    assert r["band_equal"] and r["bits16_equal"]
    assert r["kernel_path"] == ["kernel", "Feathermap 64x4: sf_feather_render_load + sf_render", "pth"]
    assert r["torch_equal"] and r["torch_path"] == "torch"


def test_render_handle_memory(tmp_path):
    """128x8, density 0.2 (n 316, m 32: 20 240 floats of feather vector) at 1024x1024, each handle in a fresh process: the
    feather render handle takes less device memory than the training handle with sf_feather_attach, at most two 2 MiB
    allocation granules more than a plain RenderEngine of the same shape, and after close() the free memory is back within
    one granule of the reading before create (second round; GRANULE / SLACK of tests/test_gpu_handle_memory.py, whose note
    that the runtime's own shortfall is still unmeasured applies here too)."""
    fr = run_case(CHILD, "mem", "feather_render", tmp_path=tmp_path, timeout=120)
    rn = run_case(CHILD, "mem", "render", tmp_path=tmp_path, timeout=120)
    tr = run_case(CHILD, "mem", "train", tmp_path=tmp_path, timeout=120)
    print({"feather_render": fr, "render": rn, "train": tr})
    assert fr["feather_elems"] == 20240
    assert 0 <= fr["taken"] < tr["taken"]
    assert fr["taken"] - rn["taken"] <= 2 * GRANULE
    assert fr["levels"] > 16 and fr["shortfall"] <= SLACK
