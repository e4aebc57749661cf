"""The inference-only FourierNet render path (sf_fourier_render_create / sf_render on FourierNet handles,
csrc/fourier_render.hip) and `decode decode.render=kernel` on an MI355X.  One case of tests/_fourier_render_child.py per
child process."""
import json

import pytest

import _fourier_render_child as child  # (the shape lists only: nothing touches the device at import)
from _gpu_child import run_case
from _gpu_fixtures import TRAINING_CALLS

pytestmark = pytest.mark.gpu
CHILD = "_fourier_render_child.py"


@pytest.fixture(scope="module")
def bitid(tmp_path_factory):
    return run_case(CHILD, "bitid", tmp_path=tmp_path_factory.mktemp("fourier_bitid"), timeout=300)["cases"]


def test_every_shape_ran(bitid):
    """hidden 32 / 64 / 128 / 256 x map 64 / 512 (and 128 / 256 at hidden 128) x 2 / 3 / 5 Linear layers x pictures 1x1, 5x7,
    33x31, 64x64, 37x300 x chunk_pixels 0 / 256: every combination, none left out; map 512 at hidden 256 streams the first
    weight image in slices, 2 layers have no hidden-to-hidden layer, 256-pixel chunks give several chunks and a ragged
    last one.  Seeded random parameters, B = randn * 16."""
    want = child.shapes()
    assert len(want) == (4 * 2 + 2) * 3 * 5 * 2 == 300
    got = [((c["hidden"], c["map_size"]), c["n_linear"], (c["H"], c["W"]), c["chunk"]) for c in bitid]
    assert got == want
    assert all(c["rc"] == 0 and c["finite"] for c in bitid)
    # the parameters give pictures, not constants: the larger grids spread over many byte levels
    assert all(c["levels"] > 16 for c in bitid if c["H"] * c["W"] >= 1023), [c for c in bitid if c["levels"] <= 16][:3]


def test_render_pred_is_bit_identical_to_sf_forward(bitid):
    """torch.equal(sf_render's pred on a render handle, sf_forward's pred on a training handle with the same parameters,
    encoding and coordinates): no tolerance.  The same for pred alone (no byte buffer) and for sf_render on the training
    handle itself."""
    bad = [c for c in bitid if not (c["pred_equal"] and c["pred_only_equal"] and c["train_pred_equal"])]
    assert not bad, bad[:4]


def test_render_bytes_equal_to_u8_of_the_prediction(bitid):
    """rgb8 == decode.to_u8(sf_forward's pred) exactly; bytes alone, bytes with pred and bytes from the training handle agree;
    the 16 pattern bytes behind the byte buffer are untouched (1x1 is a 3-byte picture, 5x7 ends in a ragged dword, 33x31
    and 37x300 end in a ragged 32-pixel block)."""
    bad = [c for c in bitid if not (c["u8_equal"] and c["u8_only_equal"] and c["train_u8_equal"])]
    assert not bad, bad[:4]
    bad = [c for c in bitid if not c["guard_intact"]]
    assert not bad, bad[:4]


def test_windows_and_bands_equal_the_full_render(tmp_path):
    """rows=32:96 cols=16:80 of a 128x128 grid == that region of the full 128x128 render, bytes and pred; band_rows=7 == one
    band"""
    r = run_case(CHILD, "windows", tmp_path=tmp_path, timeout=120)
    print(r)
    assert r["shape"] == [128, 128, 3]
    assert r["window_equal"] and r["window_pred_equal"]
    assert r["band_equal"] and r["band_pred_equal"]
    assert r["distinct_levels"] > 16          # a picture, not a constant


def test_render_handle_refusals(tmp_path):
    """every training call (TRAINING_CALLS) on a FourierNet render handle: -1 with "render handle" in the
    message; sf_render before sf_set_encoding / sf_set_coords: SF_ERR_STATE (-4); both outputs NULL, an unaligned byte
    pointer and sf_wavelet_render: -1.  The handle's profile counts no launch over all of them."""
    r = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=120)
    for name in TRAINING_CALLS + ["sf_set_target"]:
        assert r[name]["rc"] == -1, (name, r[name])
        assert "render handle" in r[name]["msg"], (name, r[name])
    assert r["before_anything"]["rc"] == -4 and r["before_coords"]["rc"] == -4
    assert "sf_set_coords" in r["before_coords"]["msg"]
    assert r["before_encoding"]["rc"] == -4 and "sf_set_encoding" in r["before_encoding"]["msg"]
    assert r["sf_render_both_null"]["rc"] == -1 and "NULL" in r["sf_render_both_null"]["msg"]
    assert r["sf_render_misaligned"]["rc"] == -1 and "aligned" in r["sf_render_misaligned"]["msg"]
    assert r["sf_wavelet_render"]["rc"] == -1 and "WaveletSiren" in r["sf_wavelet_render"]["msg"]
    assert r["launches_state_a"] == 0 and r["launches_state_b"] == 0
    for name, v in r.items():
        if name.startswith("ok_"):
            assert v["rc"] == 0, (name, v)
    assert r["num_params"] == 64 * 64 + 64 + 64 * 64 + 64 + 3 * 64 + 3
    assert r["k_ff_render_launches"] == 1 and r["k_fwd_launches"] == 0
    for name in ("create_hidden", "create_map", "create_layers", "create_bf16", "create_abi"):
        assert r[name]["rc"] == -1 and r[name]["handle_null"] and r[name]["same_as_train"], (name, r[name])


def test_render_handle_memory(tmp_path):
    """128 hidden, 7 Linear layers, map 256 at 1024x1024, each handle in a fresh process: the render handle takes less
    device memory than the training handle by at least the ffH + ffG + ffZ planes of sf_fourier_create,
    2 (D - 1) WD chunk 2 + 8 chunk bytes with chunk = 2^20, and its own footprint is under 64 MiB."""
    tr = run_case(CHILD, "mem", "train", tmp_path=tmp_path, timeout=120)
    rn = run_case(CHILD, "mem", "render", tmp_path=tmp_path, timeout=120)
    m = child.MEM
    chunk = m["height"] * m["width"]
    planes = 2 * (m["n_linear"] - 1) * m["hidden"] * chunk * 2 + 8 * chunk
    print({"train": tr, "render": rn, "planes": planes})
    assert planes == 3229614080
    assert tr["taken"] - rn["taken"] >= planes
    assert 0 <= rn["taken"] < (64 << 20)


def test_fit_then_decode_kernel_against_torch(tmp_path):
    """fit_one (mlp=fourier masking=none quant=none, 64x64, 30 steps) -> decode with decode.render=kernel against
    decode.render=torch: the PPMs are identical byte for byte, `path` is "kernel" against "torch", and with
    decode.truth=synthetic the three printed figures are equal - at the fitted size, at decode.height=96 decode.width=80,
    for a window with decode.band_rows=5, and for a Small_Dense density-0.5 fit (width 90 zero-padded to 128).
    decode.render=auto still reports "torch" for the run."""
    r = run_case(CHILD, "e2e", tmp_path=tmp_path, timeout=600)
    print(json.dumps(r, indent=1))
    pairs = [r["none"]["fitted"], r["none"]["resized"], r["none"]["window"], r["small_dense"]["fitted"]]
    for c in pairs:
        assert c["paths"] == ["kernel", "torch"], c
        assert c["ppm_identical"], c
        assert c["figures_kernel"] == c["figures_torch"], c
    assert r["none"]["fitted"]["size"] == [64, 64] and r["none"]["resized"]["size"] == [96, 80]
    assert r["none"]["window"]["size"] == [40, 61]
    assert (r["small_dense"]["logical_width"], r["small_dense"]["engine_width"]) == (90, 128)
    assert r["none"]["auto_path"] == "torch" and r["none"]["auto_identical"]
