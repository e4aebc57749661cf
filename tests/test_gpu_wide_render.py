"""The wide render handle (sf_wide_render_create / sf_wide_render / sf_wide_render16: the RENDER forms of k_wlayer0, k_wgemm2
and k_wgemm, csrc/siren_wide.hip) and decode.render=wide on an MI355X.  One case of tests/_wide_render_child.py per child
process."""
import json

import pytest

from _gpu_child import run_case
from _gpu_fixtures import TRAINING_CALLS

pytestmark = pytest.mark.gpu
CHILD = "_wide_render_child.py"
SHAPES = [(512, 3), (512, 4), (1024, 3), (1024, 5)]
MIB = 1 << 20


@pytest.fixture(scope="module")
def bitid(tmp_path_factory):
    """every row of the bit-identity matrix, one child per shape"""
    tmp = tmp_path_factory.mktemp("wide_bitid")
    return [row for hid, dep in SHAPES for row in run_case(CHILD, "bitid", str(hid), str(dep), tmp_path=tmp, timeout=300)["cases"]]


def test_wide_render_pred_is_bit_identical_to_the_training_forward(bitid):
    """(hidden, depth) in {(512,3), (512,4), (1024,3), (1024,5)} x {1x1, 5x7, 67x45, 512x512, 1031x517 in 64 Ki-pixel chunks} x
    outermost_linear True / False, with out_features 1 and 3 at depth 3 and bf16 operands at (512, 4), at the SIREN
    initialisation and with a scaled output layer: torch.equal(sf_wide_render's pred on the render handle, sf_forward's pred on
    a training handle), whichever outputs the call writes.  No tolerance: the weight images, the MFMA chain and v_sin_f32 are
    the same on both sides.  512x512 gives every persistent workgroup of k_wgemm2 several tiles, the one path on which the
    wait that counts a tile's epilogue stores is used."""
    per_shape = {(512, 3): 5 * 2 * 2 * 1, (512, 4): 5 * 2 * 1 * 2, (1024, 3): 5 * 2 * 2 * 1, (1024, 5): 5 * 2 * 1 * 1}
    for (hid, dep), n in per_shape.items():
        assert len([c for c in bitid if (c["hidden"], c["depth"]) == (hid, dep)]) == n * 2, (hid, dep)
    assert len(bitid) == 140
    assert {(c["H"], c["W"], c["chunk"]) for c in bitid} == {(1, 1, 0), (5, 7, 0), (67, 45, 0), (512, 512, 0), (1031, 517, 65536)}
    assert [c for c in bitid if c["dtype"] == "bf16"] and all((c["hidden"], c["depth"]) == (512, 4) for c in bitid if c["dtype"] == "bf16")
    bad = [c for c in bitid if not (c["pred_equal"] and c["pred16_equal"] and c["pred_only_equal"] and c["finite"])]
    assert not bad, bad[:4]
    assert all(c["render_format"] == 16 for c in bitid)


def test_wide_render_samples_equal_the_conversion_of_the_kernels_own_prediction(bitid):
    """rgb8 == min(max(trunc(pred * 255), 0), 255) and rgb16 == min(max(trunc(pred * 65535), 0), 65535) of the kernel's fp32
    output, exactly, and the same whether or not pred is also written.  With a linear output layer scaled by 400 (zero output
    bias) every case of more than one pixel has predictions below 0 and above 1, so both clamps are hit; a sine output layer
    cannot leave [0, 1]."""
    bad = [c for c in bitid if not (c["u8_equal"] and c["u8_only_equal"] and c["u16_equal"] and c["u16_only_equal"])]
    assert not bad, bad[:4]
    for c in bitid:
        if c["linear"] and c["scale"] > 1 and c["H"] * c["W"] > 1:
            assert c["below0"] > 0 and c["above1"] > 0, c
        if not c["linear"]:
            assert c["pmin"] >= 0.0 and c["pmax"] <= 1.0, c


def test_training_handles_of_every_scratch_format_give_the_same_prediction(tmp_path):
    """(512, 4) at 512x512, fp16: sf_forward on training handles of scratch_format 16, 12 and 8 equals the render handle's
    pred bit for bit - the formats change the phases, which a forward never reads back, not the activations"""
    r = run_case(CHILD, "formats", tmp_path=tmp_path, timeout=180)
    print(r)
    assert sorted(r) == ["12", "16", "8"]
    for fmt, c in r.items():
        assert c["format"] == int(fmt) and c["pred_equal"], (fmt, c)


def test_ragged_pictures_stay_inside_their_buffers(tmp_path):
    """5x7 (105 bytes, a ragged last dword, and an odd sample count at 16 bits), 1x1, 3x3 at one channel and 9x29 at hidden
    512 and 1024: the samples equal the conversion of pred and the 64 sentinel bytes behind every buffer are intact"""
    rows = run_case(CHILD, "guards", tmp_path=tmp_path, timeout=180)["cases"]
    assert len(rows) == 5 * 2
    for c in rows:
        assert c["rc"] == [0, 0, 0, 0] and c["finite"], c
        assert c["u8_equal"] and c["u8_alone_equal"] and c["u16_equal"] and c["u16_alone_equal"], c
        assert c["guards_intact"], c


def test_wide_render_against_the_fp64_oracle(tmp_path):
    """(512, 3) at 64x64 from the oracle's seeded initialisation: max |pred - oracle.forward| < 5e-4, the bound smoke() and
    test_wide_vs_oracle hold the forward of fp16 operands to, and the byte image differs from the oracle's by at most one
    level anywhere."""
    r = run_case(CHILD, "oracle", tmp_path=tmp_path, timeout=120)
    print(r)
    assert r["max_abs"] < 5e-4
    assert r["max_levels"] <= 1
    assert r["u16_equal"] and r["distinct_levels"] > 16


def test_refusals_come_before_anything_is_launched(tmp_path):
    """argument checks that return an error code with a message; the profile of every handle involved counts no launch"""
    r = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=180)
    print(json.dumps(r, indent=1))
    assert r["create_256"]["rc"] == -1 and "sf_render_create" in r["create_256"]["msg"] and r["create_256_handle_null"]
    for name in ("wide_render_on_narrow_render_handle", "wide_render16_on_narrow_render_handle"):
        assert r[name]["rc"] == -1 and "sf_wide_render_create" in r[name]["msg"] and "sf_render draws" in r[name]["msg"], r[name]
    c = r["wide_render_on_wide_training_handle"]
    assert c["rc"] == -1 and "sf_wide_render_create" in c["msg"] and "sf_forward" in c["msg"], c
    assert r["launches_narrow"] == 0 and r["launches_train"] == 0 and r["launches_render"] == 0
    for name in TRAINING_CALLS + ["sf_set_target"]:
        assert r[name]["rc"] == -1, (name, r[name])
        assert "render handle" in r[name]["msg"], (name, r[name])
    # sf_render keeps render_any's answer for a wide handle, of either kind
    for name in ("sf_render_on_wide_render_handle", "sf_render16_on_wide_render_handle", "sf_render_on_wide_training_handle"):
        assert r[name]["rc"] == -1 and "built for SIREN handles of hidden width 32 .. 256" in r[name]["msg"], r[name]
    assert r["sf_feather_render_attach"]["rc"] == -1 and "sf_wide_render_create" in r["sf_feather_render_attach"]["msg"]
    assert r["before_coords"]["rc"] == -4 and "sf_set_coords" in r["before_coords"]["msg"]
    for name in ("both_null", "both_null16"):
        assert r[name]["rc"] == -1 and "both NULL" in r[name]["msg"], r[name]
    for name in ("odd_base", "two_byte_base16"):
        assert r[name]["rc"] == -1 and "4-byte aligned" in r[name]["msg"], r[name]
    assert r["null_handle"]["rc"] == -1
    for name, v in r.items():
        if name.startswith("ok_"):
            assert v["rc"] == 0, (name, v)
    P = 2 * 512 + 512 + 2 * (512 * 512 + 512) + 3 * 512 + 3
    assert r["offsets"] == [2 * 512 + 512, 2 * 512 + 512 + 512 * 512, P] and r["format"] == 16
    # two renders of one chunk at depth 4: k_wlayer0, two hidden products and the last layer each, all under k_render
    assert r["k_render_launches"] == 2 * 4 and r["other_launches"] == 0


def test_wide_render_handle_memory(tmp_path):
    """512x4 at 1024x1024, each handle in a fresh process: the render handle takes at most two activation planes of the
    default chunk (2^18 pixels x 512 x 2 B each), the two hidden forward images (512^2 x 2 B each) and 16 MiB for everything
    else; the training handle's figure is printed beside it and is larger."""
    tr = run_case(CHILD, "mem", "train", tmp_path=tmp_path, timeout=180)
    rn = run_case(CHILD, "mem", "render", tmp_path=tmp_path, timeout=180)
    chunk = 1 << 18
    bound = 2 * chunk * 512 * 2 + 2 * 512 * 512 * 2 + 16 * MIB
    print({"train_MiB": tr["taken"] / MIB, "render_MiB": rn["taken"] / MIB, "bound_MiB": bound / MIB})
    assert 0 < rn["taken"] <= bound
    assert rn["taken"] < tr["taken"]


@pytest.mark.parametrize("tag", ["pth", "container", "padded"])
def test_fit_then_decode_wide_end_to_end(tmp_path, tag):
    """fit_one (engine width 512, depth 3, synthetic 64x64, 30 steps, masking=none; model.pth, the plain k-means container,
    and mlp.hidden_size=300 zero-padded to 512) -> decode: decode.render=wide and decode.render=torch write byte-identical
    PPMs at 8 and 16 bits, on the kernel against the torch path; without decode.render the run still decodes on torch.  A
    window (rows 8:40, cols 4:36) equals that region of the full render, band_rows=7 the one-band file."""
    r = run_case(CHILD, "e2e", tag, tmp_path=tmp_path, timeout=600)
    print(json.dumps(r, indent=1))
    assert r["wide_path"] == "kernel" and r["wide16_path"] == "kernel" and r["torch_path"] == "torch" and r["auto_path"] == "torch"
    assert r["source"] == ("container" if tag == "container" else "pth")
    assert r["wide_why"] == ("SIREN 512x3 (width 300 zero-padded): sf_wide_render" if tag == "padded" else "SIREN 512x3: sf_wide_render")
    assert r["files8_identical"] and r["files16_identical"] and r["auto_identical"] and r["header16_ok"]
    assert r["levels"] > 16                       # a picture, not a constant
    if tag != "padded":
        assert r["window_path"] == "kernel" and r["window_shape"] == [32, 32]
        assert r["window_equal"] and r["band_identical"] and r["window16_equal"]
