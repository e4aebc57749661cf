"""sf_mask_update on an MI355X (csrc/siren_mask.hip): the RigL topology update as one device call.  One case of
tests/_mask_update_child.py per child process; the contract the kernels are held to is tests/_mask_update_ref.py."""
import json

import pytest

import _mask_update_child as child  # (the shape lists only: nothing touches the device at import)
from _gpu_child import run_case

pytestmark = pytest.mark.gpu
CHILD = "_mask_update_child.py"


@pytest.mark.parametrize("which", range(len(child.HANDLES)), ids=[f"{h}x{d}" for h, d in child.HANDLES])
def test_abi_against_the_restatement(which, tmp_path):
    """Handles on an 8x8 image whose layers reach every size class of the kernels: shorter than one workgroup (64, 96
    elements), a few 64-element steps per wave (1024 .. 4096), the 65 536-element layer of the metric width, the 262 144 of
    the wide path.  State from seeded CPU tensors through sf_set_params / sf_set_masks / sf_set_grads / sf_set_adam_state.
    Continuous values and values quantised to 0.5 (heavy ties, live zeros, more zeros than dead + drop), rate 0 / 0.1 /
    0.3, growth 0 / 1, dense_gradients 0 / 1, the largest layer wholly live (nothing of it changes) or 90 % live (the rate
    cap), a growth budget above the non-zero candidates, a layer list without layer 0.  All five state vectors bit for bit
    (int32 views: -0.0 counts) and every statistics row equal the restatement's; a second run on the same state gives the
    same bits."""
    hidden, depth = child.HANDLES[which]
    r = run_case(CHILD, "abi", str(which), tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1)[:20000])
    assert r["sizes"] == [2 * hidden] + [hidden * hidden] * (depth - 2) + [3 * hidden]
    v = r["variants"]
    assert len(v) == 28
    for name, c in v.items():
        assert c["diff"] == {"w": 0, "g": 0, "m": 0, "v": 0, "k": 0}, (name, c["diff"])
        assert c["rows_equal"], (name, c["rows"], c["ref_rows"])
        assert c["repeat"], name
        assert c["status"] == [0] * 8, name
    assert all(c["tied"] for name, c in v.items() if name.startswith("q_r0.3"))       # the quantised layers split groups of ties
    assert not any(c["tied"] for name, c in v.items() if name.startswith("c_"))
    assert all(sum(c["removed"]) == 0 for name, c in v.items() if "_r0.0_" in name)
    assert all(min(c["removed"]) > 0 for name, c in v.items() if name.startswith("c_r0.3"))
    assert v["c_r0.3_g1_d0"]["minus_zero"] > 0                                        # pruned negative weights become -0.0
    assert v["all_live"]["big_rate"] == 0.0 and v["all_live"]["big_removed"] == 0
    assert 0.0 < v["capped"]["big_rate"] < 0.2 and v["capped"]["big_removed"] > 0
    assert v["few_candidates"]["tied"] and len(v["without_layer0"]["removed"]) == depth - 1
    assert r["all_zero"] == {"status": 1, "untouched": True}


@pytest.mark.parametrize("dense", ["1", "0"], ids=["dense_gradients", "sparse_gradients"])
@pytest.mark.parametrize("density", ["0.5", "0.2"])
@pytest.mark.parametrize("which", range(len(child.HOST_SHAPES)), ids=[f"{h}x{d}_{s}" for h, d, s in child.HOST_SHAPES])
def test_device_route_against_the_host_path(which, density, dense, tmp_path):
    """Two Siren models from the same seed under conf/masking/RigL.yaml's configuration, one with SIREN_FIT_DEVICE_MASK=0 and
    one on the device route: four updates with three train_epoch calls before each.  After every update the masks, params,
    exp_avg, exp_avg_sq, grads (int32 views), stats, name2prune_rate and adjustments are equal, and so are the next three
    losses.  The child also works out from the host side's tensors whether any selection boundary was tied - the one case
    in which the two routes may differ: a tied boundary fails the test, it is not skipped."""
    r = run_case(CHILD, "host", str(which), density, dense, tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["device_updates"] == [0, 4]
    assert r["tied"] == [False] * 4
    for u in r["updates"]:
        assert u["losses_equal"] and u["state_equal"] == [True] * 5 and u["masks_equal"], u
        assert u["stats_equal"] and u["rates_equal"] and u["adjustments_equal"], u
        assert u["mask_step"][0] == u["mask_step"][1]
    assert r["next_losses_equal"], r["next_losses"]


@pytest.mark.parametrize("upd", [5, 10])
def test_device_update_against_the_reference(upd, tmp_path):
    """tests/golden/masking_rigl.npz (the real reference's RigL run on the 64x4 model, make_golden_rigl_update.py): its
    state before the update at step `upd` is copied into the engine's views, update_connections() runs as sf_mask_update,
    and masks, weights and exp_avg equal the reference's state after it bit for bit."""
    r = run_case(CHILD, "golden", str(upd), tmp_path=tmp_path, timeout=120)
    print(r)
    assert r["init_equal"] and r["rate_error"] <= 1e-15 and r["device_updates"] == 1
    assert r["mask_equal"] and r["w_equal"] and r["m_equal"] and r["nnz_equal"] and r["mask_step_equal"]
    assert r["growth_error"] <= 1e-12 and r["density_error"] <= 1e-15


def test_refusals_launch_nothing(tmp_path):
    """every refusal of include/siren_fit.h returns its code with a message that names the entry point, and the profile
    counters of the handle stay at zero; the binding's WaveletEngine / FourierEngine have no mask_update at all"""
    r = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=120)
    print(json.dumps(r, indent=1))
    invalid = ["render", "fourier", "wavelet", "feather", "null_handle", "null_args", "null_layers", "wrong_abi",
               "layer_out_of_range", "layer_negative", "not_ascending", "descending", "no_layers", "too_many_layers", "growth_2",
               "growth_negative"]
    for name in invalid:
        assert r[name]["rc"] == -1 and r[name]["msg"], (name, r[name])
    for name in ("render", "fourier", "wavelet", "feather", "layer_out_of_range", "not_ascending", "growth_2", "no_layers"):
        assert "sf_mask_update" in r[name]["msg"], (name, r[name])
    assert r["no_masks"]["rc"] == -4 and "sf_set_masks" in r["no_masks"]["msg"]
    assert set(r["launches_after_refusals"].values()) == {0}
    assert r["binding_wavelet"].startswith("TypeError")
    assert r["ok_update"]["rc"] == 0 and r["ok_without_stats_again"]["rc"] == 0
    assert r["plan_after_two_updates"] == {"k_mask_update": 2}


def test_launch_count_does_not_depend_on_the_depth(tmp_path):
    r = run_case(CHILD, "launches", tmp_path=tmp_path, timeout=120)
    print(r)
    assert r["3"] == r["8"] == {"k_mask_update": 1}


def test_fit_is_byte_equal_on_both_routes(tmp_path):
    """fit_one, masking=RigL quant=none, 64x4 on 64x64, 60 steps, an update every 10: model.pth of the run with
    SIREN_FIT_DEVICE_MASK=0 and of the run on the device route are the same bytes, result.json the same PSNR, loss and
    density."""
    r = run_case(CHILD, "e2e", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["host"]["device_updates"] == 0 and r["device"]["device_updates"] == 6
    assert r["pth_equal"] and r["pth_bytes"] > 4 * 8000
    for key in ("PSNR", "loss", "PSNR_8bit", "density"):
        assert r["host"][key] == r["device"][key], key
    assert 0.3 < r["device"]["density"] < 0.7
