"""sf_mask_prune_global on an MI355X (csrc/siren_mask.hip): the global-magnitude update of masking=Pruning as one device call.
One case of tests/_prune_global_child.py per child process; the contract the kernels are held to is
tests/_prune_global_ref.py."""
import json

import pytest

import _prune_global_child as child  # (the shape lists only: nothing touches the device at import)
from _gpu_child import run_case
from _prune_global_ref import TRIAL_CAP

pytestmark = pytest.mark.gpu
CHILD = "_prune_global_child.py"


@pytest.mark.parametrize("which", range(len(child.HANDLES)), ids=[f"{h}x{d}" for h, d in child.HANDLES])
def test_abi_against_the_restatement(which, tmp_path):
    """Handles on an 8x8 image whose layers reach every size class of the kernels (128 .. 2^20 elements).  State from seeded
    CPU tensors through sf_set_params / sf_set_masks / sf_set_grads / sf_set_adam_state.  A search from the shipped start
    threshold with dense_gradients 0 / 1, half the network pruned, target 0, a target above `alive` (the count saturates, the
    stall break ends the search), weights quantised to 2^-7 (the count jumps over the target), a start threshold equal to a
    weight (strict >: one trial), start thresholds three decades above and below, a layer list without layer 0, an all-zero
    network.  All five state vectors bit for bit (int32 views: -0.0 counts) and every row, the status row included, equal the
    restatement's; a second run on the same state gives the same bits; the trials stay below the cap."""
    hidden, depth = child.HANDLES[which]
    r = run_case(CHILD, "abi", str(which), tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1)[:20000])
    assert r["sizes"] == [2 * hidden] + [hidden * hidden] * (depth - 2) + [3 * hidden]
    v = r["variants"]
    assert len(v) == 11
    for name, c in v.items():
        assert c["diff"] == {"w": 0, "g": 0, "m": 0, "v": 0, "k": 0}, (name, c["diff"])
        assert c["rows_equal"], (name, c["rows"], c["ref_rows"])
        assert c["repeat"], name
        assert c["status"][0] == (1 if name == "all_zero" else 0), name
        assert 0 <= c["status"][1] < TRIAL_CAP, name
    for name in ("natural_d0", "natural_d1", "half_d0", "from_above", "without_layer0"):
        assert v[name]["status"][1] > 1 and v[name]["masks_changed"] > 0, name
    assert v["natural_d0"]["minus_zero"] > 0 and v["half_d0"]["minus_zero"] > 0       # pruned negative weights become -0.0
    tz = v["target_zero"]["status"]
    assert tz[1] == tz[3] == tz[4] == 0 and tz[2] > 0 and v["target_zero"]["threshold"] == 0.001
    assert v["target_zero"]["masks_changed"] == 0 and sum(v["target_zero"]["removed"]) == 0
    assert v["target_above_alive"]["status"][3] == v["target_above_alive"]["status"][2] > 0 and v["target_above_alive"]["status"][1] >= 10
    q = v["quantised"]["status"]
    assert abs(q[3] - q[4]) > q[4] * 1e-6 and q[1] > 10                                # ended by stalling, off the target
    assert v["strict"]["status"][1] == 1 and v["strict"]["status"][3] == r["strict_target"]
    assert v["from_below"]["status"][1] >= 10                      # (ten equal counts at the least, or a long walk up)
    assert len(v["without_layer0"]["removed"]) == depth - 1
    assert v["all_zero"]["untouched"] and v["all_zero"]["threshold"] == 0.001


@pytest.mark.parametrize("dense", ["1", "0"], ids=["dense_gradients", "sparse_gradients"])
@pytest.mark.parametrize("which", range(len(child.HOST_SHAPES)), ids=[f"{h}x{d}" for h, d in child.HOST_SHAPES])
def test_device_route_against_the_host_path(which, dense, tmp_path):
    """Two Siren models from the same seed under conf/masking/Pruning.yaml's keys (on a schedule that prunes at every one of
    the four updates), one with SIREN_FIT_DEVICE_MASK=0 and one on the device route, three train_epoch calls before each
    update.  After every update the masks, params, exp_avg, exp_avg_sq, grads (int32 views), stats, name2prune_rate,
    adjustments and prune_threshold (bit for bit) are equal, and so are the next three losses.  The rule is value-based:
    there is no tie exception."""
    r = run_case(CHILD, "host", str(which), dense, tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["device_updates"] == [0, 4]
    assert len(r["trials"]) == 4 and all(0 < t < TRIAL_CAP for t in r["trials"])
    for u in r["updates"]:
        assert u["losses_equal"] and u["state_equal"] == [True] * 5 and u["masks_equal"], u
        assert u["stats_equal"] and u["rates_equal"] and u["adjustments_equal"] and u["threshold_equal"], u
        assert u["mask_step"][0] == u["mask_step"][1]
    assert r["updates"][-1]["density"] < 0.95
    assert r["next_losses_equal"], r["next_losses"]


@pytest.mark.parametrize("upd", [5, 10])
def test_device_update_against_the_reference(upd, tmp_path):
    """tests/golden/masking_pruning.npz (the real reference's Pruning run on the 64x4 model): its state before the update at
    step `upd` is copied into the engine's views, update_connections() runs as sf_mask_prune_global, and masks, weights
    and exp_avg equal the reference's state after it bit for bit; prune_threshold and adjusted_growth to the rel=1e-12
    tests/test_masking_modes.py holds the host path to."""
    r = run_case(CHILD, "golden", str(upd), tmp_path=tmp_path, timeout=120)
    print(r)
    assert r["init_equal"] and r["device_updates"] == 1 and r["target"] > 0
    assert r["mask_equal"] and r["w_equal"] and r["m_equal"] and r["nnz_equal"] and r["mask_step_equal"]
    assert r["threshold_rel_error"] <= 1e-12 and r["growth_rel_error"] <= 1e-12 and r["density_error"] <= 1e-15


def test_refusals_launch_nothing(tmp_path):
    """every refusal of include/siren_fit.h returns its code with a message that names the entry point, and the profile
    counters of the handle stay at zero; the binding's WaveletEngine / FourierEngine have no mask_prune_global at all"""
    r = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=120)
    print(json.dumps(r, indent=1))
    named = ["render", "fourier", "wavelet", "feather", "layer_out_of_range", "layer_negative", "not_ascending", "descending",
             "no_layers", "too_many_layers", "threshold_zero", "threshold_negative", "threshold_inf", "threshold_nan",
             "increment_zero", "increment_one", "increment_nan", "tolerance_negative", "tolerance_inf", "tolerance_nan",
             "target_negative"]
    for name in named + ["null_handle", "null_args", "null_layers", "wrong_abi"]:
        assert r[name]["rc"] == -1 and r[name]["msg"], (name, r[name])
    for name in named:
        assert "sf_mask_prune_global" in r[name]["msg"], (name, r[name])
    assert r["no_masks"]["rc"] == -4 and "sf_set_masks" in r["no_masks"]["msg"] and "sf_mask_prune_global" in r["no_masks"]["msg"]
    assert set(r["launches_after_refusals"].values()) == {0}
    assert r["binding_wavelet"].startswith("TypeError")
    assert r["ok_update"]["rc"] == 0 and r["ok_without_stats_again"]["rc"] == 0
    assert r["plan_after_two_updates"] == {"k_mask_prune_global": 2}


def test_launch_count_depends_on_neither_depth_nor_trials(tmp_path):
    """the kernels that ran on the device during one update, from torch.profiler's device activity records (the engine's own
    profile keeps one record per call, whatever is launched inside it): the same six launches at depth 3 and depth 8, for
    a search of one trial and for one of more than fifty"""
    r = run_case(CHILD, "launches", tmp_path=tmp_path, timeout=120)
    print(r)
    assert r["3"] == r["8"] == r["few"] == r["many"] == {"k_mask_prune_global": 1}
    six = {"k_mask_count": 1, "k_prune_file": 2, "k_prune_scan": 1, "k_prune_search": 1, "k_prune_apply": 1}
    assert r["kernels_3"] == r["kernels_8"] == r["kernels_few"] == r["kernels_many"] == six
    assert r["trials_8"] > 1
    assert r["trials_few"] == 1 and r["removed_few"] == r["target"]
    assert 50 < r["trials_many"] < TRIAL_CAP


def test_fit_is_byte_equal_on_both_routes(tmp_path):
    """fit_one, masking=Pruning quant=none, 64x4 on 64x64, 60 steps, an update every 10: model.pth of the run with
    SIREN_FIT_DEVICE_MASK=0 and of the run on the device route are the same bytes, result.json the same PSNR, loss and
    density."""
    r = run_case(CHILD, "e2e", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["host"]["device_updates"] == 0 and r["device"]["device_updates"] == 6
    assert r["pth_equal"] and r["pth_bytes"] > 4 * 8000
    for key in ("PSNR", "loss", "PSNR_8bit", "density"):
        assert r["host"][key] == r["device"][key], key
    assert r["device"]["density"] < 1.0
